// spg — variable-base MSM (msm_var.hip): what the device pipeline and the host share.
//   * the signed c-bit recode and the bucket key, one SPG_HD function each (the kernels, the host path and the
//     CPU-checkable emulation in hostcheck.cpp call the same code);
//   * the window choice;
//   * the host side: bucket fill from (key, entry) pairs in the device's group layout (host path and emulation),
//     and the finish over the group sums W_g, G_g -- window sums, Horner with c doublings per window, encoding.
//
// Layout. MSM b of a batch, window w (W = 253 / c + 1 of them), digit d != 0 goes to bucket
//   key = (b W + w) NB + |d| - 1,  NB = 2^(c-1),
// as the entry (point index | sign << 31). Buckets reduce in groups of GS = min(64, NB) consecutive keys: group g
// holds W_g = sum_j (j + 1) B_{GS g + j} and G_g = sum_j B_{GS g + j} at groups[2 g], groups[2 g + 1].
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "curve.hpp"

namespace spg {

constexpr int kVmsmCMin = 4, kVmsmCMax = 14;
constexpr int kVmsmGroupMax = 64;

SPG_HD int vmsm_windows(int c) { return 253 / c + 1; }
SPG_HD int vmsm_group(int c) { return (1 << (c - 1)) < kVmsmGroupMax ? (1 << (c - 1)) : kVmsmGroupMax; }

// digit w of the canonical scalar k (8 x u32, < 2^253) in signed c-bit form: the window's bits plus the carry of the
// window below; a digit above NB = 2^(c-1) becomes d - 2^c and carries one up (the recode of k_big_digits / emit_digits)
SPG_HD int vmsm_digit(const uint32_t k[8], int c, int w, int& carry) {
  const int bit = w * c, li = bit >> 5, of = bit & 31;
  uint32_t lo = 0, hi = 0;  // limbs li and li + 1 by selection: a runtime index would put k into scratch memory
  for (int j = 0; j < 8; j++) {
    lo = j == li ? k[j] : lo;
    hi = j == li + 1 ? k[j] : hi;
  }
  const uint32_t v = (uint32_t)((((uint64_t)hi << 32) | lo) >> of);
  int d = (int)(v & ((1u << c) - 1u)) + carry;
  carry = d > (1 << (c - 1)) ? 1 : 0;
  return d - (carry << c);
}
// bucket of digit d != 0 of window w of MSM b
SPG_HD uint32_t vmsm_key(uint32_t b, int w, int d, int c) {
  return (b * (uint32_t)vmsm_windows(c) + (uint32_t)w) * (1u << (c - 1)) + (uint32_t)((d < 0 ? -d : d) - 1);
}
SPG_HD uint32_t vmsm_entry(uint32_t point, int d) { return point | (d < 0 ? 0x80000000u : 0u); }

// affine Niels form of a decompressed ristretto point (Z = 1, T = x y: no inversion), as k_points_load writes it
SPG_HD Niels vmsm_niels_affine(const Ext& P) {
  Niels n;
  n.ypx = fp_canon(fp_add(P.Y, P.X));
  n.ymx = fp_canon(fp_sub(P.Y, P.X));
  n.t2d = fp_canon(fp_mul(P.T, c_d2()));
  return n;
}

}  // namespace spg

// ---- host side
#include <functional>
#include <vector>

#include "hcurve.hpp"
#include "hpool.hpp"
#include "knobs.hpp"

namespace spg {

// Window width for B MSMs of N points in all, from the points per MSM n = N / B: a table read off the SPG_VMSM_C
// sweep on MI355X (c = 4 .. 14 at 2^10, 2^13 and 2^16 .. 2^20; DESIGN.md 3.3, profiles/vmsm_sizes.json). An entry costs
// ~0.10 ns and a bucket ~26 ns of whole-chip time (a bucket is a workgroup's LDS tree and its share of a group
// reduction, an entry one lane's addition), so W (n + 150 NB) orders the small windows well: c = 4 below 2^12, 5 to
// 2^13, then 6 and 7 (2^14 and 2^15, not swept). From 2^16 the sweep itself decides, since c = 9 and 10 run well
// above their neighbours at every swept size and no such model has that dip: c = 8 is best at 2^16, 2^17 and 2^18 and
// within 1 % of the best at 2^19, c = 11 at 2^20 (and stays above it: not swept). SPG_VMSM_C forces c.
inline int vmsm_choose_c(size_t N, size_t B) {
  const int forced = knob::vmsm_c();
  if (forced) return forced < kVmsmCMin ? kVmsmCMin : (forced > kVmsmCMax ? kVmsmCMax : forced);
  const size_t n = N / (B ? B : 1);
  if (n < ((size_t)1 << 12)) return 4;
  if (n < ((size_t)1 << 14)) return 5;
  if (n < ((size_t)1 << 15)) return 6;
  if (n < ((size_t)1 << 16)) return 7;
  if (n < ((size_t)3 << 18)) return 8;
  return 11;
}

inline h::HNiels vmsm_hniels(const Niels& q) {
  return h::HNiels{h::fe_from_fp(q.ypx), h::fe_from_fp(q.ymx), h::fe_from_fp(q.t2d)};
}
inline h::HNiels vmsm_hniels_neg(const h::HNiels& q) { return h::HNiels{q.ymx, q.ypx, h::fe_neg(q.t2d)}; }

// The bucket stage on the host, in the device's layout: MSM b sums lens[b] points pts[offs[b] + i] (affine Niels,
// canonical, as k_points_load writes them) with the Montgomery scalars s[soff_b + i] (concatenated in b order).
// Every (key, entry) pair lands in its bucket; the buckets of each group then give W_g and G_g. One pool task per
// (MSM, window). groups: 2 B W (NB / GS) points.
inline void vmsm_host_groups(const Niels* pts, const size_t* offs, const size_t* lens, size_t B, const Fq* s, int c,
                             std::vector<h::HExt>& groups) {
  const int W = vmsm_windows(c), NB = 1 << (c - 1), GS = vmsm_group(c), NGW = NB / GS;
  std::vector<size_t> soff(B + 1, 0);
  for (size_t b = 0; b < B; b++) soff[b + 1] = soff[b] + lens[b];
  // digits first (the carry runs up the windows of one scalar)
  std::vector<int16_t> dig((size_t)W * soff[B]);
  for (size_t i = 0; i < soff[B]; i++) {
    const Fq k = fq_from_mont(s[i]);
    int carry = 0;
    for (int w = 0; w < W; w++) dig[(size_t)w * soff[B] + i] = (int16_t)vmsm_digit(k.l, c, w, carry);
  }
  groups.assign(2 * B * (size_t)W * NGW, h::hext_identity());
  pool().parallel_for((int)(B * W), [&](int bw) {
    const size_t b = (size_t)bw / W;
    const int w = bw % W;
    const uint32_t key0 = vmsm_key((uint32_t)b, w, 1, c);
    std::vector<h::HExt> bk(NB, h::hext_identity());
    for (size_t i = 0; i < lens[b]; i++) {
      const int d = dig[(size_t)w * soff[B] + soff[b] + i];
      if (!d) continue;
      const uint32_t key = vmsm_key((uint32_t)b, w, d, c), e = vmsm_entry((uint32_t)(offs[b] + i), d);
      const h::HNiels q = vmsm_hniels(pts[e & 0x7fffffffu]);
      bk[key - key0] = h::hext_madd(bk[key - key0], (e >> 31) ? vmsm_hniels_neg(q) : q);
    }
    for (int g = 0; g < NGW; g++) {  // suffix sums: S_j = sum_{u >= j} B_u, W_g = sum_j S_j, G_g = S_0
      h::HExt run = h::hext_identity(), acc = h::hext_identity();
      for (int j = GS - 1; j >= 0; j--) {
        run = h::hext_add(run, bk[g * GS + j]);
        acc = h::hext_add(acc, run);
      }
      groups[2 * ((size_t)bw * NGW + g)] = acc;
      groups[2 * ((size_t)bw * NGW + g) + 1] = run;
    }
  });
}

// The finish over the group sums: S_w = sum_g W_g + GS sum_g g G_g per (MSM, window) on the pool, then per MSM Horner
// from the top window with c doublings between windows, then the encoding (one pool burst for all B).
// get(k): point k of the groups array (2 B W NB / GS of them) as a host point.
inline void vmsm_finish(const std::function<h::HExt(size_t)>& get, size_t B, int c, uint8_t* out) {
  const int W = vmsm_windows(c), GS = vmsm_group(c), NGW = (1 << (c - 1)) / GS;
  int lg = 0;
  while ((1 << lg) < GS) lg++;
  std::vector<h::HExt> win(B * (size_t)W);
  pool().parallel_for((int)(B * W), [&](int bw) {
    const size_t g0 = (size_t)bw * NGW;
    // sum_g g G_g = sum_{g >= 1} sum_{h >= g} G_h
    h::HExt wsum = get(2 * g0), S = h::hext_identity(), T = h::hext_identity();
    for (int g = NGW - 1; g >= 1; g--) {
      wsum = h::hext_add(wsum, get(2 * (g0 + g)));
      S = h::hext_add(S, get(2 * (g0 + g) + 1));
      T = h::hext_add(T, S);
    }
    if (NGW > 1) {
      for (int k = 0; k < lg; k++) T = h::hext_dbl(T);
      wsum = h::hext_add(wsum, T);
    }
    win[bw] = wsum;
  });
  pool().parallel_for((int)B, [&](int b) {
    h::HExt acc = win[(size_t)b * W + W - 1];
    for (int w = W - 2; w >= 0; w--) {
      for (int k = 0; k < c; k++) acc = h::hext_dbl(acc);
      acc = h::hext_add(acc, win[(size_t)b * W + w]);
    }
    h::hext_compress(acc, out + 32 * (size_t)b);
  });
}

// B MSMs on the host: buckets, groups and finish as above (the path below SPG_VMSM_HOST_MAX points, and the emulation)
inline void vmsm_host(const Niels* pts, const size_t* offs, const size_t* lens, size_t B, const Fq* s, int c,
                      uint8_t* out) {
  std::vector<h::HExt> groups;
  vmsm_host_groups(pts, offs, lens, B, s, c, groups);
  vmsm_finish([&](size_t k) { return groups[k]; }, B, c, out);
}

}  // namespace spg
