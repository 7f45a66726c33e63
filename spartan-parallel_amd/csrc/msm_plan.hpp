// spg — the launch shapes of the MSM, Bullet, layer and round-evaluation kernels as pure functions of the sizes and
// the knob values (knobs.hpp): the call sites read the knobs and pass them in, so this header has no environment, no
// device code and no state. libspg_hostcheck.so exports each function as spgh_* (hostcheck.cpp);
// tests/test_msm_plan_host.py sweeps them against the dispatch switches' instantiation lists, and the GPU form tests
// choose their sizes by them, so that a retuned threshold moves the tests with it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace spg {

// most partial points per MSM that a comb Bullet round or comb_msm_parts leaves for the host (the host staging)
constexpr int kBulletPartsMax = 512;
// msm_big.hip: threads per workgroup (64 quads)
constexpr int kBigBS = 256;

// ---------------------------------------------------------------- bucket pipeline (msm.hip msm_batch_device)
// window width of the batch pipeline by the scalars of one MSM: W windows of 7 units per scalar against 9 per bucket
inline int pick_window(size_t n_per_msm) {
  int best = 4;
  double best_cost = 1e300;
  for (int c = 4; c <= 16; c++) {
    int W = 253 / c + 1;
    double cost = (double)n_per_msm * W * 7.0 + (double)(1 << c) * 9.0;
    if (cost < best_cost) {
      best_cost = cost;
      best = c;
    }
  }
  return best;
}

// window width of the latency path: forced (SPG_SMSM_C) when in 4..9, else by the scalars of one MSM
inline int pick_small_window(size_t per, int forced) {
  if (forced >= 4 && forced <= 9) return forced;
  // measured on MI355X (scripts/perf_small_msm.py): n = 130 -> c = 7, n = 4098 -> c = 8; the compacted
  // Bullet MSMs (n/2 + 2 = 514 scalars) finish on the host, where 64 buckets per MSM are cheaper than 128
  // (scripts/ab_env.sh SPG_SMSM_C "7 0": 39.7 vs 39.9-40.9 ms per SNARK::prove)
  return per <= 1024 ? 7 : 8;
}

// row batches that ask for the comb table first: B rows of n contiguous generators, tot scalars with the blinds
inline bool msm_comb_rule(bool has_idx, size_t B, size_t n, size_t tot) {
  return !has_idx && B >= 64 && (n <= 1024 ? tot >= ((size_t)1 << 14) : (n <= 16384 && tot >= ((size_t)1 << 22)));
}

// the route of B MSMs of per scalars each (blind included) through the bucket pipeline
struct MsmRoute {
  int c, NB, W;   // window width, buckets per MSM, windows per scalar
  bool rows;      // one workgroup per MSM sorts its digits in LDS (k_digits_rows); else count, scan, scatter
  int m, S, log2m;  // buckets per running-sum segment, segments per MSM
  bool seg_quad;  // k_segments_q; else the lane k_segments
  bool quad;      // k_final_q (+ k_compress_ext); else k_final
  bool regroup;   // k_regroup_q ahead of the final scan (quad form only)
  int final_S, final_log2m;  // what the final scan sees
  int final_sl;   // slots of k_final_q: 32, 64, else 128
};
inline MsmRoute msm_batch_route(size_t B, size_t per, int seg_m, int rows_cmax, bool quad, long seg_quad_max,
                                int final_sl) {
  MsmRoute r;
  r.c = pick_window(per);
  r.NB = 1 << (r.c - 1);
  r.W = 253 / r.c + 1;
  r.m = r.NB < seg_m ? r.NB : seg_m;
  r.S = r.NB / r.m;
  r.log2m = 0;
  while ((1 << r.log2m) < r.m) r.log2m++;
  r.rows = B >= 64 && r.c <= rows_cmax;
  r.quad = quad;
  r.seg_quad = quad && B * (size_t)r.S <= (size_t)seg_quad_max;
  r.regroup = quad && B <= 16 && r.S > 1024;  // few MSMs with many segments: regroup 8 segments per group first
  r.final_S = r.regroup ? r.S >> 3 : r.S;
  r.final_log2m = r.regroup ? r.log2m + 3 : r.log2m;
  const int sl = final_sl ? final_sl : (B >= 256 ? 32 : 128);
  r.final_sl = sl == 32 || sl == 64 ? sl : 128;
  return r;
}

// ---------------------------------------------------------------- comb rows (comb.hip msm_comb)
// window groups per scalar (few rows get up to 4 lanes per scalar: >= 2^17 lanes when there are that few) and
// workgroups per row, for B rows of per scalars; want = SPG_COMB_WGS
inline void comb_rows_shape(size_t B, size_t per, size_t want, size_t gmax, size_t gmin, size_t* G_out,
                            size_t* S_out) {
  size_t G = gmin == 2 || gmin == 4 ? gmin : 1;
  while (G < gmax && G < 4 && B * per * G < ((size_t)1 << 17)) G *= 2;
  const size_t spw = 256 / G;
  *G_out = G;
  *S_out = std::max<size_t>(1, std::min((want + B - 1) / B, (per + spw - 1) / spw));
}

// ---------------------------------------------------------------- one large MSM (msm_big.hip msm_single_big)
// digit blocks: spt scalars per thread (SPG_BIG_SPT), at most 512 blocks (the histogram matrix is NB x G)
inline void big_digit_blocks(int per, int spt, int* G, int* spb) {
  *G = std::max(1, std::min(512, (per + spt * kBigBS - 1) / (spt * kBigBS)));
  *spb = (per + *G - 1) / *G;
}

// ---------------------------------------------------------------- Bullet comb rounds (msm.hip)
// the comb form's launch shape by MSM size P = n / 2: G quads per scalar (window groups of ceil(22 / G)), BS threads,
// R points per workgroup (eg / ebs / er: SPG_BCOMB_G / SPG_BCOMB_BS / SPG_BCOMB_R override, for A/B runs;
// notree: SPG_BCOMB_NOTREE)
inline void bullet_comb_shape(int P, int eg, int ebs, int er, int notree, int* G, int* BS, int* R) {
  // same-box A/Bs on the 2^20 SNARK (Bullet device ms per prove; profiles/r04_ab_bullet_shapes.txt): G 4 -> 8 at
  // P = 512: 1.92 -> 1.88; G 8 -> 11 (two dependent quad additions per quad): 1.87 -> 1.81; R 4 -> 8 (one tree level
  // fewer, twice the host-summed parts): 1.89 -> 1.74, R = 16: 1.85
  *G = P >= 2048 ? 4 : 11;
  *BS = P <= 64 ? 64 : (P <= 128 ? 128 : 256);
  // R: round 4 chose 8 on device time alone; on the prover's wall clock the host's part sums weigh more (91 ns per
  // addition on the box, K <= 4 chunks per MSM: scripts/micro/parts_finals_cpu.cpp, profiles/r05_parts_finals.txt),
  // and R = 2 was fastest (2-rep A/B, SNARK median ms: R 8: 16.66 / 17.13, 2: 16.08 / 16.13, 1: 17.56 / 16.71); with the
  // IFMA part sums (hvec.hpp) R = 4 was (ABBA A/B: 15.23 / 15.93 / 16.39 / 15.67 -> 15.13 / 15.04 / 15.84 / 15.02), and
  // later in the round R = 8 (ABBA, 3 blocks: mean 16.03 -> 15.34 ms, device busy 8.65 -> 8.53 ms; R = 16 15.29 against
  // 15.40; profiles/r05_ab_bcomb_r8.txt)
  *R = P >= 2048 ? 1 : 8;  // the SPARK PolyEvalProofs at 2^24 nonzeros (P = 4096): 256 workgroups per MSM
  if (eg == 4 || eg == 8 || eg == 11) *G = eg;
  if (ebs == 64 || ebs == 128 || ebs == 256) *BS = ebs;
  if (er >= 1 && er <= *BS / 4 && (er & (er - 1)) == 0) *R = er;
  // the last rounds (P <= SPG_BCOMB_NOTREE): every quad its own part, no LDS tree (one level is a full quad addition,
  // ~2.1 us on the round's latency path, scripts/micro/bullet_comb_phases) for at most 2 x 16 parts per MSM
  if (P <= notree) *R = *BS / 4;
  // at most kBulletPartsMax parts per MSM (the host staging): fewer points per workgroup for the largest proofs
  const int wgs = (P * *G + *BS / 4 - 1) / (*BS / 4);
  while (*R > 1 && wgs * *R > kBulletPartsMax) *R /= 2;
}

// the launch of a comb Bullet round (shape_P = P = n / 2) or of comb_msm_parts (P = n scalars, shape_P = max(2, n))
// over a table of c-bit windows (12 or 13): the shape above, G = 10 for 13-bit windows unless 4 (20 windows: groups
// of 2; 11 would leave one empty), and the workgroups per MSM. False when the parts would exceed kBulletPartsMax: the
// caller takes the bucket form.
inline bool bullet_comb_launch(int shape_P, int P, int c, int eg, int ebs, int er, int notree, int* G, int* BS,
                               int* R, int* wgs) {
  bullet_comb_shape(shape_P, eg, ebs, er, notree, G, BS, R);
  if (c == 13 && *G != 4) *G = 10;
  const int S = *BS / 4;
  *wgs = (P * *G + S - 1) / S;
  // the shape's clamp of R counted the workgroups of its own G: an 8 that became 10 has more of them (with the default
  // 11 -> 10 there are fewer and this changes nothing); without this SPG_BCOMB_G=8 over 13-bit windows fell back to
  // the bucket form at P >= 512
  while (*R > 1 && *wgs * *R > kBulletPartsMax) *R /= 2;
  return *wgs * *R <= kBulletPartsMax;
}

// ---------------------------------------------------------------- SPARK layers (layers.hip)
// workgroups and block size of a fused layer round over W = nt * len elements: one workgroup up to one_wg
// (SPG_LAYER_ONEWG) elements (no ticket), else about ept (SPG_LAYER_EPT) elements per thread over 256-thread workgroups
inline void layer_grid(size_t W, size_t one_wg, size_t ept, unsigned* K, int* BS) {
  if (W <= 64) {
    *K = 1;
    *BS = 64;
  } else if (W <= one_wg) {
    *K = 1;
    *BS = 256;
  } else {
    *BS = 256;
    *K = (unsigned)std::min<size_t>((W + 256 * ept - 1) / (256 * ept), 2048);
  }
}

// ---------------------------------------------------------------- sumcheck round evaluations (sumcheck.hip)
// workgroups of a round's evaluation: one per 256 threads of work, at most cap (SPG_SC_GRID)
inline int grid_for(uint32_t total, int cap) {
  int nb = (int)((total + 255) / 256);
  if (nb > cap) nb = cap;
  return nb < 1 ? 1 : nb;
}

}  // namespace spg
