// spg — variable-base MSM over caller-supplied points (GroupElement::vartime_multiscalar_mul, src/group.rs:98-116, on
// points that are not a resident generator set: the verifier's sums over proof points, a one-off commitment against
// someone else's generators). spg_points keeps n points in HBM as affine Niels (96 B each) -- no 2^k P rows, no comb --
// and spg_msm_var* sum over them with a bucket Pippenger whose buckets are per (MSM, window), since a variable base
// has no precomputed doublings: signed c-bit digits, key = (b W + w) NB + |d| - 1 (vmsm.hpp).
//   k_points_load    one lane per point: RFC 9496 DECODE, then (y + x, y - x, 2d x y) directly (Z = 1: no inversion);
//                    the lowest invalid index by atomicMin
//   k_vmsm_digits    signed digits (kept in HBM as int16) and block-local LDS histograms, a few windows per pass
//   hipcub scan      over the [key][block] histogram matrix: the entry range of each (key, block) pair
//   k_vmsm_scatter   counting-sort scatter of (point index | sign) into key order, LDS cursors
//   k_vmsm_nchunks, scan, k_vmsm_chunks   the accumulation's work list: key k split into chunks of <= CH entries (an
//                    overfull bucket -- all scalars equal -- only lengthens the list), the group tickets, and the
//                    identity for groups that no chunk will report
//   k_vmsm_accum     one workgroup per chunk: one-lane mixed additions over every 256th entry, the LDS quad tree
//                    (quad.hpp), and the workgroup that finishes the last chunk of a group of GS = min(64, NB) keys
//                    reduces that group to W_g = sum_j (j + 1) B_j and G_g = sum_j B_j (ticket, agent-scope release /
//                    acquire as msm_big.hip's big_chunk). No workgroup waits on another.
//   host             vmsm_finish (vmsm.hpp): window sums, Horner with c doublings per window, encodings.
// Below SPG_VMSM_HOST_MAX points per MSM the whole sum runs on the host pool from the same recode and layout
// (vmsm_host). Single-rank: no sharded form.
#include <hipcub/hipcub.hpp>

#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ctx.hpp"
#include "hcurve.hpp"
#include "knobs.hpp"
#include "quad.hpp"
#include "vmsm.hpp"

namespace spg {

namespace {

constexpr int kVBS = 256;     // threads per workgroup (64 quads)
constexpr int kVQuads = kVBS / 4;
constexpr int kVKeys = 8192;  // LDS histogram / cursor words per pass (one window at c = 14)

struct VMsm {  // one MSM of a batch
  uint32_t poff, soff, len;  // first point, first scalar, length
  uint32_t base, G;          // its rows of the histogram matrix start at base; G digit blocks (columns per key)
};
struct VBlk {  // one digit block: scalars [i0, i1) of MSM b, column j
  uint32_t b, i0, i1, j;
};
struct VChunk {
  uint32_t key, start, len, pad;
};
struct VArgs {
  const Fq* scalars;
  const VMsm* msm;
  const VBlk* blk;
  int c, W, NB, N;  // N scalars in all
  int wpp;          // windows per LDS pass
  uint32_t M;       // histogram matrix entries
  int16_t* digits;  // [W][N]
  uint32_t* bh;     // histogram matrix (+ a zero at [M])
  uint32_t* off;    // its exclusive scan; off[M] = the number of entries
  uint32_t* entries;
};

__global__ void __launch_bounds__(64) k_points_load(const uint8_t* __restrict__ comp, Niels* __restrict__ out,
                                                    int* __restrict__ bad, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t c[32];
  for (int k = 0; k < 32; k++) c[k] = comp[32 * (size_t)i + k];
  Ext P;
  if (!ext_decompress(c, P)) {
    atomicMin(bad, i);
    P = ext_identity();
  }
  out[i] = vmsm_niels_affine(P);
}

__global__ void __launch_bounds__(kVBS) k_vmsm_digits(VArgs a) {
  __shared__ uint32_t cnt[kVKeys];
  const int t = threadIdx.x;
  const VBlk blk = a.blk[blockIdx.x];
  const VMsm m = a.msm[blk.b];
  for (uint32_t i = blk.i0 + t; i < blk.i1; i += kVBS) {
    const Fq k = fq_from_mont(a.scalars[m.soff + i]);  // Scalar::to_bytes (src/scalar/mod.rs:32-36)
    int carry = 0;
    for (int w = 0; w < a.W; w++) a.digits[(size_t)w * a.N + m.soff + i] = (int16_t)vmsm_digit(k.l, a.c, w, carry);
  }
  // (each lane reads back only the digits it wrote)
  for (int w0 = 0; w0 < a.W; w0 += a.wpp) {
    const int nw = min(a.wpp, a.W - w0), nk = nw * a.NB;
    for (int k = t; k < nk; k += kVBS) cnt[k] = 0;
    __syncthreads();
    for (uint32_t i = blk.i0 + t; i < blk.i1; i += kVBS)
      for (int w = 0; w < nw; w++) {
        const int d = a.digits[(size_t)(w0 + w) * a.N + m.soff + i];
        if (d) atomicAdd(&cnt[w * a.NB + (d < 0 ? -d : d) - 1], 1u);
      }
    __syncthreads();
    for (int k = t; k < nk; k += kVBS) a.bh[m.base + ((size_t)w0 * a.NB + k) * m.G + blk.j] = cnt[k];
    __syncthreads();
  }
  if (blockIdx.x == 0 && t == 0) a.bh[a.M] = 0;
}

__global__ void __launch_bounds__(kVBS) k_vmsm_scatter(VArgs a) {
  __shared__ uint32_t cur[kVKeys];
  const int t = threadIdx.x;
  const VBlk blk = a.blk[blockIdx.x];
  const VMsm m = a.msm[blk.b];
  for (int w0 = 0; w0 < a.W; w0 += a.wpp) {
    const int nw = min(a.wpp, a.W - w0), nk = nw * a.NB;
    for (int k = t; k < nk; k += kVBS) cur[k] = a.off[m.base + ((size_t)w0 * a.NB + k) * m.G + blk.j];
    __syncthreads();
    for (uint32_t i = blk.i0 + t; i < blk.i1; i += kVBS)
      for (int w = 0; w < nw; w++) {
        const int d = a.digits[(size_t)(w0 + w) * a.N + m.soff + i];
        if (d) {
          const uint32_t slot = atomicAdd(&cur[w * a.NB + (d < 0 ? -d : d) - 1], 1u);
          a.entries[slot] = vmsm_entry(m.poff + i, d);
        }
      }
    __syncthreads();
  }
}

// first row of key's entries in the scanned histogram matrix (its last is the next key's first: the rows of one MSM are
// contiguous, and MSM b + 1 starts where b ends)
__device__ __forceinline__ uint32_t vmsm_row(const VMsm* __restrict__ msm, uint32_t key, uint32_t kpm) {
  const uint32_t b = key / kpm;
  return msm[b].base + (key - b * kpm) * msm[b].G;
}

// nch[key] = the number of chunks of key (keys: K = B W NB; nch[K] = 0 so that the scan's last element is the total)
__global__ void __launch_bounds__(kVBS) k_vmsm_nchunks(const VMsm* __restrict__ msm, const uint32_t* __restrict__ off,
                                                       uint32_t K, uint32_t kpm, uint32_t ch,
                                                       uint32_t* __restrict__ nch) {
  const uint32_t key = blockIdx.x * kVBS + threadIdx.x;
  if (key > K) return;
  uint32_t v = 0;
  if (key < K) {
    const uint32_t r = vmsm_row(msm, key, kpm), G = msm[key / kpm].G;
    v = (off[r + G] - off[r] + ch - 1) / ch;
  }
  nch[key] = v;
}

// one lane per key: its chunks; the first key of a group also zeroes the group's ticket and, for a group without
// chunks, writes the identity as its sums
__global__ void __launch_bounds__(kVBS) k_vmsm_chunks(const VMsm* __restrict__ msm, const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ first, uint32_t K, uint32_t kpm,
                                                      uint32_t ch, int GS, VChunk* __restrict__ chunks,
                                                      unsigned* __restrict__ gcnt, Ext* __restrict__ out) {
  const uint32_t key = blockIdx.x * kVBS + threadIdx.x;
  if (key >= K) return;
  const uint32_t r = vmsm_row(msm, key, kpm), G = msm[key / kpm].G;
  const uint32_t s = off[r], c = off[r + G] - s;
  uint32_t run = first[key];
  for (uint32_t o = 0; o < c; o += ch) chunks[run++] = VChunk{key, s + o, min(ch, c - o), 0u};
  if (key % (uint32_t)GS == 0) {
    const uint32_t g = key / (uint32_t)GS;
    gcnt[g] = 0u;
    if (first[key + GS] == first[key]) out[2 * g] = out[2 * g + 1] = ext_identity();
  }
}

// Group g of GS <= 64 keys (run by the workgroup that finishes the group's last chunk): quad j < GS holds
// B_j = bucket GS g + j (its chunks summed), the other quads the identity; the suffix scan S_j = sum_{u >= j} B_u and
// the tree sum_j S_j = sum_j (j + 1) B_j; out[2 g] = that weighted sum, out[2 g + 1] = S_0 = the group's plain sum
__device__ __forceinline__ void vmsm_group_reduce(uint32_t g, int GS, const Ext* __restrict__ sums,
                                                  const uint32_t* __restrict__ first, Ext* __restrict__ out,
                                                  uint32_t* pts) {
  const int t = threadIdx.x, q = t & 3, slot = t >> 2;
  Ext B = ext_identity();
  if (slot < GS) {
    const uint32_t key = g * (uint32_t)GS + slot;
    bool any = false;
    for (uint32_t c = first[key]; c < first[key + 1]; c++) {
      B = any ? quad_add(B, sums[c], q) : sums[c];
      any = true;
    }
  }
  Ext suf = B;
  for (int d = 1; d < kVQuads; d <<= 1) {
    quad_put_op<kVQuads>(pts, slot, suf, q);
    __syncthreads();
    if (slot + d < kVQuads) suf = quad_add_op(suf, quad_get_op<kVQuads>(pts, slot + d, q), q);
    __syncthreads();
  }
  if (slot == 0 && q == 0) out[2 * g + 1] = suf;
  Ext acc = suf;
  for (int d = kVQuads / 2; d >= 1; d >>= 1) {
    if (slot >= d && slot < 2 * d) quad_put_op<kVQuads>(pts, slot - d, acc, q);
    __syncthreads();
    if (slot < d) acc = quad_add_op(acc, quad_get_op<kVQuads>(pts, slot, q), q);
    __syncthreads();
  }
  if (t == 0) out[2 * g] = acc;
}

// quad_operand(Q, q) of lane sum `idx` in the SoA buffer (Ext words: X 0..7, Y 8..15, Z 16..23, T 24..31): lane q of
// the quad reads the two coordinates it needs (Y and X, or T or Z alone), not the whole point
__device__ __forceinline__ Fp lane_sum_operand(const uint32_t* s, int idx, int q) {
  const int o = q < 2 ? 8 : (q == 2 ? 24 : 16);
  Fp u, x;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    u.l[i] = s[(o + i) * kVBS + idx];
    x.l[i] = s[i * kVBS + idx];
  }
  return q < 2 ? fp_addsub(u, x, q == 0) : u;
}

// one workgroup per chunk (grid-stride over the list). Every lane adds every 256th entry of the chunk in one-lane mixed
// additions, the 256 lane sums meet in LDS (quad j adds sums 4j .. 4j + 3), an LDS quad tree gives the chunk's sum.
// Cross-XCD hand-off as big_chunk (msm_big.hip): plain stores + agent-scope release before the ticket, agent-scope
// acquire in the reducer before plain loads (the per-XCD L2s are not coherent).
__global__ void __launch_bounds__(kVBS, 4) k_vmsm_accum(const VChunk* __restrict__ chunks,
                                                        const uint32_t* __restrict__ first,
                                                        const uint32_t* __restrict__ entries,
                                                        const Niels* __restrict__ tab, Ext* __restrict__ sums,
                                                        unsigned* __restrict__ gcnt, Ext* __restrict__ out, uint32_t K,
                                                        int GS) {
  __shared__ uint32_t pts[soa_words<Ext, kVBS>()];  // the lane sums (SoA over 256), then the quad tree's operands
  __shared__ bool last;
  const int t = threadIdx.x, q = t & 3, slot = t >> 2;
  const uint32_t n = first[K];
  for (uint32_t cid = blockIdx.x; cid < n; cid += gridDim.x) {  // uniform per workgroup
    const VChunk c = chunks[cid];
    Ext P = ext_identity();
    if ((uint32_t)t < c.len) {
      P = load_signed(tab, entries[c.start + t]);
      for (uint32_t e = t + kVBS; e < c.len; e += kVBS) {
        const uint32_t x = entries[c.start + e];
        P = ext_madd(P, tab[x & 0x7fffffffu], (x >> 31) != 0);
      }
    }
    soa_put<kVBS>(pts, t, P);
    __syncthreads();
    Ext acc = soa_get<kVBS, Ext>(pts, 4 * slot);
    for (int k = 1; k < 4; k++) acc = quad_add_op(acc, lane_sum_operand(pts, 4 * slot + k, q), q);
    __syncthreads();
    for (int d = kVQuads / 2; d >= 1; d >>= 1) {
      if (slot >= d && slot < 2 * d) quad_put_op<kVQuads>(pts, slot - d, acc, q);
      __syncthreads();
      if (slot < d) acc = quad_add_op(acc, quad_get_op<kVQuads>(pts, slot, q), q);
      __syncthreads();
    }
    const uint32_t g = c.key / (uint32_t)GS;
    if (t == 0) {
      sums[cid] = acc;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const uint32_t total = first[(g + 1) * GS] - first[g * GS];
      last = __hip_atomic_fetch_add(&gcnt[g], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == total - 1;
      if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    __syncthreads();
    if (last) vmsm_group_reduce(g, GS, sums, first, out, pts);
    __syncthreads();  // pts / last are reused by the next chunk
  }
}

// below this many points per MSM the sum runs on the host pool; 0: every size through the kernels.
// SPG_VMSM_HOST_MAX is read once per process; spg_set_vmsm_host_max overrides it for one context.
size_t vmsm_host_max(const spg_ctx* ctx) {
  return ctx->vmsm_host_max >= 0 ? (size_t)ctx->vmsm_host_max : (size_t)knob::vmsm_host_max();
}

// the device pipeline: B MSMs (MSM b: lens[b] points from offs[b], scalars d_s[soff_b ..) concatenated), out: B x 32
int vmsm_device(spg_ctx* ctx, const spg_points* P, const size_t* offs, const size_t* lens, size_t B, const Fq* d_s,
                size_t N, uint8_t* out) {
  hipStream_t s = ctx->stream;
  const int c = vmsm_choose_c(N, B), W = vmsm_windows(c), NB = 1 << (c - 1), GS = vmsm_group(c);
  const size_t kpm = (size_t)W * NB, K = B * kpm, NG = K / GS, E = N * (size_t)W;
  // digit blocks: at least NB scalars each (the histogram matrix has NB W rows per block), at least one per lane
  const size_t spb = std::max<size_t>(kVBS, NB);
  std::vector<VMsm> msm(B);
  std::vector<VBlk> blk;
  size_t M = 0, soff = 0;
  for (size_t b = 0; b < B; b++) {
    const size_t G = std::max<size_t>(1, (lens[b] + spb - 1) / spb);
    SPG_CHECK(ctx, M + kpm * G < 0x7fffffffULL, "variable-base MSM too large");
    msm[b] = VMsm{(uint32_t)offs[b], (uint32_t)soff, (uint32_t)lens[b], (uint32_t)M, (uint32_t)G};
    for (size_t j = 0; j < G; j++)  // (an empty MSM keeps one empty block: it zeroes the MSM's histogram rows)
      blk.push_back(VBlk{(uint32_t)b, (uint32_t)(j * spb), (uint32_t)std::min(lens[b], (j + 1) * spb), (uint32_t)j});
    M += kpm * G;
    soff += lens[b];
  }
  SPG_CHECK(ctx, E < 0x7fffffffULL && K < 0x7fffffffULL, "variable-base MSM too large");
  // chunk size: up to 4 entries per lane (a bucket with more -- skewed scalars -- splits into several chunks)
  static_assert(knob::vmsm_ch_dflt == 4 * kVBS, "knobs.hpp default");
  const uint32_t ch = (uint32_t)knob::vmsm_ch();
  const size_t max_chunks = E / ch + K + 1;
  VArgs a{};
  a.scalars = d_s;
  a.c = c;
  a.W = W;
  a.NB = NB;
  a.N = (int)N;
  a.wpp = std::max(1, kVKeys / NB);
  a.M = (uint32_t)M;
  const size_t desc_bytes = B * sizeof(VMsm), blk_bytes = blk.size() * sizeof(VBlk);
  uint8_t* desc = (uint8_t*)ws_get(ctx, Ws::VmsmDesc, desc_bytes + blk_bytes + 64);
  a.digits = (int16_t*)ws_get(ctx, Ws::VmsmDigits, E * sizeof(int16_t) + 64);
  a.bh = (uint32_t*)ws_get(ctx, Ws::VmsmHist, (M + 1) * 4 + 64);
  a.off = (uint32_t*)ws_get(ctx, Ws::VmsmOff, (M + 1) * 4 + 64);
  a.entries = (uint32_t*)ws_get(ctx, Ws::VmsmEntries, E * 4 + 64);
  VChunk* chunks = (VChunk*)ws_get(ctx, Ws::VmsmChunks, max_chunks * sizeof(VChunk));
  uint32_t* nch = (uint32_t*)ws_get(ctx, Ws::VmsmNumChunks, (K + 1) * 4 + 64);
  uint32_t* first = (uint32_t*)ws_get(ctx, Ws::VmsmFirst, (K + GS + 1) * 4 + 64);
  Ext* sums = (Ext*)ws_get(ctx, Ws::VmsmSums, max_chunks * sizeof(Ext));
  unsigned* gcnt = (unsigned*)ws_get(ctx, Ws::VmsmGroupCnt, NG * 4 + 64);
  Ext* groups = (Ext*)ws_get(ctx, Ws::VmsmGroups, 2 * NG * sizeof(Ext));
  if (!desc || !a.digits || !a.bh || !a.off || !a.entries || !chunks || !nch || !first || !sums || !gcnt || !groups)
    return set_err(ctx, SPG_E_NOMEM, "variable-base MSM workspace");
  size_t tmp1 = 0, tmp2 = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, tmp1, a.bh, a.off, (int)(M + 1), s);
  hipcub::DeviceScan::ExclusiveSum(nullptr, tmp2, nch, first, (int)(K + 1), s);
  size_t tmp_bytes = std::max(tmp1, tmp2);
  void* tmp = ws_get(ctx, Ws::VmsmScanTmp, tmp_bytes + 16);
  if (!tmp) return set_err(ctx, SPG_E_NOMEM, "variable-base MSM scan workspace");
  Ext* h_groups = (Ext*)pinned_get(ctx, 2 * NG * sizeof(Ext));
  if (!h_groups) return set_err(ctx, SPG_E_NOMEM, "variable-base MSM staging");
  SPG_HIP(ctx, hipMemcpyAsync(desc, msm.data(), desc_bytes, hipMemcpyHostToDevice, s));
  SPG_HIP(ctx, hipMemcpyAsync(desc + desc_bytes, blk.data(), blk_bytes, hipMemcpyHostToDevice, s));
  a.msm = (const VMsm*)desc;
  a.blk = (const VBlk*)(desc + desc_bytes);
  static_assert(sizeof(VMsm) % 4 == 0 && sizeof(VBlk) == 16, "descriptor layout");
  const unsigned nblk = (unsigned)blk.size(), kgrid = (unsigned)((K + 1 + kVBS - 1) / kVBS);
  const double nz = (double)E * (1.0 - 1.0 / (double)(1 << c));  // nonzero digits of random scalars
  timer_start(ctx);
  {
    KScope ks(ctx, "vmsm_digits", (double)N * 32 + (double)E * 2);
    hipLaunchKernelGGL(k_vmsm_digits, dim3(nblk), dim3(kVBS), 0, s, a);
  }
  {
    KScope ks(ctx, "vmsm_scatter", (double)E * 2 + nz * 4);
    SPG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, a.bh, a.off, (int)(M + 1), s));
    hipLaunchKernelGGL(k_vmsm_scatter, dim3(nblk), dim3(kVBS), 0, s, a);
    hipLaunchKernelGGL(k_vmsm_nchunks, dim3(kgrid), dim3(kVBS), 0, s, a.msm, a.off, (uint32_t)K, (uint32_t)kpm, ch,
                       nch);
    SPG_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, nch, first, (int)(K + 1), s));
    hipLaunchKernelGGL(k_vmsm_chunks, dim3(kgrid), dim3(kVBS), 0, s, a.msm, a.off, first, (uint32_t)K, (uint32_t)kpm,
                       ch, GS, chunks, gcnt, groups);
  }
  {
    // modelled: 96 B of point plus 4 B of index per entry, one mixed addition per nonzero digit
    KScope ks(ctx, "vmsm_accum", nz * 100.0, nz);
    hipLaunchKernelGGL(k_vmsm_accum, dim3((unsigned)std::min<size_t>(max_chunks, 8192)), dim3(kVBS), 0, s, chunks, first,
                       a.entries, P->niels, sums, gcnt, groups, (uint32_t)K, GS);
  }
  SPG_HIP(ctx, hipGetLastError());
  timer_stop(ctx);
  SPG_HIP(ctx, hipMemcpyAsync(h_groups, groups, 2 * NG * sizeof(Ext), hipMemcpyDeviceToHost, s));
  SPG_HIP(ctx, hipStreamSynchronize(s));
  vmsm_finish([&](size_t k) { return h::hext_from_dev(h_groups[k]); }, B, c, out);
  float ms = 0.f;
  hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  ctx->last_us = ms * 1000.0;
  return SPG_OK;
}

// B MSMs over P; the scalars either on the host (h_s) or resident (d_s), concatenated in b order
int vmsm_run(spg_ctx* ctx, const spg_points* P, const size_t* offs, const size_t* lens, size_t B, const Fq* h_s,
             const Fq* d_s, uint8_t* out) {
  size_t N = 0, longest = 0;
  for (size_t b = 0; b < B; b++) {
    SPG_CHECK(ctx, offs[b] <= P->n && lens[b] <= P->n - offs[b], "variable-base MSM: range past the points");
    N += lens[b];
    longest = std::max(longest, lens[b]);
  }
  SPG_CHECK(ctx, N < 0x7fffffffULL, "variable-base MSM too large");
  if (N == 0) {  // empty sums: the identity, whose encoding is 32 zero bytes
    memset(out, 0, 32 * B);
    return SPG_OK;
  }
  hipStream_t s = ctx->stream;
  if (longest < vmsm_host_max(ctx)) {
    std::vector<Fq> hs;
    if (!h_s) {
      hs.resize(N);
      SPG_HIP(ctx, hipMemcpyAsync(hs.data(), d_s, N * sizeof(Fq), hipMemcpyDeviceToHost, s));
      SPG_HIP(ctx, hipStreamSynchronize(s));
      h_s = hs.data();
    }
    const int c = vmsm_choose_c(N, B);
    // the handle keeps the points in HBM only: fetch the ranges this call sums (96 B per point, a few KB)
    std::vector<Niels> pts(N);
    std::vector<size_t> o2(B);
    size_t at = 0;
    for (size_t b = 0; b < B; b++) {
      o2[b] = at;
      if (lens[b])
        SPG_HIP(ctx, hipMemcpyAsync(pts.data() + at, P->niels + offs[b], lens[b] * sizeof(Niels),
                                    hipMemcpyDeviceToHost, s));
      at += lens[b];
    }
    SPG_HIP(ctx, hipStreamSynchronize(s));
    vmsm_host(pts.data(), o2.data(), lens, B, h_s, c, out);
    return SPG_OK;
  }
  if (!d_s) {
    Fq* up = (Fq*)ws_get(ctx, Ws::VmsmScalars, N * sizeof(Fq) + 64);
    if (!up) return set_err(ctx, SPG_E_NOMEM, "scalar upload");
    SPG_HIP(ctx, hipMemcpyAsync(up, h_s, N * sizeof(Fq), hipMemcpyHostToDevice, s));
    d_s = up;
  }
  return vmsm_device(ctx, P, offs, lens, B, d_s, N, out);
}

}  // namespace

}  // namespace spg

using namespace spg;

extern "C" int spg_points_upload(spg_ctx* ctx, const uint8_t* compressed, size_t n, spg_points** out) {
  if (!ctx || !out || !compressed) return SPG_E_ARG;
  SPG_CHECK(ctx, n >= 1 && n < 0x7fffffffULL, "spg_points_upload: n out of range");
  hipStream_t s = ctx->stream;
  uint8_t* d_comp = nullptr;
  int* d_bad = nullptr;
  Niels* d_niels = nullptr;
  auto release = [&] {
    if (d_comp) hipFree(d_comp);
    if (d_bad) hipFree(d_bad);
    if (d_niels) hipFree(d_niels);
  };
  if (hipMalloc(&d_comp, 32 * n) != hipSuccess || hipMalloc(&d_bad, sizeof(int)) != hipSuccess ||
      hipMalloc(&d_niels, n * sizeof(Niels)) != hipSuccess) {
    release();
    return set_err(ctx, SPG_E_NOMEM, "points allocation");
  }
  int bad = INT_MAX;
  hipError_t e = hipMemcpyAsync(d_comp, compressed, 32 * n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_bad, &bad, sizeof(int), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    KScope ks(ctx, "vmsm_load", (double)n * (32 + 96));
    hipLaunchKernelGGL(k_points_load, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, d_comp, d_niels, d_bad, (int)n);
    e = hipGetLastError();
  }
  int got = INT_MAX;
  if (e == hipSuccess) e = hipMemcpyAsync(&got, d_bad, sizeof(int), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    release();
    return set_err(ctx, SPG_E_HIP, std::string("spg_points_upload: ") + hipGetErrorString(e));
  }
  if (got != INT_MAX) {
    release();
    return set_err(ctx, SPG_E_POINT, "invalid compressed point at index " + std::to_string(got));
  }
  hipFree(d_comp);
  hipFree(d_bad);
  spg_points* P = new spg_points();
  P->n = n;
  P->niels = d_niels;
  P->compressed = new uint8_t[32 * n];
  memcpy(P->compressed, compressed, 32 * n);
  *out = P;
  return SPG_OK;
}

extern "C" int spg_set_vmsm_host_max(spg_ctx* ctx, long n) {
  if (!ctx) return SPG_E_ARG;
  ctx->vmsm_host_max = n < 0 ? -1 : n;
  return SPG_OK;
}

extern "C" size_t spg_points_n(const spg_points* P) { return P ? P->n : 0; }

extern "C" int spg_points_download(spg_ctx* ctx, const spg_points* P, uint8_t* out) {
  if (!ctx || !P || !out) return SPG_E_ARG;
  memcpy(out, P->compressed, 32 * P->n);
  return SPG_OK;
}

extern "C" int spg_points_free(spg_ctx* ctx, spg_points* P) {
  if (!P) return SPG_OK;
  if (ctx) hipStreamSynchronize(ctx->stream);
  if (P->niels) hipFree(P->niels);
  delete[] P->compressed;
  delete P;
  return SPG_OK;
}

extern "C" int spg_msm_var(spg_ctx* ctx, const spg_points* P, size_t offset, const uint64_t* scalars_mont, size_t n,
                           uint8_t out[32]) {
  if (!ctx || !P || !out || (!scalars_mont && n)) return SPG_E_ARG;
  return vmsm_run(ctx, P, &offset, &n, 1, (const Fq*)scalars_mont, nullptr, out);
}

extern "C" int spg_msm_var_buf(spg_ctx* ctx, const spg_points* P, size_t offset, const spg_buf* buf, size_t s_offset,
                               size_t n, uint8_t out[32]) {
  if (!ctx || !P || !buf || !out) return SPG_E_ARG;
  SPG_CHECK(ctx, s_offset <= buf->n && n <= buf->n - s_offset, "spg_msm_var_buf: range past the buffer");
  return vmsm_run(ctx, P, &offset, &n, 1, nullptr, buf->d + s_offset, out);
}

extern "C" int spg_msm_var_batch(spg_ctx* ctx, const spg_points* P, const size_t* offsets, const size_t* lens, size_t B,
                                 const uint64_t* scalars_mont, uint8_t* out) {
  if (!ctx || !P || (B && (!offsets || !lens || !out))) return SPG_E_ARG;
  if (B == 0) return SPG_OK;
  size_t N = 0;
  for (size_t b = 0; b < B; b++) N += lens[b];
  if (N && !scalars_mont) return SPG_E_ARG;
  return vmsm_run(ctx, P, offsets, lens, B, (const Fq*)scalars_mont, nullptr, out);
}

extern "C" int spg_msm_points(spg_ctx* ctx, const uint8_t* compressed, const uint64_t* scalars_mont, size_t n,
                              uint8_t out[32]) {
  if (!ctx || !out || (n && (!compressed || !scalars_mont))) return SPG_E_ARG;
  if (n == 0) {
    memset(out, 0, 32);
    return SPG_OK;
  }
  spg_points* P = nullptr;
  int rc = spg_points_upload(ctx, compressed, n, &P);
  if (rc) return rc;
  rc = spg_msm_var(ctx, P, 0, scalars_mont, n, out);
  spg_points_free(ctx, P);
  return rc;
}
