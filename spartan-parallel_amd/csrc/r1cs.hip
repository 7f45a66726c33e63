// spg — R1CSProof::prove (src/r1csproof.rs:210-685) with every O(N) table resident in HBM.
//
// Device work (HIP, this file + sumcheck.hip + msm.hip):
//   z_mat assembly into the (p, q_rev, w, x_rev) Z layout        r1csproof.rs:278-293, custom_dense_mlpoly.rs:67-111
//   multiply_vec_block (CSR SpMV for A, B, C at once)             r1csinstance.rs:363-436, sparse_mlpoly.rs:454-472
//   phase-1 / phase-2 round evaluation and folds                  sumcheck.rs:1067-1380, :788-1065
//   compute_eval_table_sparse_disjoint_rounds (CSC, eq-weighted)  r1csinstance.rs:484-534, sparse_mlpoly.rs:524-541
//   bound_poly_vars_rq on Z                                       custom_dense_mlpoly.rs:300-304
//   DensePolynomial::bound / evaluate of the witness sections     dense_mlpoly.rs:258-265, :361-367
//   Bulletproof L/R/delta MSMs                                    proto.hip
// Host work: the Fiat-Shamir transcript, the round polynomials (4 scalars), the sigma protocols over
// <= 5 fixed generators, and the bincode writer. Per sumcheck round exactly three scalars come back.
#include <chrono>
#include <stdio.h>
#include <stdlib.h>

#include "comm.hpp"
#include "hostpoly.hpp"
#include "knobs.hpp"
#include "pe_plan.hpp"
#include "proto.hpp"
#include "lds.hpp"
#include "satcheck.hpp"
#include "sumcheck.hpp"
#include "zk_rounds.hpp"


// R1CSInstance resident in HBM: per matrix instance p, CSR of A_p, B_p, C_p (SpMV) and one merged CSC
// (rows tagged 0/1/2) for the transposed eq-weighted product.
struct spg_r1cs_inst {
  size_t num_instances = 0, max_num_cons = 0, num_vars = 0;
  std::vector<size_t> num_cons;
  std::vector<uint64_t> rp_off, cp_off;  // [3p+m] offsets into rowptr ; [p] offsets into colptr
  std::vector<size_t> nnz;               // [3p+m]
  uint32_t* d_rowptr = nullptr;          // absolute entry indices
  uint32_t* d_col = nullptr;
  spg::Fq* d_val = nullptr;
  uint32_t* d_colptr = nullptr;
  uint32_t* d_crow = nullptr;            // row * 4 + tag
  spg::Fq* d_cval = nullptr;
};

// ProverWitnessSecInfo list resident in HBM: w_mat[p] flattened (q-major), sections concatenated.
static const uint64_t kNotResident = ~0ULL;  // instance held by another rank
struct spg_r1cs_witness {
  size_t nws = 0;
  std::vector<std::vector<size_t>> num_proofs, num_inputs;  // [w][p]
  std::vector<std::vector<uint64_t>> off;                   // [w][p] element offset into d_w
  // [w][p] device address of the instance's w_mat: d_w + off, or a caller's resident device buffer used in place
  // (witness_from_parts); nullptr: held by another rank
  std::vector<std::vector<const spg::Fq*>> ptr;
  spg::Fq* d_w = nullptr;
  size_t total = 0;
};

namespace spg {

// ------------------------------------------------------------------------------------ kernels
__device__ __forceinline__ uint32_t brev(uint32_t v, uint32_t lg) { return lg ? (__brev(v) >> (32 - lg)) : 0u; }

template <class D>
__device__ __forceinline__ int find_desc(const D* d, int P, uint64_t t) {
  int lo = 0, hi = P - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (d[mid].dom_off <= t) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

struct ZDesc {
  uint64_t dom_off, z_off;
  uint32_t lg_q, ni, lg_ni, pad;
};
struct SecDesc {
  const Fq* w;  // the instance's w_mat (spg_r1cs_witness::ptr)
  uint32_t np, ni;
};

// Z[p][q_rev][w][x_rev] = w_mat_w[pw][qw][x]  (zero beyond the section's width)
__global__ void k_z_fill(const ZDesc* __restrict__ zd, int P, const SecDesc* __restrict__ sd, int nws,
                         Fq* __restrict__ Z, uint64_t total) {
  uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  int p = find_desc(zd, P, t);
  const ZDesc d = zd[p];
  uint64_t loc = t - d.dom_off;
  uint32_t i = (uint32_t)(loc % d.ni);
  uint64_t rest = loc / d.ni;
  uint32_t w = (uint32_t)(rest % nws), q = (uint32_t)(rest / nws);
  const SecDesc s = sd[(size_t)w * P + p];
  Fq v = fq_zero();
  if (i < s.ni) v = s.w[(size_t)(s.np == 1 ? 0 : q) * s.ni + i];
  Z[d.z_off + ((size_t)brev(q, d.lg_q) * nws + w) * d.ni + brev(i, d.lg_ni)] = v;
}

// The same fill when every instance has ni >= 256: one workgroup per 16 x 16 tile of a (q, w) row, i = a 2^(lg-4) +
// m 16 + b (a, b < 16; m the tile). brev(i) = brev4(b) 2^(lg-4) + brev(m) 16 + brev4(a), so the tile's reads (b
// contiguous for each a) and its writes (a contiguous for each b) are both 16 runs of 512 bytes; the tile turns
// through LDS. The one-element form's stores land one 32-byte sector per line at bit-reversed positions.
__global__ void __launch_bounds__(256) k_z_fill_tiled(const ZDesc* __restrict__ zd, int P,
                                                      const SecDesc* __restrict__ sd, int nws, Fq* __restrict__ Z) {
  __shared__ uint32_t sh[8][16 * 17];  // component-major, row pitch 17: conflict-free both ways
  const uint64_t t0 = (uint64_t)blockIdx.x * 256;
  const int p = find_desc(zd, P, t0);
  const ZDesc d = zd[p];
  const uint64_t loc0 = t0 - d.dom_off;
  const uint64_t rest = loc0 / d.ni;
  const uint32_t m = (uint32_t)(loc0 % d.ni) >> 8;
  const uint32_t w = (uint32_t)(rest % nws), q = (uint32_t)(rest / nws);
  const SecDesc s = sd[(size_t)w * P + p];
  const uint32_t k = threadIdx.x, sh_hi = d.lg_ni - 4;
  {
    const uint32_t a = k >> 4, b = k & 15;
    const uint32_t i = (a << sh_hi) + (m << 4) + b;
    Fq v = fq_zero();
    if (i < s.ni) v = s.w[(size_t)(s.np == 1 ? 0 : q) * s.ni + i];
#pragma unroll
    for (int c = 0; c < 8; c++) sh[c][a * 17 + b] = v.l[c];
  }
  __syncthreads();
  const uint32_t a = k & 15, b = k >> 4;
  Fq v;
#pragma unroll
  for (int c = 0; c < 8; c++) v.l[c] = sh[c][a * 17 + b];
  const uint32_t ri = (brev(b, 4) << sh_hi) + (brev(m, d.lg_ni - 8) << 4) + brev(a, 4);
  Z[d.z_off + ((size_t)brev(q, d.lg_q) * nws + w) * d.ni + ri] = v;
}

struct SpDesc {
  uint64_t dom_off, out_off;
  uint32_t pi, lg_q, nrows, lg_rows, ni, lg_ni;
};
struct MatDesc {
  uint64_t rp[3];
  uint64_t cp;
};

// Az/Bz/Cz[p][q_rev][x_rev] = sum_e val_e * z[p][q][col_e / Y][col_e % Y], z gathered from the witness sections
// themselves (the mapping k_z_fill applies), so the Z table's fill is off this kernel's path.
// TILED (every instance has >= 256 rows): as k_z_fill_tiled, a workgroup takes a 16 x 16 tile of one q row, lanes read
// 16 consecutive CSR rows each (row = a 2^(lg-4) + m 16 + b) and the three outputs turn through LDS so that the stores
// are 16 runs of 512 bytes at the bit-reversed positions, instead of one 32-byte sector per line per lane. (Mapping the
// lanes to consecutive output positions instead, row = brev(position), made the CSR reads scatter: 289 -> 341 us on
// config 4.) SPG_SPMV_TILED=0: lanes by row, stores scattered.
template <bool TILED>
__global__ void __launch_bounds__(256) k_spmv(const SpDesc* __restrict__ sd, int P, const MatDesc* __restrict__ md,
                                              const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col,
                                              const Fq* __restrict__ val, const SecDesc* __restrict__ sec, int nws,
                                              uint32_t Y,
                                              Fq* __restrict__ Az, Fq* __restrict__ Bz, Fq* __restrict__ Cz,
                                              uint64_t total) {
  // the section descriptors of the block's first instance (nws <= 8) sit in LDS: a nonzero's gather then waits on
  // an LDS read instead of a dependent global load; lanes of a later instance in the same block read them globally
  __shared__ SecDesc s_sec[8];
  const uint64_t t0 = (uint64_t)blockIdx.x * 256;
  const int pb = find_desc(sd, P, t0);
  if ((int)threadIdx.x < nws) s_sec[threadIdx.x] = sec[(size_t)threadIdx.x * P + pb];
  __syncthreads();
  uint64_t t = t0 + threadIdx.x;
  if (!TILED && t >= total) return;  // (tiled: total is whole tiles, every lane is live up to the LDS turn)
  const int p = TILED ? pb : find_desc(sd, P, t);
  const SpDesc d = sd[p];
  const uint64_t loc = t - d.dom_off;
  const uint32_t q = (uint32_t)(loc / d.nrows), k = threadIdx.x, mt = (uint32_t)(loc % d.nrows) >> 8;
  const uint32_t row = TILED ? ((k >> 4) << (d.lg_rows - 4)) + (mt << 4) + (k & 15) : (uint32_t)(loc % d.nrows);
  Fq sums[3];
#pragma unroll
  for (int m = 0; m < 3; m++) {
    const uint32_t* rp = rowptr + md[d.pi].rp[m];
    uint32_t e0 = rp[row], e1 = rp[row + 1];
    Fq s = fq_zero();
    for (uint32_t e = e0; e < e1; e++) {
      uint32_t c = col[e];
      uint32_t w = c / Y, i = c % Y;
      if (w < (uint32_t)nws && i < d.ni) {
        const Fq* xw;
        uint32_t xnp, xni;
        if (p == pb) {
          xw = s_sec[w].w;
          xnp = s_sec[w].np;
          xni = s_sec[w].ni;
        } else {
          const SecDesc& x = sec[(size_t)w * P + p];
          xw = x.w;
          xnp = x.np;
          xni = x.ni;
        }
        if (i < xni) s = fq_add(s, fq_mul(val[e], xw[(size_t)(xnp == 1 ? 0 : q) * xni + i]));
      }
    }
    sums[m] = s;
  }
  Fq* outs[3] = {Az, Bz, Cz};
  const size_t rowbase = d.out_off + (size_t)brev(q, d.lg_q) * d.nrows;
  if (!TILED) {
#pragma unroll
    for (int m = 0; m < 3; m++) outs[m][rowbase + brev(row, d.lg_rows)] = sums[m];
    return;
  }
  __shared__ uint32_t sh[3][8][16 * 17];  // component-major, row pitch 17: conflict-free both ways
#pragma unroll
  for (int m = 0; m < 3; m++)
#pragma unroll
    for (int c = 0; c < 8; c++) sh[m][c][(k >> 4) * 17 + (k & 15)] = sums[m].l[c];
  __syncthreads();
  const uint32_t a = k & 15, b = k >> 4;
  const uint32_t ri = (brev(b, 4) << (d.lg_rows - 4)) + (brev(mt, d.lg_rows - 8) << 4) + brev(a, 4);
#pragma unroll
  for (int m = 0; m < 3; m++) {
    Fq v;
#pragma unroll
    for (int c = 0; c < 8; c++) v.l[c] = sh[m][c][a * 17 + b];
    outs[m][rowbase + ri] = v;
  }
}

struct AbcDesc {
  uint64_t dom_off, out_off;
  uint32_t pi, ni, lg_ni, pad;
};

// ABC[p][w][x_rev] = sum_{M in A,B,C} r_M * sum_{e in M_p, col_e = w*Y + x} eq_rx[row_e] * val_e
// SPLIT (spg_r1cs_eval_tables): the three per-matrix sums themselves, A[p][w][x] into ABC, B's into outB, C's into
// outC, x in natural order (DensePolynomialPqx::new, not new_rev), no weights
template <bool SPLIT>
__global__ void __launch_bounds__(256) k_abc(const AbcDesc* __restrict__ ad, int Pm, const MatDesc* __restrict__ md,
                                             const uint32_t* __restrict__ colptr, const uint32_t* __restrict__ crow,
                                             const Fq* __restrict__ cval, const Fq* __restrict__ eq, uint32_t Y,
                                             Fq rA, Fq rB, Fq rC, Fq* __restrict__ ABC, Fq* __restrict__ outB,
                                             Fq* __restrict__ outC, uint64_t total) {
  uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  int p = find_desc(ad, Pm, t);
  const AbcDesc d = ad[p];
  uint64_t loc = t - d.dom_off;
  uint32_t i = (uint32_t)(loc % d.ni), w = (uint32_t)(loc / d.ni);
  const uint32_t* cp = colptr + md[d.pi].cp;
  uint32_t c = w * Y + i;
  Fq acc[3] = {fq_zero(), fq_zero(), fq_zero()};
  for (uint32_t e = cp[c]; e < cp[c + 1]; e++) {
    uint32_t rt = crow[e];
    Fq v = fq_mul(cval[e], eq[rt >> 2]);
    uint32_t tag = rt & 3;
    if (tag == 0) acc[0] = fq_add(acc[0], v);
    else if (tag == 1) acc[1] = fq_add(acc[1], v);
    else acc[2] = fq_add(acc[2], v);
  }
  if (SPLIT) {
    const size_t o = d.out_off + (size_t)w * d.ni + i;
    ABC[o] = acc[0];
    outB[o] = acc[1];
    outC[o] = acc[2];
    return;
  }
  Fq r = fq_add(fq_add(fq_mul(rA, acc[0]), fq_mul(rB, acc[1])), fq_mul(rC, acc[2]));
  ABC[d.out_off + (size_t)w * d.ni + brev(i, d.lg_ni)] = r;
}

// every witness polynomial's L.Z bound of one proof in two launches (instead of two per polynomial): job k's
// partial rows are blocks [b0, b0 + nbx * S) of the first launch, its column sums blocks
// [c0, c0 + ceil(Rs / kSumCols)) of the second
struct BoundDesc {
  const Fq* Z;
  uint32_t offL, Ls, Rs, chunk, S, offP, o, b0, c0;
};
constexpr int kBoundMax = 32;
struct BoundJobs {
  BoundDesc d[kBoundMax];
  int n;
};
__device__ __forceinline__ int bound_job(const BoundJobs& j, uint32_t b, bool cols) {
  int k = 0;
  while (k + 1 < j.n && (cols ? j.d[k + 1].c0 : j.d[k + 1].b0) <= b) k++;
  return k;
}
__global__ void __launch_bounds__(256) k_bound_part_multi(BoundJobs jobs, const Fq* __restrict__ L, Fq* __restrict__ part) {
  const int k = bound_job(jobs, blockIdx.x, false);
  const BoundDesc& d = jobs.d[k];
  const uint32_t nbx = (d.Rs + 255) / 256, rel = blockIdx.x - d.b0, y = rel / nbx;
  const uint32_t i = (rel % nbx) * 256 + threadIdx.x;
  if (i >= d.Rs) return;
  const uint32_t j0 = y * d.chunk, j1 = min(d.Ls, j0 + d.chunk);
  Fq acc = fq_zero();
  for (uint32_t j = j0; j < j1; j++) acc = fq_add(acc, fq_mul(L[d.offL + j], d.Z[(size_t)j * d.Rs + i]));
  part[d.offP + (size_t)y * d.Rs + i] = acc;
}
// a block owns kSumCols columns of one job and 256 / kSumCols lanes per column split its S partials, then an LDS
// tree (one lane per column made S dependent additions)
constexpr int kSumCols = 16;
__global__ void __launch_bounds__(256) k_sum_cols_multi(BoundJobs jobs, const Fq* __restrict__ part, Fq* __restrict__ out) {
  __shared__ Fq sm[256];
  constexpr int YL = 256 / kSumCols;
  const int k = bound_job(jobs, blockIdx.x, true);
  const BoundDesc& d = jobs.d[k];
  const int t = threadIdx.x, y0 = t / kSumCols;
  const uint32_t i = (blockIdx.x - d.c0) * kSumCols + t % kSumCols;
  Fq acc = fq_zero();
  if (i < d.Rs)
    for (uint32_t y = y0; y < d.S; y += YL) acc = fq_add(acc, part[d.offP + (size_t)y * d.Rs + i]);
  sm[t] = acc;
  __syncthreads();
#pragma unroll
  for (int h = YL / 2; h >= 1; h >>= 1) {
    if (y0 < h) sm[t] = fq_add(sm[t], sm[t + kSumCols * h]);
    __syncthreads();
  }
  if (y0 == 0 && i < d.Rs) out[d.o + i] = sm[t];
}

// SparseMatPolynomial::evaluate_with_tables (src/sparse_mlpoly.rs:427-436) for every matrix of the
// instance at once: segment s = 3p + m (A, B, C of matrix instance p); one thread per CSR row computes
// eq_rx[row] * sum_e val_e * eq_ry[col_e]; blocks publish partial sums, k_sum_segments adds them.
__device__ __forceinline__ Fq block_sum1(Fq v) {
  __shared__ uint32_t sh[soa_words<Fq, 256>()];  // component-major: no bank conflicts
  int t = threadIdx.x;
  for (int d = 128; d >= 1; d >>= 1) {
    if (t >= d && t < 2 * d) soa_put<256>(sh, t - d, v);
    __syncthreads();
    if (t < d) v = fq_add(v, soa_get<256, Fq>(sh, t));
    __syncthreads();
  }
  if (t == 0) soa_put<256>(sh, 0, v);
  __syncthreads();
  Fq r = soa_get<256, Fq>(sh, 0);
  __syncthreads();
  return r;
}
__global__ void __launch_bounds__(256) k_sparse_eval(const MatDesc* __restrict__ md, const uint32_t* __restrict__ rows,
                                                     const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col,
                                                     const Fq* __restrict__ val, const Fq* __restrict__ eq_rx,
                                                     const Fq* __restrict__ eq_ry, Fq* __restrict__ partials) {
  // rows[2p], rows[2p + 1]: the row range [r0, r1) of instance p evaluated here (a rank's share when sharded)
  const int seg = blockIdx.y, p = seg / 3, m = seg % 3;
  const uint32_t row = rows[2 * p] + blockIdx.x * 256 + threadIdx.x;
  Fq acc = fq_zero();
  if (row < rows[2 * p + 1]) {
    const uint32_t* rp = rowptr + md[p].rp[m];
    Fq sr = fq_zero();
    for (uint32_t e = rp[row]; e < rp[row + 1]; e++) sr = fq_add(sr, fq_mul(val[e], eq_ry[col[e]]));
    acc = fq_mul(eq_rx[row], sr);
  }
  acc = block_sum1(acc);
  if (threadIdx.x == 0) partials[(size_t)seg * gridDim.x + blockIdx.x] = acc;
}
__global__ void __launch_bounds__(256) k_sum_segments(const Fq* __restrict__ partials, int nblk, Fq* __restrict__ out) {
  Fq acc = fq_zero();
  for (int i = threadIdx.x; i < nblk; i += 256) acc = fq_add(acc, partials[(size_t)blockIdx.x * nblk + i]);
  acc = block_sum1(acc);
  if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

// ------------------------------------------------------------------------------------ host helpers
// (eq tables, UniPoly::from_evals, short MLE evaluations: hostmath.hpp)

// (the prover's switches: knobs.hpp) a pair's size limits, within the buffers sized by kP1PairMax
static size_t p1_pair_max() { return std::min<size_t>(kP1PairMax, (size_t)knob::p1_pair_max()); }
static size_t p2_pair_max() { return std::min<size_t>(kP1PairMax, (size_t)knob::p2_pair_max()); }

// (ZKRounds, the ZK sumcheck round bookkeeping shared by phase 1 and phase 2: zk_rounds.hpp)

// (a pair's posted grid -> round j's and round j + 1's (e0, e2, e3): pair_round_j, pair_round_j1 of hostmath.hpp)

// ------------------------------------------------------------------------------------ the R1CS prover
// R1CSProof::prove (r1csproof.rs). Prover::run_stages calls the stages in protocol order: setup_tables (Z, Az, Bz, Cz
// shapes, descriptors, tau eq tables, k_spmv), run_phase1, sigma1, phase2_prep (ABC, the Z join and q folds, eq(rp)),
// run_phase2, witness_evals (lz_bound on the device), polyeval_batched, final_claims. A phase's loop asks
// p*_next_launch for the next launch form after every challenge; p*_round_single and p*_round_pair are its two arms
// (round_pair_arm is the host sequence both phases' pair arms share).

// the sizes of one prove
struct Shape {
  size_t np, nq, nx, nw, ny;                       // variables of p, q, x (constraints), w (sections), y (inputs)
  size_t PLn;                                      // this rank's instances [p0, p1)
  std::vector<size_t> l_proofs, l_inputs, l_cons;  // their proofs, inputs and constraints
  size_t num_cons;                                 // the padded maximum of constraints
  bool single;                                     // one matrix triple shared by every instance
};

// a ragged table's shape: instance p owns rows[p] x secs x cols[p] elements, packed in order (total: all of them);
// the four padded maxima are the Pqx fields the folds halve. The caller allocates d.
static PqxDev pqx_shape(const std::vector<size_t>& rows, size_t secs, const std::vector<size_t>& cols,
                        size_t num_instances, size_t max_num_proofs, size_t num_witness_secs, size_t max_num_inputs) {
  PqxDev T;
  const size_t n = rows.size();
  T.zlen = n;
  T.off.resize(n);
  T.anp = rows;
  T.anw.assign(n, secs);
  T.ani = cols;
  for (size_t p = 0; p < n; p++) {
    T.off[p] = T.total;
    T.total += rows[p] * secs * cols[p];
  }
  T.num_instances = num_instances;
  T.max_num_proofs = max_num_proofs;
  T.num_witness_secs = num_witness_secs;
  T.max_num_inputs = max_num_inputs;
  T.num_proofs = rows;
  T.num_inputs = cols;
  return T;
}

// The Z fill. k_spmv gathers from the witness itself, so the fill only has to land before phase 2. On the second
// stream it is queued once phase 1's round SPG_Z_AFTER (default 4) has been evaluated, and runs beside the later,
// smaller rounds: overlapping k_spmv or the first, HBM-bound rounds, the kernels slow each other (rocprof and same-box
// A/Bs: DESIGN §4, round 4). SPG_Z_SIDE=0 fills it in order at setup. Whatever way the prove returns, `stream` is
// ordered after the fill before anything later reuses the Z slot (the destructor joins).
struct ZFill {
  spg_ctx* c = nullptr;
  const ZDesc* dz = nullptr;
  const SecDesc* dsec = nullptr;
  int n = 0, nws = 0;  // local instances, witness sections
  Fq* Z = nullptr;
  size_t total = 0;
  bool tiled = false;  // k_z_fill_tiled: every instance's row is whole 256-element tiles
  bool side = false;
  bool queued = false, armed = false;
  int queue() {
    if (queued) return 0;
    queued = true;
    const hipStream_t main_stream = c->stream;
    if (side) {
      SPG_HIP(c, hipEventRecord(c->ev_pre, main_stream));
      SPG_HIP(c, hipStreamWaitEvent(c->stream2, c->ev_pre, 0));
      c->stream = c->stream2;
    }
    {
      KScope ks(c, "z_fill", 64.0 * total);
      if (tiled)  // (total is a multiple of 256 then, and so is every instance's offset)
        hipLaunchKernelGGL(k_z_fill_tiled, dim3((uint32_t)(total / 256)), dim3(256), 0, c->stream, dz, n, dsec, nws, Z);
      else
        hipLaunchKernelGGL(k_z_fill, dim3(blocks_for(total)), dim3(256), 0, c->stream, dz, n, dsec, nws, Z,
                           (uint64_t)total);
    }
    c->stream = main_stream;
    SPG_HIP(c, hipGetLastError());
    if (side) {
      SPG_HIP(c, hipEventRecord(c->ev_side, c->stream2));
      armed = true;
    }
    return 0;
  }
  int join() {
    if (!armed) return 0;
    armed = false;
    return hipStreamWaitEvent(c->stream, c->ev_side, 0) == hipSuccess ? 0 : set_err(c, SPG_E_HIP, "z_fill join");
  }
  ~ZFill() { join(); }
};

// what the stages hand on to later ones
struct Carry {
  // device tables: Z; Az with Bz, Cz of its shape; ABC; the tau eq tables of phase 1; eq(rx), eq(rp) of phase 2
  PqxDev Zp, Az, ABC;
  Fq *Bz = nullptr, *Cz = nullptr;
  Fq *Ap = nullptr, *Aq = nullptr, *Ax = nullptr;
  Fq *eq_rx = nullptr, *eq_p = nullptr;
  Fq* partials = nullptr;  // round evaluations: 3 per workgroup; pair launches: one per element
  MatDesc* dmd = nullptr;  // the matrices' descriptors (k_spmv, k_abc)
  // challenges: phase 1's (x and q also in the reference's reversed order), phase 2's
  FqV rx, rq, rq_rev, rp, ry, rw, rp2;
  Fq claims1[4], claims2[3];  // (tau, Az, Bz, Cz) at phase 1's point; (eq, ABC, Z) at phase 2's
  Fq Az_blind, Bz_blind, Cz_blind, blind_post1, blind_post2;
  Fq claim2, blind2;          // phase 2's claim and its blind
  Pt comm_Az, comm_Bz, comm_Cz, comm_prod;
};

// how the folds of the `pending` rounds whose challenges are drawn reach the tables, and what evaluates the next round
struct NextLaunch {
  bool ride;   // the next launch applies them; else a launch of their own does (then the compaction, when due)
  int rounds;  // of the next launch: 0 (none left), 1 or 2
};

// phase 1 as it goes (Prover::run_phase1)
struct Phase1 {
  size_t rounds = 0;
  ZKRounds zk;
  size_t cons_len, proof_len, instance_len;  // the half lengths of the reference's loop
  size_t lenP, lenQ, lenX;                   // live lengths of the eq tables
  std::vector<size_t> sc_np, sc_nc;          // local; P rounds use all-ones of length P
  PqxDev Ac;                                 // compact Az for the instance rounds; TB, TC share its shape there
  PqxDev* T = nullptr;                       // Az, then Ac
  Fq *TB = nullptr, *TC = nullptr;
  Fq *Aq = nullptr, *Ax = nullptr;           // the live eq(tau_q), eq(tau_x)
  Fq *Aq2 = nullptr, *Ax2 = nullptr;         // the other halves of their ping-pong pairs (a fused fold writes there)
  const Fq* Ap_l = nullptr;                  // eq(tau_p) indexed by the global instance in the x / q rounds
  bool cur_pair = false;                     // the launch in flight evaluates rounds j, j + 1
  FqV r;                                     // the challenges so far
};
// phase 2 as it goes (Prover::run_phase2)
struct Phase2 {
  size_t rounds = 0;
  ZKRounds zk;
  size_t inputs_len, ws_len, instance_len;
  size_t lenP;
  std::vector<size_t> sc_ni;
  PqxDev Zc, ABCc;              // compact Z and ABC for the instance rounds
  PqxDev *TZ = nullptr, *TA = nullptr;
  const Fq* eq_l = nullptr;     // eq(rp) at the local instances
  bool fuse2 = false;           // a single round's fold may ride in the next evaluation
  Fq* ABC2 = nullptr;           // a shared ABC's ping-pong buffer
  size_t W2 = 0;                // witness-section rows per instance of a pair
  bool cur_pair = false;
  FqV r;
};

// a witness-section polynomial (section w, instance p) in the batched opening
struct PolyRef {
  size_t w, p, np, ni, Rs;
  bool mine;
  FqV LZ, R;
  Fq ev;
};

struct Prover {
  spg_ctx* ctx;
  ProverGens& g;
  const spg_r1cs_inst& inst;
  const spg_r1cs_witness& wit;
  size_t P, max_np, Y, nws;
  std::vector<size_t> num_proofs, num_inputs;
  Tr& t;
  Tape& tape;
  R1CSProofP pf;
  std::vector<FqV> challenges;
  // device descriptor staging (kept alive until the stream is synchronised)
  std::vector<uint8_t> desc_host;

  Prover(spg_ctx* c, ProverGens& gg, const spg_r1cs_inst& in, const spg_r1cs_witness& w, Tr& tt, Tape& tp)
      : ctx(c), g(gg), inst(in), wit(w), t(tt), tape(tp) {}

  // descriptors are staged in desc_host (256-byte aligned, at most 1 MB per proof) and go up to the device in one
  // copy per flush_desc(); a staged descriptor's device address is valid for kernels launched after that flush
  size_t desc_cur = 0, desc_done = 0;
  uint8_t* desc_dev = nullptr;
  template <class D>
  int stage_desc(const std::vector<D>& v, D** dptr) {
    if (!desc_dev && !(desc_dev = (uint8_t*)ws_get(ctx, Ws::R1csDesc, 1 << 20)))
      return set_err(ctx, SPG_E_NOMEM, "descriptor buffer");
    const size_t bytes = v.size() * sizeof(D), off = (desc_cur + 255) & ~(size_t)255;
    if (off + bytes > (1 << 20)) return set_err(ctx, SPG_E_ARG, "too many descriptors");
    if (desc_host.size() < off + bytes) desc_host.resize(off + bytes);
    memcpy(desc_host.data() + off, v.data(), bytes);
    *dptr = (D*)(desc_dev + off);
    desc_cur = off + bytes;
    return 0;
  }
  int flush_desc() {
    if (desc_cur > desc_done)
      SPG_HIP(ctx, hipMemcpyAsync(desc_dev + desc_done, desc_host.data() + desc_done, desc_cur - desc_done,
                                  hipMemcpyHostToDevice, ctx->stream));
    desc_done = desc_cur;
    return 0;
  }

  // instance shard of this rank (R1CSProof sharded by instance p over nranks processes): balanced split,
  // the first P % nranks ranks hold one instance more, so every rank holds one when nranks <= P
  size_t rank = 0, nranks = 1, p0 = 0, p1 = 0;
  static size_t shard_begin(size_t P, size_t nranks, size_t r) {
    return r * (P / nranks) + std::min(r, P % nranks);
  }
  size_t owner_of(size_t p) const {
    size_t r = 0;
    while (r + 1 < nranks && shard_begin(P, nranks, r + 1) <= p) r++;
    return r;
  }
  int sum_ranks(Fq e[3]);
  // the exchanges of a sharded prove, in order (payload bytes per rank): their sequence depends only on public
  // sizes, so a rank that fails locally between two of them takes part in the next one with its failure as status
  // (run()) and every rank returns from that same exchange -- none is left blocked in a later one
  std::vector<size_t> xplan;
  size_t xdone = 0;
  bool xshared = false;  // an exchange already returned a failure to every rank
  void plan_exchanges(size_t np, size_t nq, size_t nx, size_t nw, size_t ny);
  int exchange(const void* send, size_t bytes, std::vector<uint8_t>& recv);
  int gather_first(const std::vector<const PqxDev*>& tabs, std::vector<std::vector<Fq>>& full);

  Shape sh;
  Carry cy;
  Laps lp;

  int run();
  int run_stages();
  void init_shape();
  int setup_tables(ZFill& zf);
  // setup_tables in three parts, so that spg_r1cs_sat_check runs the first and the last without a transcript:
  // shapes, workspace and descriptors (want_z: the Z table too); the tau eq tables; the k_spmv launch
  int setup_desc(ZFill& zf, bool want_z);
  int setup_tau();
  int launch_spmv();
  SpDesc* dsd_ = nullptr;
  SecDesc* dsec_ = nullptr;
  bool spmv_tiled_ = false;
  double visits_ = 0;
  // Az * Bz == Cz over this rank's tables (satcheck.hip), merged over the ranks: every rank gets the same report,
  // with p the caller's instance index
  // (rc: this rank's status so far; non-zero skips its launch and fails every rank)
  int sat_check_tables(int rc, spg_sat_report* out);
  // phase 1
  int p1_mode(size_t j) const { return j < sh.nx ? MODE_X : (j < sh.nx + sh.nq ? MODE_Q : MODE_P); }
  int p1_advance(Phase1& s, size_t j);
  int p1_launch_single(Phase1& s, size_t j, const FoldPlan* fold);
  bool p1_pair_ok(const Phase1& s, size_t j) const;
  int p1_launch_pair(Phase1& s, size_t j, int nf, const FoldPlan* fp, const Fq& r1, const Fq& r2);
  int p1_fold2x(Phase1& s, int m, const Fq& r1, const Fq& r2);
  int p1_to_compact(Phase1& s);
  NextLaunch p1_next_launch(const Phase1& s, size_t j_next, int pending) const;
  int p1_launch_next(Phase1& s, size_t j_next, int pending, const Fq& r1, const Fq& r2);
  int p1_round_single(Phase1& s, size_t j, ZFill& zf);
  int p1_round_pair(Phase1& s, size_t j, ZFill& zf);
  int run_phase1(ZFill& zf, FqV& r_all);
  void sigma1();
  int phase2_prep(ZFill& zf);
  // phase 2
  int p2_mode(size_t j) const { return j < sh.ny ? MODE_X : (j < sh.ny + sh.nw ? MODE_W : MODE_P); }
  int p2_launch_single(Phase2& s, size_t j, const Fold2* fold);
  bool p2_pair_ok(const Phase2& s, size_t j, bool fold_pending) const;
  int p2_launch_pair(Phase2& s, int nf, const Fq& r1, const Fq& r2);
  int p2_fold2x(Phase2& s, const Fq& r1, const Fq& r2);
  int p2_to_compact(Phase2& s);
  NextLaunch p2_next_launch(const Phase2& s, size_t j_next, int pending) const;
  int p2_launch_next(Phase2& s, size_t j_next, int pending, const Fq& r1, const Fq& r2);
  int p2_round_single(Phase2& s, size_t j);
  int p2_round_pair(Phase2& s, size_t j);
  int run_phase2();
  // the pair arm of both phases once the grid `ev` is in: rounds j and j + 1, with the phase's `launch_next` between
  // round j + 1's challenge and the rest of its proof; `laps`: the phase's eval / host / fold lap names
  template <class Ph>
  int round_pair_arm(Ph& s, size_t j, const Fq ev[15], const char* const laps[3],
                     int (Prover::*launch_next)(Ph&, size_t, int, const Fq&, const Fq&));
  // openings and final claims
  int lz_bound(std::vector<PolyRef>& polys, size_t lz_total, std::vector<Fq>& lz_mine);
  int witness_evals(std::vector<PolyRef>& polys, std::vector<FqV>& eval_list);
  int polyeval_batched(std::vector<PolyRef>& polys);
  void final_claims(const std::vector<FqV>& eval_list);
};

int Prover::run() {
  lp = Laps();  // the breakdown's clock starts here
  int rc0 = run_stages();
  lp.print();
  if (rc0 && nranks > 1 && !xshared && xdone < xplan.size()) {
    // this rank failed alone: the next exchange of the plan carries the failure to every rank
    std::vector<uint8_t> none(xplan[xdone], 0), r;
    xdone++;
    comm_allgather(ctx, Shard{(int)rank, (int)nranks}, rc0, none.data(), none.size(), r);
  }
  return rc0;
}

// ---- cross-rank exchange (identity when nranks == 1): comm.hpp through api.hip's comm_allgather, so every exchange
// carries this rank's status and a failure on one rank fails all of them
int Prover::exchange(const void* send, size_t bytes, std::vector<uint8_t>& recv) {
  const Shard sh{(int)rank, (int)nranks};
  if (nranks > 1 && (xdone >= xplan.size() || xplan[xdone] != bytes)) {
    // the plan is a restatement of the stages' control flow (sum_ranks in p*_round_single, gather_first in
    // p*_to_compact, the L.Z gather in witness_evals); a mismatch is a library bug
    const int rc = set_err(ctx, SPG_E_ARG, "sharded R1CSProof: exchange " + std::to_string(xdone) + " of " +
                                               std::to_string(bytes) + " bytes is not in the exchange plan");
    xshared = true;
    std::vector<uint8_t> r;
    comm_allgather(ctx, sh, rc, send, bytes, r);
    return rc;
  }
  xdone++;
  const int rc = comm_allgather(ctx, sh, 0, send, bytes, recv);
  if (rc) xshared = true;
  return rc;
}
// (e0, e2, e3) summed over the ranks' instance shards
int Prover::sum_ranks(Fq e[3]) {
  if (nranks == 1) return 0;
  std::vector<uint8_t> r;
  const int rc = exchange(e, 3 * sizeof(Fq), r);
  if (rc) return rc;
  sum_over_ranks(r.data(), (int)nranks, 3, e);
  return 0;
}
// Witness-section polynomials' L.Z widths: Rs = 2^(nv - nv/2) of each (section, instance) polynomial (the bound
// rows that the LZ allgather carries)
static size_t lz_width(size_t np, size_t ni) {
  const size_t nv = lg2(np) + lg2(ni);
  return (size_t)1 << (nv - nv / 2);
}
void Prover::plan_exchanges(size_t np, size_t nq, size_t nx, size_t nw, size_t ny) {
  xplan.clear();
  xdone = 0;
  xshared = false;
  if (nranks == 1) return;
  const size_t PL = (P + nranks - 1) / nranks, sum = 3 * sizeof(Fq);
  // phase 1: one sum per x / q round (p1_round_single), the gather of Az, Bz, Cz before the instance rounds
  // (p1_to_compact)
  const size_t r1 = nx + nq + np;
  if (r1 && nx + nq == 0) xplan.push_back(PL * 3 * sizeof(Fq));
  for (size_t j = 0; j < r1; j++) {
    if (j < nx + nq) xplan.push_back(sum);
    if (j + 1 == nx + nq && np > 0) xplan.push_back(PL * 3 * sizeof(Fq));
  }
  // phase 2: one sum per y / w round (p2_round_single), the gather of Z (and ABC unless shared) before the instance
  // rounds (p2_to_compact)
  const size_t k2 = inst.num_instances == 1 ? 1 : 2, r2 = ny + nw + np;
  if (r2 && ny + nw == 0) xplan.push_back(PL * k2 * sizeof(Fq));
  for (size_t j = 0; j < r2; j++) {
    if (j < ny + nw) xplan.push_back(sum);
    if (j + 1 == ny + nw && np > 0) xplan.push_back(PL * k2 * sizeof(Fq));
  }
  // the L.Z bounds of every witness polynomial (witness_evals)
  size_t lz_total = 0;
  for (size_t i = 0; i < nws; i++)
    for (size_t p = 0; p < wit.num_proofs[i].size(); p++) lz_total += lz_width(wit.num_proofs[i][p], wit.num_inputs[i][p]);
  xplan.push_back(lz_total * sizeof(Fq));
}
// per local instance p, the element (p, 0, 0, 0) of each table -> the same for all P instances, on the host
int Prover::gather_first(const std::vector<const PqxDev*>& tabs, std::vector<std::vector<Fq>>& full) {
  const size_t k = tabs.size(), PL = (P + nranks - 1) / nranks;  // the largest shard; slots per rank
  std::vector<Fq> mine(PL * k, fq_zero());
  {  // one gather per kSegMax elements
    std::vector<FqSeg> segs;
    std::vector<Fq*> dst;
    std::vector<Fq> got;
    auto flush = [&]() -> int {
      got.resize(segs.size());
      int rc = d2h_multi(ctx, segs.data(), (int)segs.size(), got.data());
      for (size_t j = 0; j < segs.size(); j++) *dst[j] = got[j];
      segs.clear();
      dst.clear();
      return rc;
    };
    for (size_t i = 0; i < k; i++) {
      const PqxDev& T = *tabs[i];
      for (size_t p = 0; p < T.zlen; p++) {
        segs.push_back({T.d + T.off[p], 1});
        dst.push_back(&mine[i * PL + p]);
        if (segs.size() == (size_t)kSegMax)
          if (int rc = flush()) return rc;
      }
    }
    if (!segs.empty())
      if (int rc = flush()) return rc;
  }
  std::vector<uint8_t> r;
  int rc = exchange(mine.data(), mine.size() * sizeof(Fq), r);
  if (rc) return rc;
  const Fq* v = (const Fq*)r.data();
  full.assign(k, std::vector<Fq>(P, fq_zero()));
  for (size_t q = 0; q < nranks; q++)
    for (size_t i = 0; i < k; i++)
      for (size_t b = shard_begin(P, nranks, q), p = 0; b + p < shard_begin(P, nranks, q + 1); p++)
        full[i][b + p] = v[q * PL * k + i * PL + p];
  return 0;
}
// a table of n instances holding one element each (what remains of a Pqx table when only the instance
// variables are left unbound); its index / index_high behave exactly like the full table's at (p,0,0,0)
static PqxDev compact_table(Fq* d, size_t n, size_t P) {
  const std::vector<size_t> ones(n, 1);
  PqxDev T = pqx_shape(ones, 1, ones, npow2(n), 1, 1, 1);
  T.d = d;
  T.num_proofs.assign(P, 1);
  T.num_inputs.assign(P, 1);
  return T;
}

// the sizes of the prove and this rank's instances, from the arguments
void Prover::init_shape() {
  sh.num_cons = inst.max_num_cons;
  sh.single = inst.num_instances == 1;
  std::vector<size_t> block_num_cons(P);
  for (size_t p = 0; p < P; p++) block_num_cons[p] = inst.num_cons[sh.single ? 0 : p];
  sh.np = lg2(npow2(P)), sh.nq = lg2(max_np), sh.nx = lg2(sh.num_cons), sh.nw = lg2(nws), sh.ny = lg2(Y);
  // this rank's instances [p0, p1): everything O(N) lives only here; nranks == 1 -> all of them
  sh.PLn = p1 - p0;
  sh.l_proofs.assign(num_proofs.begin() + p0, num_proofs.begin() + p1);
  sh.l_inputs.assign(num_inputs.begin() + p0, num_inputs.begin() + p1);
  sh.l_cons.assign(block_num_cons.begin() + p0, block_num_cons.begin() + p1);
}

int Prover::run_stages() {
  t.protocol("R1CS proof");
  init_shape();
  plan_exchanges(sh.np, sh.nq, sh.nx, sh.nw, sh.ny);

  ZFill zf;
  int rc = setup_tables(zf);
  if (!rc && !knob::z_side()) rc = zf.queue();
  if (rc) return rc;
  lp.lap("setup");
  cy.partials = (Fq*)ws_get(ctx, Ws::R1csPart, std::max(3 * (size_t)kScGridMax, kP1PairMax) * sizeof(Fq) + 64);
  if (!cy.partials) return set_err(ctx, SPG_E_NOMEM, "partials");
  FqV r1;  // phase 1's challenges in round order: x, q, p
  if ((rc = run_phase1(zf, r1))) return rc;
  lp.lap("p1_claims");
  const FqV rx_rev(r1.begin(), r1.begin() + sh.nx);
  cy.rq_rev.assign(r1.begin() + sh.nx, r1.begin() + sh.nx + sh.nq);
  cy.rp.assign(r1.begin() + sh.nx + sh.nq, r1.end());
  cy.rx.assign(rx_rev.rbegin(), rx_rev.rend());
  cy.rq.assign(cy.rq_rev.rbegin(), cy.rq_rev.rend());
  // eq(rx) of phase 2 depends on phase 1's challenges alone: on the device while the host runs the sigma protocols
  cy.eq_rx = (Fq*)ws_get(ctx, Ws::R1csEqRx, (sizeof(Fq) << sh.nx) + 64);
  if (!cy.eq_rx) return set_err(ctx, SPG_E_NOMEM, "eq(rx)");
  if ((rc = eq_table(ctx, cy.rx, cy.eq_rx))) return rc;
  sigma1();
  lp.lap("sigma1");
  if ((rc = phase2_prep(zf))) return rc;
  lp.lap("p2_prep");
  if ((rc = run_phase2())) return rc;
  std::vector<PolyRef> polys;
  std::vector<FqV> eval_list;
  if ((rc = witness_evals(polys, eval_list))) return rc;
  lp.lap("polyeval_bound");
  if ((rc = polyeval_batched(polys))) return rc;
  lp.lap("polyeval_dotlog");
  final_claims(eval_list);
  lp.lap("final");
  return 0;
}

// Z (p, q_rev, w, x_rev) and Az, Bz, Cz = multiply_vec_block (p, q_rev, 0, x_rev) for the local instances: shapes,
// workspace, every setup descriptor in one host-to-device copy, the tau eq tables, k_spmv; zf: the Z fill, made ready
int Prover::setup_tables(ZFill& zf) {
  int rc = setup_desc(zf, true);
  if (!rc) rc = setup_tau();
  if (!rc) rc = launch_spmv();
  if (!ctx->check_sat) return rc;
  // check mode (spg_set_check_sat): refuse a witness that does not satisfy the instance, naming the row. Every rank
  // holds the merged report, so all of them return here together and none waits in a later exchange; a rank whose
  // setup failed still takes part, with its failure as status.
  spg_sat_report rep;
  if ((rc = sat_check_tables(rc, &rep))) return rc;
  if (!rep.violations) return 0;
  xshared = true;
  std::string msg = sat_message(rep);
  if (ctx->sat_stage) {
    if (ctx->sat_order) msg += "; block " + std::to_string(ctx->sat_order[rep.p]);
    msg = std::string(ctx->sat_stage) + ": " + msg;
  }
  return set_err(ctx, SPG_E_UNSAT, msg);
}

int Prover::sat_check_tables(int rc, spg_sat_report* out) {
  std::vector<SatDesc> d;
  uint64_t total = 0;
  spg_sat_report mine;
  memset(&mine, 0, sizeof(mine));
  memset(out, 0, sizeof(*out));
  if (rc) {
  } else if (const char* why = sat_descs(sh.l_proofs.data(), sh.l_cons.data(), sh.PLn, &d, &total))
    rc = set_err(ctx, SPG_E_ARG, std::string("sat_check: ") + why);
  else if (total != cy.Az.total)
    rc = set_err(ctx, SPG_E_ARG, "sat_check: descriptors do not cover the tables");
  else
    rc = sat_check_run(ctx, d, total, cy.Az.d, cy.Bz, cy.Cz, &mine);
  if (mine.violations) mine.p += p0;
  if (nranks == 1) {
    *out = mine;
    return rc;
  }
  // one framed allgather, outside the round plan: a rank whose check failed to run fails every rank with it
  std::vector<uint8_t> all;
  rc = comm_allgather(ctx, Shard{(int)rank, (int)nranks}, rc, &mine, sizeof(mine), all);
  if (rc) {
    xshared = true;
    return rc;
  }
  sat_merge((const spg_sat_report*)all.data(), (int)nranks, out);
  return 0;
}

int Prover::setup_desc(ZFill& zf, bool want_z) {
  const size_t PLn = sh.PLn;
  cy.Zp = pqx_shape(sh.l_proofs, nws, sh.l_inputs, npow2(P), max_np, npow2(nws), Y);
  const size_t ztot = cy.Zp.total;
  if (want_z) {
    cy.Zp.d = (Fq*)ws_get(ctx, Ws::R1csZ, ztot * sizeof(Fq) + 64);
    if (!cy.Zp.d) return set_err(ctx, SPG_E_NOMEM, "Z table");
  }
  PqxDev& Az = cy.Az;
  Az = pqx_shape(sh.l_proofs, 1, sh.l_cons, npow2(P), max_np, 1, sh.num_cons);
  const size_t atot = Az.total;
  Az.d = (Fq*)ws_get(ctx, Ws::R1csAz, atot * sizeof(Fq) + 64);
  cy.Bz = (Fq*)ws_get(ctx, Ws::R1csBz, atot * sizeof(Fq) + 64);
  cy.Cz = (Fq*)ws_get(ctx, Ws::R1csCz, atot * sizeof(Fq) + 64);
  if (!Az.d || !cy.Bz || !cy.Cz) return set_err(ctx, SPG_E_NOMEM, "Az/Bz/Cz");
  // every descriptor of the setup kernels (Z fill, Az/Bz/Cz) goes up in one host-to-device copy
  ZDesc* dz = nullptr;
  bool z_tiled = knob::z_tiled();
  spmv_tiled_ = knob::spmv_tiled();
  visits_ = 0;
  int rc = 0;
  {
    std::vector<ZDesc> zd(PLn);
    std::vector<SecDesc> sd(nws * PLn);
    for (size_t p = 0; p < PLn; p++) {
      zd[p].dom_off = cy.Zp.off[p];
      zd[p].z_off = cy.Zp.off[p];
      zd[p].lg_q = (uint32_t)lg2(sh.l_proofs[p]);
      zd[p].ni = (uint32_t)sh.l_inputs[p];
      zd[p].lg_ni = (uint32_t)lg2(sh.l_inputs[p]);
      if (sh.l_inputs[p] < 256) z_tiled = false;
      if (sh.l_cons[p] < 256) spmv_tiled_ = false;
      for (size_t w = 0; w < nws; w++) {
        size_t pw = wit.num_proofs[w].size() == 1 ? 0 : p0 + p;
        if (!wit.ptr[w][pw]) return set_err(ctx, SPG_E_ARG, "witness shard does not hold instance");
        sd[w * PLn + p].w = wit.ptr[w][pw];
        sd[w * PLn + p].np = (uint32_t)wit.num_proofs[w][pw];
        sd[w * PLn + p].ni = (uint32_t)wit.num_inputs[w][pw];
      }
    }
    std::vector<MatDesc> md(inst.num_instances);
    for (size_t p = 0; p < inst.num_instances; p++) {
      for (int m = 0; m < 3; m++) md[p].rp[m] = inst.rp_off[3 * p + m];
      md[p].cp = inst.cp_off[p];
    }
    std::vector<SpDesc> spd(PLn);
    for (size_t p = 0; p < PLn; p++) {
      size_t pi = sh.single ? 0 : p0 + p;
      spd[p].dom_off = Az.off[p];
      spd[p].out_off = Az.off[p];
      spd[p].pi = (uint32_t)pi;
      spd[p].lg_q = (uint32_t)lg2(sh.l_proofs[p]);
      spd[p].nrows = (uint32_t)sh.l_cons[p];
      spd[p].lg_rows = (uint32_t)lg2(sh.l_cons[p]);
      spd[p].ni = (uint32_t)sh.l_inputs[p];
      spd[p].lg_ni = (uint32_t)lg2(sh.l_inputs[p]);
      visits_ += (double)sh.l_proofs[p] * (inst.nnz[3 * pi] + inst.nnz[3 * pi + 1] + inst.nnz[3 * pi + 2]);
    }
    rc = stage_desc(zd, &dz);
    if (!rc) rc = stage_desc(sd, &dsec_);
    if (!rc) rc = stage_desc(md, &cy.dmd);
    if (!rc) rc = stage_desc(spd, &dsd_);
    if (!rc) rc = flush_desc();
    if (rc) return rc;
  }
  zf.c = ctx, zf.dz = dz, zf.dsec = dsec_, zf.n = (int)PLn, zf.nws = (int)nws;
  zf.Z = cy.Zp.d, zf.total = ztot, zf.tiled = z_tiled, zf.side = knob::z_side();
  return 0;
}

// ---- tau tables (identical on every rank)
int Prover::setup_tau() {
  const size_t np = sh.np, nq = sh.nq, nx = sh.nx;
  FqV tau_p = t.challenges("challenge_tau_p", np);
  FqV tau_q = t.challenges("challenge_tau_q", nq);
  FqV tau_x = t.challenges("challenge_tau_x", nx);
  if (knob::debug_tr()) fprintf(stderr, "[prove] r1cs P=%zu np=%zu nq=%zu nx=%zu tau_x0 %08x\n", (size_t)P, (size_t)np, (size_t)nq, (size_t)nx, tau_x[0].l[0]);
  cy.Ap = (Fq*)ws_get(ctx, Ws::R1csTp, (sizeof(Fq) << np) + 64);
  cy.Aq = (Fq*)ws_get(ctx, Ws::R1csTq, (sizeof(Fq) << nq) + 64);
  cy.Ax = (Fq*)ws_get(ctx, Ws::R1csTx, (sizeof(Fq) << nx) + 64);
  if (!cy.Ap || !cy.Aq || !cy.Ax) return set_err(ctx, SPG_E_NOMEM, "eq tables");
  return eq_tables(ctx, {{tau_p, cy.Ap}, {tau_q, cy.Aq}, {tau_x, cy.Ax}});
}

// ---- Az, Bz, Cz: outputs, CSR row pointers, and per visited entry its column, value and z gather
int Prover::launch_spmv() {
  const PqxDev& Az = cy.Az;
  const size_t atot = Az.total, PLn = sh.PLn;
  KScope ks(ctx, "spmv_block", 96.0 * atot + 12.0 * atot + 68.0 * visits_);
  hipLaunchKernelGGL(spmv_tiled_ ? k_spmv<true> : k_spmv<false>, dim3(blocks_for(atot)), dim3(256), 0, ctx->stream,
                     dsd_, (int)PLn, cy.dmd, inst.d_rowptr, inst.d_col, inst.d_val, dsec_, (int)nws, (uint32_t)Y, Az.d,
                     cy.Bz, cy.Cz, (uint64_t)atot);
  SPG_HIP(ctx, hipGetLastError());
  return 0;
}

// ---- phase 1 (sumcheck.rs:1067-1380)
// round j's sizes: the half lengths of the reference's loop and the per-instance domain sizes of the round
int Prover::p1_advance(Phase1& s, size_t j) {
  const int mode = p1_mode(j);
  if (s.cons_len > 1) s.cons_len /= 2;
  else if (s.proof_len > 1) s.proof_len /= 2;
  else s.instance_len /= 2;
  if (mode != MODE_P)
    for (size_t p = 0; p < s.sc_np.size(); p++) {  // instance_len >= P here: every instance takes part
      if (mode == MODE_X && s.sc_nc[p] > 1) s.sc_nc[p] /= 2;
      if (mode == MODE_Q && s.sc_np[p] > 1) s.sc_np[p] /= 2;
    }
  return mode;
}
// round j's evaluation is enqueued right after round j-1's folds, so it runs on the device while the host finishes
// round j-1's proof (comm_eval, DotProductProof); eval_wait then collects (e0, e2, e3)
int Prover::p1_launch_single(Phase1& s, size_t j, const FoldPlan* fold) {
  const int mode = p1_advance(s, j);
  if (mode == MODE_P) {
    std::vector<size_t> ones(P, 1);
    return phase1_eval(ctx, *s.T, mode, s.proof_len, s.cons_len, s.instance_len, ones, ones, cy.Ap, s.Aq, s.Ax, s.T->d,
                       s.TB, s.TC, cy.partials, nullptr);
  }
  return phase1_eval(ctx, *s.T, mode, s.proof_len, s.cons_len, s.instance_len, s.sc_np, s.sc_nc, s.Ap_l, s.Aq, s.Ax,
                     s.T->d, s.TB, s.TC, cy.partials, nullptr, fold);
}
// before the first instance round: collect every instance's remaining (Az, Bz, Cz) value
int Prover::p1_to_compact(Phase1& s) {
  std::vector<std::vector<Fq>> full;
  PqxDev Bt = cy.Az, Ct = cy.Az;
  Bt.d = cy.Bz;
  Ct.d = cy.Cz;
  int rc = gather_first({&cy.Az, &Bt, &Ct}, full);
  if (rc) return rc;
  Fq* buf = (Fq*)ws_get(ctx, Ws::R1csC1, 3 * P * sizeof(Fq) + 64);
  if (!buf) return set_err(ctx, SPG_E_NOMEM, "compact tables");
  for (int i = 0; i < 3; i++)
    SPG_HIP(ctx, hipMemcpyAsync(buf + i * P, full[i].data(), P * sizeof(Fq), hipMemcpyHostToDevice, ctx->stream));
  SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  s.Ac = compact_table(buf, P, P);
  s.T = &s.Ac;
  s.TB = buf + P;
  s.TC = buf + 2 * P;
  return 0;
}
// Two rounds per launch (sumcheck.hip k_phase1_pair; SPG_P1_PAIR=0: one per launch). A pair takes rounds j, j + 1 of
// one mode (x or q) when every instance's size in that mode is >= 4 and round j + 1's domain holds at most
// SPG_P1_PAIR_MAX (default 8192) points: the latency-bound rounds. Unsharded proofs only (a sharded round sums 3
// scalars over the ranks, a pair would sum 15).
bool Prover::p1_pair_ok(const Phase1& s, size_t j) const {
  if (!knob::p1_pair() || !s.Aq2 || nranks != 1 || j + 1 >= s.rounds || s.T != &cy.Az) return false;
  const int m = p1_mode(j);
  if (m == MODE_P || p1_mode(j + 1) != m) return false;
  size_t dom = 0;
  for (size_t p = 0; p < s.sc_np.size(); p++) {
    const size_t N = m == MODE_X ? s.T->num_inputs[p] : s.T->num_proofs[p];
    const size_t Nl = m == MODE_X ? s.sc_nc[p] : s.sc_np[p];  // the round's local size before its halving
    if (N < 4 || N != Nl) return false;
    dom += m == MODE_X ? s.sc_np[p] * (N / 4) : (N / 4) * s.sc_nc[p];
  }
  return dom > 0 && dom <= p1_pair_max();
}
// rounds j, j + 1 in one launch; nf = 1: round j - 1's pending fold (fp), 2: the previous pair's (r1, r2)
int Prover::p1_launch_pair(Phase1& s, size_t j, int nf, const FoldPlan* fp, const Fq& r1, const Fq& r2) {
  const int m = p1_advance(s, j);
  P1Pair pp;
  pp.mode = m;
  pp.c = m == MODE_X ? s.cons_len : s.proof_len;  // round j's half length of the mode's eq table
  for (size_t p = 0; p < s.sc_np.size(); p++) {
    const size_t N = m == MODE_X ? s.T->num_inputs[p] : s.T->num_proofs[p];
    if (m == MODE_X) {
      pp.rows.push_back(s.sc_np[p]);
      pp.cols.push_back(N / 4);
      pp.step_x.push_back(pp.c / (N / 2));
      pp.step_q.push_back(s.proof_len / s.sc_np[p]);
    } else {
      pp.rows.push_back(N / 4);
      pp.cols.push_back(s.sc_nc[p]);
      pp.step_q.push_back(pp.c / (N / 2));
      pp.step_x.push_back(s.cons_len / s.sc_nc[p]);
    }
  }
  p1_advance(s, j + 1);
  pp.nf = nf;
  pp.r1 = r1;
  pp.r2 = r2;
  Fq*& E = m == MODE_X ? s.Ax : s.Aq;
  Fq*& Ealt = m == MODE_X ? s.Ax2 : s.Aq2;
  size_t& lenE = m == MODE_X ? s.lenX : s.lenQ;
  if (nf == 1) {
    pp.fstride = fp->stride;
    pp.fmode = fp->arg.fmode;
    pp.side_in = fp->arg.side_in;
    pp.side_out = fp->arg.side_out;
    pp.side_live = fp->arg.side_half;
  } else if (nf == 2) {  // the previous pair's folds of this mode's eq table: E (live lenE) -> Ealt (lenE / 4)
    pp.fmode = m;
    pp.side_in = E;
    pp.side_out = Ealt;
    pp.side_live = lenE / 4;
    std::swap(E, Ealt);
    lenE /= 4;
  }
  pp.Ap = s.Ap_l;
  pp.Aq = s.Aq;
  pp.Ax = s.Ax;
  pp.B = s.T->d;
  pp.C = s.TB;
  pp.D = s.TC;
  int rc = phase1_pair(ctx, *s.T, pp, cy.partials, nullptr);
  if (rc) return rc;
  // the size bookkeeping of both rounds' folds (the folds themselves ride in the next launch)
  FoldPlan tmp;
  if ((rc = pqx_fold_plan(ctx, *s.T, m, &tmp)) || (rc = pqx_fold_plan(ctx, *s.T, m, &tmp))) return rc;
  return 0;
}
// a pair's pending folds (r1, r2) on their own launch, before a single round or the instance rounds
int Prover::p1_fold2x(Phase1& s, int m, const Fq& r1, const Fq& r2) {
  P1Pair pp;
  pp.mode = m;
  for (size_t p = 0; p < s.sc_np.size(); p++) {
    pp.rows.push_back(s.T->num_proofs[p]);
    pp.cols.push_back(s.T->num_inputs[p]);
  }
  Fq*& E = m == MODE_X ? s.Ax : s.Aq;
  Fq*& Ealt = m == MODE_X ? s.Ax2 : s.Aq2;
  size_t& lenE = m == MODE_X ? s.lenX : s.lenQ;
  pp.r1 = r1;
  pp.r2 = r2;
  pp.side_in = E;
  pp.side_out = Ealt;
  pp.side_live = lenE / 4;
  pp.B = s.T->d;
  pp.C = s.TB;
  pp.D = s.TC;
  std::swap(E, Ealt);
  lenE /= 4;
  return phase1_fold2x(ctx, *s.T, pp);
}
// The launch form after round j_next - 1's challenge, `pending` folds not yet in the tables (0: the first launch; 1: a
// single round's; 2: a pair's). A single round's fold rides in the next evaluation (fused) when one follows in mode x
// or q on the same tables; a pair's two ride in another pair of its mode. Else the folds take a launch of their own
// and the compaction, when the instance rounds come next, follows it. Whether the next launch is a pair (p1_pair_ok)
// shows in the tables' sizes once a single round's fold is booked or launched: rounds = 0 until then, and the caller
// asks again with nothing pending.
NextLaunch Prover::p1_next_launch(const Phase1& s, size_t j_next, int pending) const {
  if (pending == 0) return {false, j_next >= s.rounds ? 0 : (p1_pair_ok(s, j_next) ? 2 : 1)};
  const int mode = p1_mode(j_next - 1), next_mode = p1_mode(j_next);
  if (pending == 2) {
    const bool again = j_next < s.rounds && next_mode == mode && p1_pair_ok(s, j_next);
    return {again, again ? 2 : 0};
  }
  const bool compact_next = j_next == sh.nx + sh.nq && sh.np > 0;
  return {s.Aq2 && mode != MODE_P && j_next < s.rounds && !compact_next && next_mode != MODE_P, 0};
}
// applies or books the pending folds of challenges r1 (, r2) as p1_next_launch says, then launches round j_next
int Prover::p1_launch_next(Phase1& s, size_t j_next, int pending, const Fq& r1, const Fq& r2) {
  const NextLaunch n = p1_next_launch(s, j_next, pending);
  const bool ride = n.ride;
  const int mode = pending ? p1_mode(j_next - 1) : 0;
  FoldPlan fp;
  int rc = 0;
  if (pending == 1 && ride) {  // the round's eq factor is bound in the same launch as Az, Bz, Cz
    rc = pqx_fold_plan(ctx, *s.T, mode, &fp);
    Fq*& cur = mode == MODE_Q ? s.Aq : s.Ax;
    Fq*& alt = mode == MODE_Q ? s.Aq2 : s.Ax2;
    size_t& side_len = mode == MODE_Q ? s.lenQ : s.lenX;
    fp.arg.r = r1;
    fp.arg.fmode = mode;
    fp.arg.side_in = cur;
    fp.arg.side_out = alt;
    fp.arg.side_half = (uint32_t)(side_len / 2);
    std::swap(cur, alt);
    side_len /= 2;
  } else if (pending == 1) {
    Fq* side = mode == MODE_P ? cy.Ap : (mode == MODE_Q ? s.Aq : s.Ax);
    size_t& side_len = mode == MODE_P ? s.lenP : (mode == MODE_Q ? s.lenQ : s.lenX);
    rc = pqx_bound(ctx, *s.T, s.TB, s.TC, r1, mode, side, side_len);
    side_len /= 2;
  } else if (pending == 2 && !ride) {
    rc = p1_fold2x(s, mode, r1, r2);
  }
  if (!rc && pending && !ride && j_next == sh.nx + sh.nq && sh.np > 0) rc = p1_to_compact(s);
  if (rc) return rc;
  const int nf = ride ? pending : 0;
  const int rounds = pending && !n.rounds ? p1_next_launch(s, j_next, 0).rounds : n.rounds;
  s.cur_pair = rounds == 2;
  if (rounds == 2) return p1_launch_pair(s, j_next, nf, &fp, nf ? r1 : fq_zero(), nf == 2 ? r2 : fq_zero());
  return rounds ? p1_launch_single(s, j_next, nf ? &fp : nullptr) : 0;
}
// a single round in flight: its values, its challenge, the next launch, the rest of its proof
int Prover::p1_round_single(Phase1& s, size_t j, ZFill& zf) {
  const int mode = p1_mode(j);
  Fq e[3];
  int rc = eval_wait(ctx, e);
  if (!rc && j == (size_t)knob::z_after()) rc = zf.queue();  // round j is done and round j + 1 not yet queued
  if (!rc && j == 1 && failpoint(ctx, "r1cs_round")) rc = set_err(ctx, SPG_E_HIP, "failpoint r1cs_round");
  if (!rc && mode != MODE_P) rc = sum_ranks(e);
  if (rc) return rc;
  lp.lap("p1_eval");
  const Fq r_j = s.zk.begin(g, t, j, e);
  lp.lap("p1_host");
  if ((rc = p1_launch_next(s, j + 1, 1, r_j, fq_zero()))) return rc;
  lp.lap("p1_fold");
  s.zk.finish(g, t, tape, j, r_j);
  lp.lap("p1_host");
  s.r.push_back(r_j);
  return 1;
}
// the pair arm: round j is F(X, 0) + F(X, 1) at X = 0, 2, 3; round j + 1 the cubics t -> F(t, Y) (Y = 0, 2, 3) at
// t = r_j
template <class Ph>
int Prover::round_pair_arm(Ph& s, size_t j, const Fq ev[15], const char* const laps[3],
                           int (Prover::*launch_next)(Ph&, size_t, int, const Fq&, const Fq&)) {
  lp.lap(laps[0]);
  Fq ej[3], ej1[3];
  pair_round_j(ev, ej);
  const Fq r_j = s.zk.begin(g, t, j, ej);
  s.zk.finish(g, t, tape, j, r_j);
  s.r.push_back(r_j);
  pair_round_j1(ev, r_j, ej1);
  const Fq r_j1 = s.zk.begin(g, t, j + 1, ej1);
  lp.lap(laps[1]);
  if (int rc = (this->*launch_next)(s, j + 2, 2, r_j, r_j1)) return rc;
  lp.lap(laps[2]);
  s.zk.finish(g, t, tape, j + 1, r_j1);
  lp.lap(laps[1]);
  s.r.push_back(r_j1);
  return 2;
}
int Prover::p1_round_pair(Phase1& s, size_t j, ZFill& zf) {
  static const char* const laps[3] = {"p1_eval", "p1_host", "p1_fold"};
  Fq ev[15];
  int rc = pair_wait(ctx, ev);
  if (!rc && (j == (size_t)knob::z_after() || j + 1 == (size_t)knob::z_after())) rc = zf.queue();
  if (!rc && (j == 1 || j + 1 == 1) && failpoint(ctx, "r1cs_round")) rc = set_err(ctx, SPG_E_HIP, "failpoint r1cs_round");
  if (rc) return rc;
  return round_pair_arm(s, j, ev, laps, &Prover::p1_launch_next);
}
int Prover::run_phase1(ZFill& zf, FqV& r_all) {
  const size_t nx = sh.nx, nq = sh.nq, np = sh.np;
  Phase1 s;
  s.rounds = nx + nq + np;
  s.cons_len = s.lenX = (size_t)1 << nx, s.proof_len = s.lenQ = (size_t)1 << nq;
  s.instance_len = s.lenP = (size_t)1 << np;
  s.sc_np = sh.l_proofs, s.sc_nc = sh.l_cons;
  s.T = &cy.Az, s.TB = cy.Bz, s.TC = cy.Cz;
  s.Aq = cy.Aq, s.Ax = cy.Ax, s.Ap_l = cy.Ap + p0;
  if (knob::sc_fuse()) {
    s.Aq2 = (Fq*)ws_get(ctx, Ws::R1csTq2, (sizeof(Fq) << nq) + 64);
    s.Ax2 = (Fq*)ws_get(ctx, Ws::R1csTx2, (sizeof(Fq) << nx) + 64);
    if (!s.Aq2 || !s.Ax2) return set_err(ctx, SPG_E_NOMEM, "eq tables");
  }
  int rc = s.rounds && nx + nq == 0 ? p1_to_compact(s) : 0;
  if (!rc) rc = p1_launch_next(s, 0, 0, fq_zero(), fq_zero());
  if (rc) return rc;
  s.zk.init(g, tape, s.rounds, fq_zero(), fq_zero());  // host precomputation while round 0 evaluates
  for (size_t j = 0; j < s.rounds;) {
    const int n = s.cur_pair ? p1_round_pair(s, j, zf) : p1_round_single(s, j, zf);
    if (n < 0) return n;
    j += (size_t)n;
  }
  Fq a[6];  // eq factors, then Az, Bz, Cz (a single instance: it sits on this (only) rank's local tables)
  rc = np == 0 ? d2h_multi(ctx, {{cy.Ap, 1}, {s.Aq, 1}, {s.Ax, 1}, {cy.Az.d, 1}, {cy.Bz, 1}, {cy.Cz, 1}}, a)
               : d2h_multi(ctx, {{cy.Ap, 1}, {s.Aq, 1}, {s.Ax, 1}, {s.T->d, 1}, {s.TB, 1}, {s.TC, 1}}, a);
  if (rc) return rc;
  cy.claims1[1] = a[3];
  cy.claims1[2] = a[4];
  cy.claims1[3] = a[5];
  cy.claims1[0] = fq_mul(fq_mul(a[0], a[1]), a[2]);
  cy.blind_post1 = s.zk.blinds_evals[s.rounds - 1];
  pf.sc1 = std::move(s.zk.out);
  r_all = std::move(s.r);
  return 0;
}

// the claims' blinds and commitments, and the three sigma protocols on them
void Prover::sigma1() {
  const Fq tau_claim = cy.claims1[0], Az_claim = cy.claims1[1], Bz_claim = cy.claims1[2], Cz_claim = cy.claims1[3];
  cy.Az_blind = tape.scalar("Az_blind"), cy.Bz_blind = tape.scalar("Bz_blind"), cy.Cz_blind = tape.scalar("Cz_blind");
  const Fq prod_blind = tape.scalar("prod_Az_Bz_blind");
  const Fq prod = fq_mul(Az_claim, Bz_claim);
  const Fq blind_expected1 = fq_mul(tau_claim, fq_sub(prod_blind, cy.Cz_blind));
  const Fq claim_post1 = fq_mul(fq_sub(prod, Cz_claim), tau_claim);
  Sigma1Pre sp;
  if (knob::sigma_ahead())
    sigma1_points(g, g.gens_1, tape, Cz_claim, cy.Cz_blind, Az_claim, cy.Az_blind, Bz_claim, cy.Bz_blind, prod,
                  prod_blind, claim_post1, blind_expected1, claim_post1, cy.blind_post1, &sp);
  pf.pok = knowledge_prove(g, g.gens_1, t, tape, Cz_claim, cy.Cz_blind, &cy.comm_Cz,
                           knob::sigma_ahead() ? sp.k : nullptr);
  pf.prod = product_prove(g, g.gens_1, t, tape, Az_claim, cy.Az_blind, Bz_claim, cy.Bz_blind, prod, prod_blind,
                          &cy.comm_Az, &cy.comm_Bz, &cy.comm_prod, knob::sigma_ahead() ? sp.p : nullptr);
  t.point("comm_Az_claim", cy.comm_Az);
  t.point("comm_Bz_claim", cy.comm_Bz);
  t.point("comm_Cz_claim", cy.comm_Cz);
  t.point("comm_prod_Az_Bz_claims", cy.comm_prod);
  pf.eq1 = equality_prove(g, g.gens_1, t, tape, claim_post1, blind_expected1, claim_post1, cy.blind_post1,
                          knob::sigma_ahead() ? sp.e : nullptr);
}

// phase 2's inputs: the claim, ABC = r_A A + r_B B + r_C C at rx (k_abc), Z joined and bound at rq_rev, eq(rp)
int Prover::phase2_prep(ZFill& zf) {
  const Fq r_A = t.challenge("challenge_Az"), r_B = t.challenge("challenge_Bz"), r_C = t.challenge("challenge_Cz");
  cy.claim2 = fq_add(fq_add(fq_mul(r_A, cy.claims1[1]), fq_mul(r_B, cy.claims1[2])), fq_mul(r_C, cy.claims1[3]));
  cy.blind2 = fq_add(fq_add(fq_mul(r_A, cy.Az_blind), fq_mul(r_B, cy.Bz_blind)), fq_mul(r_C, cy.Cz_blind));
  // ABC: the shared matrix once (every rank), or this rank's instances
  const size_t Ab0 = sh.single ? 0 : p0, Abn = sh.single ? 1 : sh.PLn;
  PqxDev& ABC = cy.ABC;
  ABC = pqx_shape(std::vector<size_t>(Abn, 1), nws, {num_inputs.begin() + Ab0, num_inputs.begin() + Ab0 + Abn},
                  npow2(inst.num_instances), 1, npow2(nws), Y);
  ABC.num_proofs.assign(P, 1);
  ABC.num_inputs.assign(num_inputs.begin() + Ab0, num_inputs.end());
  const size_t btot = ABC.total;
  ABC.d = (Fq*)ws_get(ctx, Ws::R1csAbc, btot * sizeof(Fq) + 64);
  if (!ABC.d) return set_err(ctx, SPG_E_NOMEM, "ABC");
  int rc = 0;
  {
    std::vector<AbcDesc> ad(Abn);
    double visits = 0;
    for (size_t p = 0; p < Abn; p++) {
      const size_t pi = Ab0 + p;
      ad[p].dom_off = ABC.off[p];
      ad[p].out_off = ABC.off[p];
      ad[p].pi = (uint32_t)pi;
      ad[p].ni = (uint32_t)num_inputs[pi];
      ad[p].lg_ni = (uint32_t)lg2(num_inputs[pi]);
      visits += inst.nnz[3 * pi] + inst.nnz[3 * pi + 1] + inst.nnz[3 * pi + 2];
    }
    AbcDesc* dad;
    rc = stage_desc(ad, &dad);
    if (!rc) rc = flush_desc();
    if (rc) return rc;
    KScope ks(ctx, "eval_table_abc", 32.0 * btot + 4.0 * btot + 68.0 * visits);
    hipLaunchKernelGGL(k_abc<false>, dim3(blocks_for(btot)), dim3(256), 0, ctx->stream, dad, (int)Abn, cy.dmd,
                       inst.d_colptr, inst.d_crow, inst.d_cval, cy.eq_rx, (uint32_t)Y, r_A, r_B, r_C, ABC.d,
                       (Fq*)nullptr, (Fq*)nullptr, (uint64_t)btot);
    SPG_HIP(ctx, hipGetLastError());
  }
  rc = zf.queue();  // (phase 1 had no rounds)
  if (!rc) rc = zf.join();  // the Z table's first use
  if (rc) return rc;
  // Z.bound_poly_vars_rq(rq_rev): every q fold in one pass over Z against eq(rq_rev), or one fold launch per
  // challenge, each a read-write pass over the live rows
  const FqV& rq_rev = cy.rq_rev;
  if (knob::q_bound_all() && rq_rev.size() >= 2) {
    Fq* eq_q = (Fq*)ws_get(ctx, Ws::R1csEqQ, (sizeof(Fq) << rq_rev.size()) + 64);
    if (!eq_q) return set_err(ctx, SPG_E_NOMEM, "eq(rq)");
    rc = eq_table(ctx, rq_rev, eq_q);
    if (!rc) rc = pqx_bound_q_all(ctx, cy.Zp, eq_q, rq_rev.size());
    if (rc) return rc;
  } else {
    for (size_t k = 0; k < rq_rev.size(); k++)
      if ((rc = pqx_bound(ctx, cy.Zp, nullptr, nullptr, rq_rev[k], MODE_Q))) return rc;
  }
  cy.eq_p = (Fq*)ws_get(ctx, Ws::R1csEqP, (sizeof(Fq) << sh.np) + 64);
  if (!cy.eq_p) return set_err(ctx, SPG_E_NOMEM, "eq(rp)");
  return eq_table(ctx, cy.rp, cy.eq_p);
}

// ---- phase 2 (sumcheck.rs:788-1065)
int Prover::p2_launch_single(Phase2& s, size_t j, const Fold2* fold) {
  const int mode = p2_mode(j);
  if (s.inputs_len > 1) s.inputs_len /= 2;
  else if (s.ws_len > 1) s.ws_len /= 2;
  else s.instance_len /= 2;
  if (mode == MODE_P) {
    std::vector<size_t> ones(P, 1);
    return phase2_eval(ctx, *s.TA, *s.TZ, mode, s.instance_len, s.ws_len, nws, sh.single, ones, cy.eq_p, cy.partials,
                       nullptr);
  }
  for (size_t p = 0; p < s.sc_ni.size(); p++)
    if (mode == MODE_X && s.sc_ni[p] > 1) s.sc_ni[p] /= 2;
  return phase2_eval(ctx, *s.TA, *s.TZ, mode, s.instance_len, s.ws_len, nws, sh.single, s.sc_ni, s.eq_l, cy.partials,
                     nullptr, fold);
}
// before the first instance round: every instance's remaining Z (and ABC) value
int Prover::p2_to_compact(Phase2& s) {
  const bool single = sh.single;
  hipStream_t st = ctx->stream;
  std::vector<std::vector<Fq>> full;
  int rc = single ? gather_first({&cy.Zp}, full) : gather_first({&cy.Zp, &cy.ABC}, full);
  if (rc) return rc;
  Fq* buf = (Fq*)ws_get(ctx, Ws::R1csC2, 2 * P * sizeof(Fq) + 64);
  if (!buf) return set_err(ctx, SPG_E_NOMEM, "compact tables");
  SPG_HIP(ctx, hipMemcpyAsync(buf, full[0].data(), P * sizeof(Fq), hipMemcpyHostToDevice, st));
  if (single) {  // the shared ABC keeps its single (0,0,0,0) element
    SPG_HIP(ctx, hipMemcpyAsync(buf + P, cy.ABC.d, sizeof(Fq), hipMemcpyDeviceToDevice, st));
  } else {
    SPG_HIP(ctx, hipMemcpyAsync(buf + P, full[1].data(), P * sizeof(Fq), hipMemcpyHostToDevice, st));
  }
  SPG_HIP(ctx, hipStreamSynchronize(st));
  s.Zc = compact_table(buf, P, P);
  s.ABCc = compact_table(buf + P, single ? 1 : P, P);
  s.TZ = &s.Zc;
  s.TA = &s.ABCc;
  return 0;
}
// Two y rounds per launch (sumcheck.hip k_phase2_pair; SPG_P2_PAIR=0: one per launch): rounds j, j + 1 both y rounds,
// ABC per instance, every instance's live y size >= 4 (the same in ABC and Z), at most SPG_P2_PAIR_MAX (default 8192)
// elements, unsharded. A run of pairs starts with no fold pending (a single round's fold before it is launched on its
// own) and ends with k_phase2_fold2x.
// (fold_pending: round j - 1's fold is not yet in the tables' sizes; the caller launches it first)
bool Prover::p2_pair_ok(const Phase2& s, size_t j, bool fold_pending) const {
  const bool single = sh.single;
  const PqxDev &ABC = cy.ABC, &Zp = cy.Zp;
  // (one ABC shared by every instance folds through its ping-pong buffer, as the fused single rounds do)
  if (!knob::p2_pair() || (single && !s.ABC2) || nranks != 1 || j + 1 >= sh.ny || s.TA != &ABC || s.TZ != &Zp ||
      ABC.zlen != (single ? 1 : Zp.zlen))
    return false;
  auto live = [&](size_t n) { return fold_pending && n > 1 ? n / 2 : n; };
  size_t dom = 0;
  for (size_t p = 0; p < s.sc_ni.size(); p++) {
    const size_t N = live(Zp.num_inputs[p]);
    if (N < 4 || live(ABC.num_inputs[single ? 0 : p]) != N || s.sc_ni[p] != N) return false;
    dom += s.W2 * (N / 4);
  }
  return dom > 0 && dom <= p2_pair_max();
}
// y rounds j, j + 1 in one launch; nf = 2: the previous pair's folds (r1, r2) ride in it
int Prover::p2_launch_pair(Phase2& s, int nf, const Fq& r1, const Fq& r2) {
  for (int k = 0; k < 2; k++) {  // p2_launch_single's size bookkeeping for both y rounds
    if (s.inputs_len > 1) s.inputs_len /= 2;
    for (size_t p = 0; p < s.sc_ni.size(); p++)
      if (s.sc_ni[p] > 1) s.sc_ni[p] /= 2;
  }
  P2Pair pp;
  pp.nf = nf;
  pp.r1 = r1;
  pp.r2 = r2;
  pp.W = s.W2;
  pp.eq = s.eq_l;
  pp.B_out = sh.single ? s.ABC2 : nullptr;
  int rc = phase2_pair(ctx, cy.ABC, cy.Zp, pp, cy.partials);
  if (rc) return rc;
  if (sh.single && nf == 2) std::swap(cy.ABC.d, s.ABC2);  // the folded shared ABC is in the other buffer now
  FoldPlan tmp;  // the table bookkeeping of both rounds' folds (the folds ride in the next launch)
  for (int k = 0; k < 2 && !rc; k++) {
    rc = pqx_fold_plan(ctx, cy.ABC, MODE_X, &tmp);
    if (!rc) rc = pqx_fold_plan(ctx, cy.Zp, MODE_X, &tmp);
  }
  return rc;
}
int Prover::p2_fold2x(Phase2& s, const Fq& r1, const Fq& r2) {
  P2Pair pp;
  pp.nf = 2;
  pp.r1 = r1;
  pp.r2 = r2;
  pp.W = s.W2;
  pp.B_out = sh.single ? s.ABC2 : nullptr;
  const int rc = phase2_fold2x(ctx, cy.ABC, cy.Zp, pp);
  if (!rc && sh.single) std::swap(cy.ABC.d, s.ABC2);
  return rc;
}
// The launch form after round j_next - 1's challenge, `pending` folds not yet in the tables (as p1_next_launch). A
// pair's two folds ride in another pair; a single y round before a run of pairs folds on its own launch (the pair
// starts with nothing pending); else a single round's fold rides in the next evaluation (k_phase2_eval<true>) when
// one follows in mode y or w on the same tables.
NextLaunch Prover::p2_next_launch(const Phase2& s, size_t j_next, int pending) const {
  const int left = j_next < s.rounds ? 1 : 0;
  if (pending == 0) return {false, left && p2_pair_ok(s, j_next, false) ? 2 : left};
  if (pending == 2) {
    const bool again = j_next < sh.ny && p2_pair_ok(s, j_next, false);
    return {again, again ? 2 : left};
  }
  const int mode = p2_mode(j_next - 1);
  if (mode == MODE_X && p2_pair_ok(s, j_next, true)) return {false, 2};
  const bool compact_next = j_next == sh.ny + sh.nw && sh.np > 0;
  return {s.fuse2 && mode != MODE_P && left && !compact_next && p2_mode(j_next) != MODE_P, left};
}
// applies or books the pending folds of challenges r1 (, r2) as p2_next_launch says, then launches round j_next
int Prover::p2_launch_next(Phase2& s, size_t j_next, int pending, const Fq& r1, const Fq& r2) {
  const NextLaunch n = p2_next_launch(s, j_next, pending);
  const int mode = pending ? p2_mode(j_next - 1) : 0;
  const bool single = sh.single;
  s.cur_pair = n.rounds == 2;
  if (pending == 2 && n.ride) return p2_launch_pair(s, 2, r1, r2);
  int rc = 0;
  if (pending == 1 && n.ride) {
    Fold2 f;
    rc = pqx_fold_plan(ctx, *s.TA, mode, &f.a);
    if (!rc) rc = pqx_fold_plan(ctx, *s.TZ, mode, &f.z);
    f.arg.r = r1;
    f.arg.fmode = mode;
    f.arg.fw = f.z.fw;
    f.arg.ping = single ? 1 : 0;
    f.arg.b_out = single ? s.ABC2 : s.TA->d;
    if (!rc) rc = p2_launch_single(s, j_next, &f);
    if (!rc && single) std::swap(s.TA->d, s.ABC2);
    return rc;
  }
  if (pending == 2) {
    rc = p2_fold2x(s, r1, r2);
  } else if (pending == 1) {
    if (mode == MODE_P) {
      rc = dev_fold_top(ctx, cy.eq_p, s.lenP, r1);
      s.lenP /= 2;
    }
    if (!rc && (mode != MODE_P || !single)) rc = pqx_bound2(ctx, *s.TA, *s.TZ, r1, mode);
    else if (!rc) rc = pqx_bound(ctx, *s.TZ, nullptr, nullptr, r1, mode);
  }
  if (!rc && pending && j_next == sh.ny + sh.nw && sh.np > 0) rc = p2_to_compact(s);
  if (rc) return rc;
  if (n.rounds == 2) return p2_launch_pair(s, 0, fq_zero(), fq_zero());
  return n.rounds ? p2_launch_single(s, j_next, nullptr) : 0;
}
int Prover::p2_round_single(Phase2& s, size_t j) {
  Fq e[3];
  int rc = eval_wait(ctx, e);
  if (!rc && p2_mode(j) != MODE_P) rc = sum_ranks(e);
  if (rc) return rc;
  lp.lap("p2_eval");
  const Fq r_j = s.zk.begin(g, t, j, e);
  lp.lap("p2_host");
  if ((rc = p2_launch_next(s, j + 1, 1, r_j, fq_zero()))) return rc;
  lp.lap("p2_fold");
  s.zk.finish(g, t, tape, j, r_j);
  lp.lap("p2_host");
  s.r.push_back(r_j);
  return 1;
}
int Prover::p2_round_pair(Phase2& s, size_t j) {
  static const char* const laps[3] = {"p2_eval", "p2_host", "p2_fold"};
  Fq ev[15];
  if (int rc = pair_wait(ctx, ev)) return rc;
  return round_pair_arm(s, j, ev, laps, &Prover::p2_launch_next);
}
int Prover::run_phase2() {
  const size_t ny = sh.ny, nw = sh.nw, np = sh.np;
  Phase2 s;
  s.rounds = ny + nw + np;
  s.inputs_len = (size_t)1 << ny, s.ws_len = (size_t)1 << nw, s.instance_len = s.lenP = (size_t)1 << np;
  s.sc_ni = sh.l_inputs;
  s.TZ = &cy.Zp, s.TA = &cy.ABC;
  s.eq_l = cy.eq_p + p0;
  s.W2 = std::min(s.ws_len, nws);
  // one ABC serving every instance is folded into ABC2 by a fused round (then the two swap). The fused fold writes it
  // from the points of local instance 0 (global p0): only when that instance spans ABC's whole width (num_inputs[0])
  // -- a sharded rank whose first instance is narrower takes the separate fold
  s.fuse2 = knob::sc_fuse() && (!sh.single || num_inputs[p0] == num_inputs[0]);
  if (s.fuse2 && sh.single) {
    s.ABC2 = (Fq*)ws_get(ctx, Ws::R1csAbc2, cy.ABC.total * sizeof(Fq) + 64);
    if (!s.ABC2) return set_err(ctx, SPG_E_NOMEM, "ABC");
  }
  int rc = s.rounds && ny + nw == 0 ? p2_to_compact(s) : 0;
  if (!rc) rc = p2_launch_next(s, 0, 0, fq_zero(), fq_zero());
  if (rc) return rc;
  s.zk.init(g, tape, s.rounds, cy.claim2, cy.blind2);  // host precomputation while round 0 evaluates
  for (size_t j = 0; j < s.rounds;) {
    const int n = s.cur_pair ? p2_round_pair(s, j) : p2_round_single(s, j);
    if (n < 0) return n;
    j += (size_t)n;
  }
  rc = d2h_multi(ctx, {{cy.eq_p, 1}, {s.TA->d, 1}, {s.TZ->d, 1}}, cy.claims2);
  if (rc) return rc;
  cy.blind_post2 = s.zk.blinds_evals[s.rounds - 1];
  pf.sc2 = std::move(s.zk.out);
  cy.ry.assign(s.r.rbegin() + (nw + np), s.r.rend());  // the y challenges, reversed
  cy.rw.assign(s.r.begin() + ny, s.r.begin() + ny + nw);
  cy.rp2.assign(s.r.begin() + ny + nw, s.r.end());
  return 0;
}

// ---- witness-section evaluations and their batched opening (r1csproof.rs:518-639)
// R = eq(rr) of every polynomial, once per distinct right point (instances of one shape share theirs), on the pool
static void right_tables(std::vector<PolyRef>& polys, const std::vector<FqV>& rr_of) {
  std::vector<size_t> uniq, at(polys.size());
  for (size_t k = 0; k < polys.size(); k++) {
    size_t u = 0;
    while (u < uniq.size() && !(rr_of[uniq[u]].size() == rr_of[k].size() &&
                                memcmp(rr_of[uniq[u]].data(), rr_of[k].data(), rr_of[k].size() * sizeof(Fq)) == 0))
      u++;
    if (u == uniq.size()) uniq.push_back(k);
    at[k] = u;
  }
  std::vector<FqV> tabs(uniq.size());
  pool().parallel_for((int)uniq.size(), [&](int u) { tabs[u] = eq_evals_host(rr_of[uniq[u]]); });
  for (size_t k = 0; k < polys.size(); k++) polys[k].R = tabs[at[k]];
}
// LZ = bound(L) of each owned polynomial on this rank's device (lz_mine, zero elsewhere). Every polynomial's eq(rl),
// partial column sums and LZ are queued back to back into disjoint workspace ranges and the LZ of all of them come
// back in one download (one host wait instead of one per polynomial). The host eq tables of the right points are
// computed while the device works (queued first; d2h_fq waits for it).
int Prover::lz_bound(std::vector<PolyRef>& polys, size_t lz_total, std::vector<Fq>& lz_mine) {
  const size_t nq = sh.nq, ny = sh.ny;
  hipStream_t st = ctx->stream;
  struct BoundJob {
    FqV rl;
    size_t Ls, Rs, S, chunk, offL, offP, o;
  };
  std::vector<BoundJob> jobs;
  size_t o = 0, totL = 0, totP = 0;
  bool all_mine = true;
  std::vector<FqV> rr_of(polys.size());  // each polynomial's right point
  size_t pk = 0;
  for (auto& pr : polys) {
    size_t lnp = lg2(pr.np), lni = lg2(pr.ni);
    FqV r(cy.rq.begin() + (nq - lnp), cy.rq.end());
    if (pr.ni >= Y) {
      r.insert(r.end(), lni - ny, fq_zero());
      r.insert(r.end(), cy.ry.begin(), cy.ry.end());
    } else {
      r.insert(r.end(), cy.ry.begin() + (ny - lni), cy.ry.end());
    }
    size_t nv = r.size(), ln = nv / 2;
    FqV rl(r.begin(), r.begin() + ln), rr(r.begin() + ln, r.end());
    size_t Ls = (size_t)1 << ln, Rs = (size_t)1 << (nv - ln);
    rr_of[pk++] = std::move(rr);
    if (pr.mine) {
      size_t S = std::min<size_t>(Ls, 32);  // 32 partial rows: short column sums
      const size_t chunk = (Ls + S - 1) / S;
      S = (Ls + chunk - 1) / chunk;
      jobs.push_back({std::move(rl), Ls, Rs, S, chunk, totL, totP, o});
      totL += Ls;
      totP += S * Rs;
    } else {
      all_mine = false;
    }
    o += Rs;
  }
  if (jobs.empty()) {
    right_tables(polys, rr_of);
    return 0;
  }
  Fq* dL = (Fq*)ws_get(ctx, Ws::R1csL, totL * sizeof(Fq) + 64);
  Fq* dpart = (Fq*)ws_get(ctx, Ws::R1csBoundPart, totP * sizeof(Fq) + 64);
  Fq* dout = (Fq*)ws_get(ctx, Ws::R1csBoundOut, lz_total * sizeof(Fq) + 64);
  if (!dL || !dpart || !dout) return set_err(ctx, SPG_E_NOMEM, "bound");
  if (!all_mine) SPG_HIP(ctx, hipMemsetAsync(dout, 0, lz_total * sizeof(Fq), st));  // other ranks' ranges
  // one eq table per distinct rl (polynomials of one shape share it)
  std::vector<size_t> eq_at(jobs.size());
  std::vector<EqJob> eqs;
  for (size_t k = 0; k < jobs.size(); k++) {
    size_t same = k;
    for (size_t m = 0; m < k; m++)
      if (jobs[m].rl.size() == jobs[k].rl.size() &&
          memcmp(jobs[m].rl.data(), jobs[k].rl.data(), jobs[k].rl.size() * sizeof(Fq)) == 0) {
        same = m;
        break;
      }
    eq_at[k] = same == k ? jobs[k].offL : eq_at[same];
    if (same == k) eqs.push_back({jobs[k].rl.data(), (int)jobs[k].rl.size(), dL + jobs[k].offL});
  }
  int rc = dev_eq_tables(ctx, eqs.data(), (int)eqs.size());
  if (rc) return rc;
  std::vector<const PolyRef*> mine;
  for (auto& pr : polys)
    if (pr.mine) mine.push_back(&pr);
  double bytes = 0;
  for (const BoundJob& j : jobs) bytes += 32.0 * j.Ls * j.Rs + 32.0 * j.Ls + 64.0 * j.S * j.Rs;
  KScope ks(ctx, "poly_bound", bytes);
  for (size_t k0 = 0; k0 < jobs.size(); k0 += kBoundMax) {  // two launches per kBoundMax polynomials
    BoundJobs bj;
    bj.n = (int)std::min<size_t>(kBoundMax, jobs.size() - k0);
    uint32_t nb = 0, nc = 0;
    for (int q = 0; q < bj.n; q++) {
      const BoundJob& j = jobs[k0 + q];
      const PolyRef& pr = *mine[k0 + q];
      const uint32_t nbx = (uint32_t)((j.Rs + 255) / 256);
      bj.d[q] = {wit.ptr[pr.w][pr.p], (uint32_t)eq_at[k0 + q], (uint32_t)j.Ls, (uint32_t)j.Rs,
                 (uint32_t)j.chunk, (uint32_t)j.S, (uint32_t)j.offP, (uint32_t)j.o, nb, nc};
      nb += nbx * (uint32_t)j.S;
      nc += (uint32_t)((j.Rs + kSumCols - 1) / kSumCols);
    }
    hipLaunchKernelGGL(k_bound_part_multi, dim3(nb), dim3(256), 0, st, bj, dL, dpart);
    hipLaunchKernelGGL(k_sum_cols_multi, dim3(nc), dim3(256), 0, st, bj, dpart, dout);
  }
  SPG_HIP(ctx, hipGetLastError());
  right_tables(polys, rr_of);
  return d2h_fq(ctx, dout, lz_mine.data(), lz_total);
}
// every witness polynomial's evaluation at (rq, ry): LZ from its owner shared with every rank, <LZ, R>, commitments
int Prover::witness_evals(std::vector<PolyRef>& polys, std::vector<FqV>& eval_list) {
  const size_t ny = sh.ny;
  FqV ry_factors(ny + 1, fq_one());
  for (size_t i = 0; i < ny; i++) ry_factors[i + 1] = fq_mul(ry_factors[i], fq_sub(fq_one(), cy.ry[i]));
  size_t lz_total = 0;
  for (size_t i = 0; i < nws; i++) {
    for (size_t p = 0; p < wit.num_proofs[i].size(); p++) {
      PolyRef pr;
      pr.w = i;
      pr.p = p;
      pr.np = wit.num_proofs[i][p];
      pr.ni = wit.num_inputs[i][p];
      pr.Rs = lz_width(pr.np, pr.ni);
      pr.mine = wit.num_proofs[i].size() == 1 ? rank == 0 : (p >= p0 && p < p1);
      lz_total += pr.Rs;
      polys.push_back(std::move(pr));
    }
  }
  std::vector<Fq> lz_mine(lz_total, fq_zero());
  int rc = lz_bound(polys, lz_total, lz_mine);
  if (rc) return rc;
  {
    std::vector<uint8_t> r;
    rc = exchange(lz_mine.data(), lz_total * sizeof(Fq), r);
    if (rc) return rc;
    const Fq* v = (const Fq*)r.data();
    size_t o = 0;
    for (auto& pr : polys) {
      size_t owner = 0;
      if (wit.num_proofs[pr.w].size() != 1) owner = owner_of(pr.p);
      pr.LZ.assign(v + owner * lz_total + o, v + owner * lz_total + o + pr.Rs);
      o += pr.Rs;
    }
  }
  // (both lists end with nws trailing empty lists, as the reference's do: verify.hip relies on it)
  eval_list.assign(nws, {});
  pf.comm_vars_at_ry_list.assign(nws, {});
  size_t k = 0;
  std::vector<CJob> cj;  // every evaluation's commitment in one host burst
  // <LZ, R> of every polynomial, one pool task each
  pool().parallel_for((int)polys.size(), [&](int q) {
    PolyRef& pr = polys[q];
    Fq ev = fq_zero();
    for (size_t m = 0; m < pr.Rs; m++) ev = fq_add(ev, fq_mul(pr.LZ[m], pr.R[m]));
    pr.ev = ev;
  });
  for (size_t i = 0; i < nws; i++) {
    eval_list.push_back({});
    for (size_t p = 0; p < wit.num_proofs[i].size(); p++, k++) {
      PolyRef& pr = polys[k];
      const Fq ev = pr.ev;
      size_t lni = lg2(pr.ni);
      eval_list[i].push_back(pr.ni >= Y ? ev : fq_mul(ev, ry_factors[ny - lni]));
      cj.push_back(CJob(g.gens_1, {ev}, fq_zero()));
    }
  }
  const std::vector<Pt> cv = commit_batch(g, cj);
  k = 0;
  for (size_t i = 0; i < nws; i++) {
    pf.comm_vars_at_ry_list.push_back({});
    for (size_t p = 0; p < wit.num_proofs[i].size(); p++) pf.comm_vars_at_ry_list[i].push_back(cv[k++]);
  }
  return 0;
}
// PolyEvalProof::prove_batched_instances_disjoint_rounds (dense_mlpoly.rs:861-960)
int Prover::polyeval_batched(std::vector<PolyRef>& polys) {
  t.protocol("polynomial evaluation proof");
  std::vector<std::pair<size_t, size_t>> shape;
  for (const PolyRef& pr : polys) shape.push_back({pr.np, pr.ni});
  const PeWalk wk = pe_walk_disjoint(shape);
  const FqV c = pe_coeff_powers(t.challenge("challenge_c"), wk.repeats());
  // the coefficients in the reference's order (the walk of pe_plan.hpp), then every LZ_list[k] += c LZ over the pool
  // (axpy_pool; config 4 adds 7 x 1024 products here, ~170 us on one thread)
  const size_t D = wk.first.size();
  std::vector<FqV> LZ_list(D), R_list(D);
  FqV Zc(D);
  std::vector<Axpy> ax;
  for (size_t q = 0; q < polys.size(); q++) {
    const PolyRef& pr = polys[q];
    const size_t k = wk.group[q];
    if (wk.opens(q)) {
      LZ_list[k] = pr.LZ, R_list[k] = pr.R, Zc[k] = pr.ev;
    } else {
      ax.push_back({&LZ_list[k], c[wk.exp[q]], &pr.LZ});
      Zc[k] = fq_add(Zc[k], fq_mul(c[wk.exp[q]], pr.ev));
    }
  }
  axpy_pool(ax);
  for (size_t k = 0; k < LZ_list.size(); k++) {
    DotProductProofLogP dp;
    Pt comm;
    int rc = dotproduct_log_prove(ctx, g, t, tape, LZ_list[k], fq_zero(), R_list[k], Zc[k], fq_zero(), &dp, &comm);
    if (rc) return rc;
    pf.evals.push_back(std::move(dp));
  }
  return 0;
}
// prefix_list (r1csproof.rs:577-606), the combined evaluation, the last equality proof and the returned challenges
void Prover::final_claims(const std::vector<FqV>& eval_list) {
  const FqV& rw = cy.rw;
  FqV prefix;
  {
    Fq one = fq_one();
    size_t W2 = npow2(nws);
    if (W2 == 1) prefix = {one};
    else if (W2 == 2) prefix = {fq_sub(one, rw[0]), rw[0]};
    else if (W2 == 4)
      prefix = {fq_mul(fq_sub(one, rw[0]), fq_sub(one, rw[1])), fq_mul(fq_sub(one, rw[0]), rw[1]),
                fq_mul(rw[0], fq_sub(one, rw[1])), fq_mul(rw[0], rw[1])};
    else
      for (int i = 0; i < 8; i++) {
        Fq a = (i & 4) ? rw[0] : fq_sub(one, rw[0]);
        Fq b = (i & 2) ? rw[1] : fq_sub(one, rw[1]);
        Fq cc = (i & 1) ? rw[2] : fq_sub(one, rw[2]);
        prefix.push_back(fq_mul(fq_mul(a, b), cc));
      }
  }
  FqV comb_list;
  for (size_t p = 0; p < P; p++) {
    Fq comb = fq_zero();
    for (size_t i = 0; i < nws; i++) {
      size_t pw = wit.num_proofs[i].size() == 1 ? 0 : p;
      comb = fq_add(comb, fq_mul(prefix[i], eval_list[i][pw]));
    }
    for (size_t q = 0; q < sh.nq - lg2(num_proofs[p]); q++) comb = fq_mul(comb, fq_sub(fq_one(), cy.rq[q]));
    comb_list.push_back(comb);
  }
  Fq eval_vars_at_ry = dense_eval_host(comb_list, cy.rp2);
  pf.comm_vars_at_ry = commit_batch(g, {CJob(g.gens_1, {eval_vars_at_ry}, fq_zero())})[0];
  Fq claim_post2 = fq_mul(fq_mul(cy.claims2[0], cy.claims2[1]), cy.claims2[2]);
  pf.eq2 = equality_prove(g, g.gens_1, t, tape, claim_post2, fq_zero(), claim_post2, cy.blind_post2);
  pf.claims_phase2[0] = cy.comm_Az;
  pf.claims_phase2[1] = cy.comm_Bz;
  pf.claims_phase2[2] = cy.comm_Cz;
  pf.claims_phase2[3] = cy.comm_prod;
  FqV rwry(rw);
  rwry.insert(rwry.end(), cy.ry.begin(), cy.ry.end());
  challenges = {cy.rp2, cy.rq_rev, cy.rx, rwry};
}


}  // namespace spg

using namespace spg;

// ------------------------------------------------------------------------------------ C-ABI
extern "C" int spg_transcript_new(const char* label, spg_transcript** out) {
  if (!label || !out) return SPG_E_ARG;
  *out = new spg_transcript(label);
  return SPG_OK;
}
extern "C" int spg_transcript_new_callbacks(spg_transcript_append_fn append, spg_transcript_challenge_fn challenge,
                                            void* user, spg_transcript** out) {
  if (!append || !challenge || !out) return SPG_E_ARG;
  spg_transcript* t = new spg_transcript("");  // its own merlin state is never used
  t->t.cb = std::make_shared<TrCallbacks>();
  t->t.cb->append = append;
  t->t.cb->challenge = challenge;
  t->t.cb->user = user;
  *out = t;
  return SPG_OK;
}
extern "C" int spg_transcript_append_message(spg_transcript* t, const char* label, const uint8_t* msg, size_t len) {
  if (!t || !label || (!msg && len)) return SPG_E_ARG;
  t->t.message(label, msg, len);
  return t->t.failed() ? SPG_E_CALLBACK : SPG_OK;
}
extern "C" int spg_transcript_append_scalar(spg_transcript* t, const char* label, const uint64_t* scalar_mont) {
  if (!t || !label || !scalar_mont) return SPG_E_ARG;
  t->t.scalar(label, ld_fq(scalar_mont));
  return t->t.failed() ? SPG_E_CALLBACK : SPG_OK;
}
extern "C" int spg_transcript_challenge_scalar(spg_transcript* t, const char* label, uint64_t* out_mont) {
  if (!t || !label || !out_mont) return SPG_E_ARG;
  st_fq(out_mont, t->t.challenge(label));
  return t->t.failed() ? SPG_E_CALLBACK : SPG_OK;
}
extern "C" int spg_transcript_challenge_bytes(spg_transcript* t, const char* label, uint8_t* out, size_t len) {
  if (!t || !label || (!out && len)) return SPG_E_ARG;
  t->t.challenge_bytes(label, out, len);
  return t->t.failed() ? SPG_E_CALLBACK : SPG_OK;
}
extern "C" int spg_transcript_free(spg_transcript* t) {
  delete t;
  return SPG_OK;
}
extern "C" int spg_random_tape_new(const char* name, const uint64_t* init_mont, spg_random_tape** out) {
  if (!name || !init_mont || !out) return SPG_E_ARG;
  *out = new spg_random_tape(name, ld_fq(init_mont));
  return SPG_OK;
}
extern "C" int spg_random_tape_scalar(spg_random_tape* tp, const char* label, uint64_t* out_mont) {
  if (!tp || !label || !out_mont) return SPG_E_ARG;
  st_fq(out_mont, tp->t.scalar(label));
  return SPG_OK;
}
extern "C" int spg_random_tape_free(spg_random_tape* tp) {
  delete tp;
  return SPG_OK;
}

extern "C" int spg_r1cs_gens_new(spg_ctx* ctx, const uint8_t* label, size_t label_len, size_t num_vars,
                                 spg_r1cs_gens** out) {
  if (!ctx || !label || !out || num_vars == 0) return SPG_E_ARG;
  size_t nv = lg2(num_vars);
  size_t n_pc = (size_t)1 << (nv - nv / 2);  // poly_commit_gens_new: 2^right
  spg_r1cs_gens* rg = new spg_r1cs_gens();
  ProverGens& g = rg->g;
  size_t n = std::max<size_t>(n_pc + 1, 4);
  int rc = spg_gens_derive(ctx, label, label_len, n, &g.dev);
  if (rc) {
    delete rg;
    return rc;
  }
  g.host.init(g.dev->compressed, n + 1);
  g.n_pc = n_pc;
  g.gens_n.G.resize(n_pc);
  for (size_t i = 0; i < n_pc; i++) g.gens_n.G[i] = i;
  g.gens_n.h = n_pc + 1;
  g.gens_1.G = {n_pc};
  g.gens_1.h = n_pc + 1;
  g.gens_4.G = {0, 1, 2, 3};
  g.gens_4.h = 4;
  // warm the host fixed-base tables of the sigma-protocol generators
  for (size_t i : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)4, n_pc, n_pc + 1}) g.host.get(i);
  *out = rg;
  return SPG_OK;
}
extern "C" int spg_r1cs_gens_free(spg_ctx* ctx, spg_r1cs_gens* g) {
  if (!g) return SPG_OK;
  spg_gens_free(ctx, g->g.dev);
  delete g;
  return SPG_OK;
}
extern "C" int spg_r1cs_gens_download(spg_ctx* ctx, const spg_r1cs_gens* g, uint8_t* out, size_t* count) {
  if (!ctx || !g || !count) return SPG_E_ARG;
  *count = g->g.dev->n + 1;
  if (out) memcpy(out, g->g.dev->compressed, 32 * (g->g.dev->n + 1));
  return SPG_OK;
}

extern "C" int spg_r1cs_inst_new(spg_ctx* ctx, const spg_r1cs_instance* ci, spg_r1cs_inst** out) {
  if (!ctx || !ci || !out || !ci->num_instances || !ci->num_cons || !ci->nnz || !ci->entries) return SPG_E_ARG;
  if (!is_pow2(ci->max_num_cons) || !is_pow2(ci->num_vars))
    return set_err(ctx, SPG_E_ARG, "max_num_cons and num_vars must be powers of two");
  size_t Pm = ci->num_instances;
  std::vector<uint32_t> rowptr, col, colptr, crow;
  std::vector<Fq> val, cval;
  spg_r1cs_inst* I = new spg_r1cs_inst();
  I->num_instances = Pm;
  I->max_num_cons = ci->max_num_cons;
  I->num_vars = ci->num_vars;
  I->num_cons.assign(ci->num_cons, ci->num_cons + Pm);
  for (size_t p = 0; p < Pm; p++) {
    size_t nc = ci->num_cons[p];
    if (!is_pow2(nc) || nc > ci->max_num_cons) {
      delete I;
      return set_err(ctx, SPG_E_ARG, "num_cons must be powers of two <= max_num_cons");
    }
    // CSR per matrix (counting sort by row, stable in entry order)
    for (int m = 0; m < 3; m++) {
      size_t nnz = ci->nnz[3 * p + m];
      I->nnz.push_back(nnz);
      const spg_sparse_entry* E = ci->entries[3 * p + m];
      if (nnz && !E) {
        delete I;
        return SPG_E_ARG;
      }
      std::vector<uint32_t> cnt(nc + 1, 0);
      for (size_t e = 0; e < nnz; e++) {
        if (E[e].row >= nc || E[e].col >= ci->num_vars) {
          delete I;
          return set_err(ctx, SPG_E_ARG, "sparse entry out of range");
        }
        cnt[E[e].row + 1]++;
      }
      for (size_t r = 0; r < nc; r++) cnt[r + 1] += cnt[r];
      I->rp_off.push_back(rowptr.size());
      size_t base = col.size();
      for (size_t r = 0; r <= nc; r++) rowptr.push_back((uint32_t)(base + cnt[r]));
      col.resize(base + nnz);
      val.resize(base + nnz);
      std::vector<uint32_t> fill(cnt.begin(), cnt.end() - 1);
      for (size_t e = 0; e < nnz; e++) {
        size_t d = base + fill[E[e].row]++;
        col[d] = (uint32_t)E[e].col;
        val[d] = ld_fq(E[e].val);
      }
    }
    // merged CSC over A, B, C with tagged rows
    size_t ncol = ci->num_vars;
    std::vector<uint32_t> cnt(ncol + 1, 0);
    for (int m = 0; m < 3; m++)
      for (size_t e = 0; e < ci->nnz[3 * p + m]; e++) cnt[ci->entries[3 * p + m][e].col + 1]++;
    for (size_t c = 0; c < ncol; c++) cnt[c + 1] += cnt[c];
    I->cp_off.push_back(colptr.size());
    size_t base = crow.size();
    for (size_t c = 0; c <= ncol; c++) colptr.push_back((uint32_t)(base + cnt[c]));
    crow.resize(base + cnt[ncol]);
    cval.resize(base + cnt[ncol]);
    std::vector<uint32_t> fill(cnt.begin(), cnt.end() - 1);
    for (int m = 0; m < 3; m++)
      for (size_t e = 0; e < ci->nnz[3 * p + m]; e++) {
        const spg_sparse_entry& en = ci->entries[3 * p + m][e];
        size_t d = base + fill[en.col]++;
        crow[d] = (uint32_t)(en.row * 4 + m);
        cval[d] = ld_fq(en.val);
      }
  }
  if (col.size() >= 0xffffffffULL || crow.size() >= 0xffffffffULL || ci->max_num_cons >= (1ull << 30)) {
    delete I;
    return set_err(ctx, SPG_E_ARG, "instance too large");
  }
  auto up = [&](void** d, const void* h, size_t bytes) -> int {
    if (hipMalloc(d, bytes ? bytes : 16) != hipSuccess) return SPG_E_NOMEM;
    if (bytes && hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) return SPG_E_HIP;
    return 0;
  };
  int rc = up((void**)&I->d_rowptr, rowptr.data(), rowptr.size() * 4);
  if (!rc) rc = up((void**)&I->d_col, col.data(), col.size() * 4);
  if (!rc) rc = up((void**)&I->d_val, val.data(), val.size() * sizeof(Fq));
  if (!rc) rc = up((void**)&I->d_colptr, colptr.data(), colptr.size() * 4);
  if (!rc) rc = up((void**)&I->d_crow, crow.data(), crow.size() * 4);
  if (!rc) rc = up((void**)&I->d_cval, cval.data(), cval.size() * sizeof(Fq));
  if (rc) {
    spg_r1cs_inst_free(ctx, I);
    return set_err(ctx, rc, "instance upload");
  }
  *out = I;
  return SPG_OK;
}
extern "C" int spg_r1cs_inst_free(spg_ctx* ctx, spg_r1cs_inst* I) {
  (void)ctx;
  if (!I) return SPG_OK;
  hipFree(I->d_rowptr);
  hipFree(I->d_col);
  hipFree(I->d_val);
  hipFree(I->d_colptr);
  hipFree(I->d_crow);
  hipFree(I->d_cval);
  delete I;
  return SPG_OK;
}

static int witness_new(spg_ctx* ctx, const spg_witness_sec* secs, size_t nws, size_t p0, size_t p1,
                       spg_r1cs_witness** out) {
  if (!ctx || !secs || !out || nws == 0) return SPG_E_ARG;
  if (nws > 8) return set_err(ctx, SPG_E_ARG, "at most 8 witness sections (prefix_list)");
  spg_r1cs_witness* W = new spg_r1cs_witness();
  W->nws = nws;
  W->num_proofs.resize(nws);
  W->num_inputs.resize(nws);
  W->off.resize(nws);
  size_t total = 0;
  for (size_t w = 0; w < nws; w++) {
    const spg_witness_sec& s = secs[w];
    if (!s.num_instances || !s.num_proofs || !s.num_inputs || !s.w) {
      delete W;
      return SPG_E_ARG;
    }
    for (size_t p = 0; p < s.num_instances; p++) {
      if (!is_pow2(s.num_proofs[p]) || !is_pow2(s.num_inputs[p])) {
        delete W;
        return set_err(ctx, SPG_E_ARG, "witness section sizes must be powers of two");
      }
      W->num_proofs[w].push_back(s.num_proofs[p]);
      W->num_inputs[w].push_back(s.num_inputs[p]);
      bool here = s.num_instances == 1 || (p >= p0 && p < p1);
      if (here && !s.w[p]) {
        delete W;
        return set_err(ctx, SPG_E_ARG, "missing witness data for a resident instance");
      }
      W->off[w].push_back(here ? total : kNotResident);
      if (here) total += s.num_proofs[p] * s.num_inputs[p];
    }
  }
  W->total = total;
  if (!(W->d_w = (Fq*)dev_cache_get(ctx, total * sizeof(Fq) + 64))) {
    delete W;
    return set_err(ctx, SPG_E_NOMEM, "witness upload");
  }
  W->ptr.resize(nws);
  for (size_t w = 0; w < nws; w++)
    for (uint64_t o : W->off[w]) W->ptr[w].push_back(o == kNotResident ? nullptr : W->d_w + o);
  for (size_t w = 0; w < nws; w++)
    for (size_t p = 0; p < secs[w].num_instances; p++) {
      if (W->off[w][p] == kNotResident) continue;
      size_t n = W->num_proofs[w][p] * W->num_inputs[w][p];
      // Scalar([u64; 4]) and Fq(u32[8]) share the little-endian byte image. Streamed through the page-locked ring
      // (h2d_stream: host pool copies, DMA on the upload stream): the call returns once the caller's buffers are read,
      // with the last chunks' DMAs in flight and the context stream ordered after them (round 6; a pageable
      // hipMemcpyAsync ran at ~26 GB/s and was synchronised here)
      if (int rc = h2d_stream(ctx, W->d_w + W->off[w][p], secs[w].w[p], n * sizeof(Fq))) {
        spg_r1cs_witness_free(ctx, W);
        return rc;
      }
    }
  *out = W;
  return SPG_OK;
}
namespace spg {
// witness sections assembled from host or device parts (SNARK::prove's ProverWitnessSecInfo lists); an
// existing *inout whose total size matches is refilled in place
int witness_from_parts(spg_ctx* ctx, const std::vector<WPart>& secs, spg_r1cs_witness** inout) {
  if (secs.empty() || secs.size() > 8) return set_err(ctx, SPG_E_ARG, "1..8 witness sections");
  size_t total = 0;
  for (auto& w : secs) {
    if (w.num_proofs.empty() || w.num_proofs.size() != w.num_inputs.size() || w.src.size() != w.num_proofs.size())
      return set_err(ctx, SPG_E_ARG, "witness part shape");
    for (size_t p = 0; p < w.num_proofs.size(); p++) {
      if (!is_pow2(w.num_proofs[p]) || !is_pow2(w.num_inputs[p]))
        return set_err(ctx, SPG_E_ARG, "witness section sizes must be powers of two");
      total += w.num_proofs[p] * w.num_inputs[p];
    }
  }
  // parts already resident on this device (SNARK::prove's block_vars and exec buffers, alive and unchanged for
  // the whole prove) are read in place; only host parts are copied into d_w
  // (a buffer on another GPU is copied like a host part: k_spmv / k_z_fill would otherwise read it across devices)
  auto on_device = [ctx](const void* q) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, q) != hipSuccess) {
      (void)hipGetLastError();  // an unregistered host pointer: not an error of the prove
      return false;
    }
    return a.type == hipMemoryTypeDevice && a.device == ctx->device;
  };
  const bool in_place = knob::wit_in_place();
  std::vector<std::vector<char>> dev(secs.size());
  size_t host_total = 0;
  for (size_t w = 0; w < secs.size(); w++)
    for (size_t p = 0; p < secs[w].num_proofs.size(); p++) {
      const bool d = in_place && on_device(secs[w].src[p]);
      dev[w].push_back(d);
      if (!d) host_total += secs[w].num_proofs[p] * secs[w].num_inputs[p];
    }
  (void)total;
  spg_r1cs_witness* W = *inout;
  if (W && W->total < host_total) {
    spg_r1cs_witness_free(ctx, W);
    W = nullptr;
  }
  if (!W) {
    W = new spg_r1cs_witness();
    if (hipMalloc(&W->d_w, host_total * sizeof(Fq) + 64) != hipSuccess) {
      delete W;
      *inout = nullptr;
      return set_err(ctx, SPG_E_NOMEM, "witness");
    }
    W->total = host_total;
  }
  *inout = W;
  W->nws = secs.size();
  W->num_proofs.assign(secs.size(), {});
  W->num_inputs.assign(secs.size(), {});
  W->off.assign(secs.size(), {});
  W->ptr.assign(secs.size(), {});
  size_t o = 0;
  for (size_t w = 0; w < secs.size(); w++)
    for (size_t p = 0; p < secs[w].num_proofs.size(); p++) {
      size_t n = secs[w].num_proofs[p] * secs[w].num_inputs[p];
      W->num_proofs[w].push_back(secs[w].num_proofs[p]);
      W->num_inputs[w].push_back(secs[w].num_inputs[p]);
      if (dev[w][p]) {
        W->off[w].push_back(0);
        W->ptr[w].push_back(secs[w].src[p]);
        continue;
      }
      W->off[w].push_back(o);
      W->ptr[w].push_back(W->d_w + o);
      SPG_HIP(ctx, hipMemcpyAsync(W->d_w + o, secs[w].src[p], n * sizeof(Fq), hipMemcpyDefault, ctx->stream));
      o += n;
    }
  return 0;
}
}  // namespace spg

extern "C" int spg_r1cs_witness_new(spg_ctx* ctx, const spg_witness_sec* secs, size_t nws, spg_r1cs_witness** out) {
  return witness_new(ctx, secs, nws, 0, ~(size_t)0, out);
}
extern "C" int spg_r1cs_witness_new_shard(spg_ctx* ctx, const spg_witness_sec* secs, size_t nws, size_t p0,
                                          size_t p1, spg_r1cs_witness** out) {
  return witness_new(ctx, secs, nws, p0, p1, out);
}
extern "C" int spg_r1cs_witness_free(spg_ctx* ctx, spg_r1cs_witness* W) {
  if (!W) return SPG_OK;
  if (ctx) {
    h2d_sync(ctx);  // a streamed upload into it may still be in flight
    dev_cache_put(ctx, W->d_w, W->total * sizeof(Fq) + 64);  // kept for the next witness of this size
  } else {
    hipFree(W->d_w);
  }
  delete W;
  return SPG_OK;
}

// argument check of spg_r1cs_prove; also derives this rank's instance shard [p0, p1)
static int check_prove_args(spg_ctx* ctx, const spg_r1cs_inst* inst, size_t num_instances, size_t max_num_proofs,
                            const size_t* num_proofs, size_t max_num_inputs, const size_t* num_inputs,
                            const spg_r1cs_witness* wit, size_t rank, size_t nranks, size_t* p0, size_t* p1) {
  if (!num_instances || !is_pow2(max_num_proofs) || !is_pow2(max_num_inputs))
    return set_err(ctx, SPG_E_ARG, "bad sizes");
  if (inst->num_instances != 1 && inst->num_instances != num_instances)
    return set_err(ctx, SPG_E_ARG, "instance count mismatch");
  if (wit->nws * max_num_inputs > inst->num_vars) return set_err(ctx, SPG_E_ARG, "witness wider than num_vars");
  for (size_t p = 0; p < num_instances; p++) {
    if (!is_pow2(num_proofs[p]) || num_proofs[p] > max_num_proofs || !is_pow2(num_inputs[p]) ||
        num_inputs[p] > max_num_inputs)
      return set_err(ctx, SPG_E_ARG, "num_proofs / num_inputs must be powers of two within the maxima");
  }
  for (size_t w = 0; w < wit->nws; w++) {
    if (wit->num_proofs[w].size() != 1 && wit->num_proofs[w].size() != num_instances)
      return set_err(ctx, SPG_E_ARG, "witness section instance count mismatch");
    for (size_t p = 0; p < num_instances; p++) {
      size_t pw = wit->num_proofs[w].size() == 1 ? 0 : p;
      if (wit->num_proofs[w][pw] != 1 && wit->num_proofs[w][pw] < num_proofs[p])
        return set_err(ctx, SPG_E_ARG, "witness section has fewer rows than num_proofs");
      if (wit->num_proofs[w][pw] > max_num_proofs) return set_err(ctx, SPG_E_ARG, "witness section too tall");
    }
  }
  if (nranks > num_instances) return set_err(ctx, SPG_E_ARG, "more ranks than instances");
  *p0 = Prover::shard_begin(num_instances, nranks, rank);
  *p1 = Prover::shard_begin(num_instances, nranks, rank + 1);
  for (size_t w = 0; w < wit->nws; w++) {
    if (wit->num_proofs[w].size() == 1) continue;
    for (size_t p = *p0; p < *p1; p++)
      if (wit->off[w][p] == kNotResident) return set_err(ctx, SPG_E_ARG, "witness shard does not hold instance");
  }
  return SPG_OK;
}

// the argument check on every rank, then the prover's sizes; shared by spg_r1cs_prove and spg_r1cs_sat_check
static int prover_args(spg_ctx* ctx, Prover& pr, const spg_r1cs_inst* inst, size_t num_instances,
                       size_t max_num_proofs, const size_t* num_proofs, size_t max_num_inputs,
                       const size_t* num_inputs, const spg_r1cs_witness* wit) {
  pr.rank = (size_t)ctx->rank;
  pr.nranks = (size_t)ctx->nranks;
  int rc_args = check_prove_args(ctx, inst, num_instances, max_num_proofs, num_proofs, max_num_inputs, num_inputs,
                                 wit, pr.rank, pr.nranks, &pr.p0, &pr.p1);
  if (pr.nranks > 1) {
    // a sharded prove starts with every rank agreeing on the argument check, so a rank-local failure
    // (e.g. a witness shard that does not hold this rank's instances) fails every rank alike instead of
    // leaving the others blocked in the first round's allgather
    int32_t mine = rc_args;
    std::vector<uint8_t> all;
    int rc = comm_allgather(ctx, Shard{(int)pr.rank, (int)pr.nranks}, 0, &mine, sizeof(mine), all);
    if (rc) return rc;
    for (size_t q = 0; q < pr.nranks && !rc_args; q++)
      if (((const int32_t*)all.data())[q]) rc_args = set_err(ctx, SPG_E_ARG, "a peer rank rejected its arguments");
  }
  if (rc_args) return rc_args;
  pr.P = num_instances;
  pr.max_np = max_num_proofs;
  pr.Y = max_num_inputs;
  pr.nws = wit->nws;
  pr.num_proofs.assign(num_proofs, num_proofs + num_instances);
  pr.num_inputs.assign(num_inputs, num_inputs + num_instances);
  return SPG_OK;
}

static int r1cs_prove_impl(spg_ctx* ctx, const spg_r1cs_gens* gens, const spg_r1cs_inst* inst,
                           size_t num_instances, size_t max_num_proofs, const size_t* num_proofs,
                           size_t max_num_inputs, const size_t* num_inputs, const spg_r1cs_witness* wit,
                           spg_transcript* transcript, spg_random_tape* tape, uint8_t* proof, size_t proof_cap,
                           size_t* proof_len, uint64_t* challenges_out, size_t* ch_lens) {
  Prover pr(ctx, const_cast<spg_r1cs_gens*>(gens)->g, *inst, *wit, transcript->t, tape->t);
  int rc = prover_args(ctx, pr, inst, num_instances, max_num_proofs, num_proofs, max_num_inputs, num_inputs, wit);
  if (rc) return rc;
  timer_start(ctx);
  rc = pr.run();
  timer_stop(ctx);
  if (rc == SPG_E_UNSAT) *proof_len = 0;  // check mode: no proof was written
  if (rc) return rc;
  Writer wr;
  pr.pf.ser(wr);
  *proof_len = wr.out.size();
  if (challenges_out && ch_lens) {
    size_t k = 0;
    for (int i = 0; i < 4; i++) {
      ch_lens[i] = pr.challenges[i].size();
      for (auto& c : pr.challenges[i]) st_fq(challenges_out + 4 * k++, c);
    }
  }
  if (!proof || wr.out.size() > proof_cap) return set_err(ctx, SPG_E_ARG, "proof buffer too small");
  memcpy(proof, wr.out.data(), wr.out.size());
  return SPG_OK;
}

extern "C" int spg_r1cs_prove(spg_ctx* ctx, const spg_r1cs_gens* gens, const spg_r1cs_inst* inst,
                              size_t num_instances, size_t max_num_proofs, const size_t* num_proofs,
                              size_t max_num_inputs, const size_t* num_inputs, const spg_r1cs_witness* wit,
                              spg_transcript* transcript, spg_random_tape* tape, uint8_t* proof, size_t proof_cap,
                              size_t* proof_len, uint64_t* challenges_out, size_t* ch_lens) {
  if (!ctx || !gens || !inst || !num_proofs || !num_inputs || !wit || !transcript || !tape || !proof_len)
    return SPG_E_ARG;
  HostPin pin;
  TrFailScope tfs(ctx, transcript->t);
  return tr_status(ctx, transcript->t,
                   r1cs_prove_impl(ctx, gens, inst, num_instances, max_num_proofs, num_proofs, max_num_inputs, num_inputs,
                                   wit, transcript, tape, proof, proof_cap, proof_len, challenges_out, ch_lens));
}

// R1CSInstance::is_sat (src/r1csinstance.rs:322-357) over every execution of every instance: the prover's own
// descriptor setup and k_spmv, then k_sat_check (satcheck.hip) -- no Z fill, transcript or generators (the Prover's
// references to them stay unused). A collective under spg_set_comm, as spg_r1cs_prove.
extern "C" int spg_r1cs_sat_check(spg_ctx* ctx, const spg_r1cs_inst* inst, size_t num_instances, size_t max_num_proofs,
                                  const size_t* num_proofs, size_t max_num_inputs, const size_t* num_inputs,
                                  const spg_r1cs_witness* wit, spg_sat_report* out) {
  if (!ctx || !inst || !num_proofs || !num_inputs || !wit || !out) return SPG_E_ARG;
  ProverGens none;
  Tr tr("sat_check");
  Tape tape("sat_check", fq_zero());
  Prover pr(ctx, none, *inst, *wit, tr, tape);
  int rc = prover_args(ctx, pr, inst, num_instances, max_num_proofs, num_proofs, max_num_inputs, num_inputs, wit);
  if (rc) return rc;
  pr.init_shape();
  ZFill zf;
  rc = pr.setup_desc(zf, false);
  if (!rc) rc = pr.launch_spmv();
  return pr.sat_check_tables(rc, out);
}

// R1CSInstance::multi_evaluate (src/r1csinstance.rs:583-596) / evaluate (:632-641):
// out[3p + m] = M_p(rx, ry) for M in (A, B, C), p < num_instances of the uploaded instance
extern "C" int spg_r1cs_multi_evaluate(spg_ctx* ctx, const spg_r1cs_inst* inst, const uint64_t* rx, size_t rx_len,
                                       const uint64_t* ry, size_t ry_len, uint64_t* out) {
  if (!ctx || !inst || !out || (!rx && rx_len) || (!ry && ry_len)) return SPG_E_ARG;
  if (rx_len > 32 || ry_len > 32 || ((size_t)1 << rx_len) < inst->max_num_cons ||
      ((size_t)1 << ry_len) < inst->num_vars)
    return set_err(ctx, SPG_E_ARG, "multi_evaluate: rx / ry shorter than the matrix dimensions");
  hipStream_t s = ctx->stream;
  const size_t Pm = inst->num_instances;
  // sharded over the ranks of spg_set_comm: every matrix's rows split (balanced), the 3 Pm partial sums added
  const Shard sh = ctx_shard(ctx);
  FqV vx(rx_len), vy(ry_len);
  for (size_t i = 0; i < rx_len; i++) vx[i] = ld_fq(rx + 4 * i);
  for (size_t i = 0; i < ry_len; i++) vy[i] = ld_fq(ry + 4 * i);
  Fq* erx = (Fq*)ws_get(ctx, Ws::R1csEvRx, (sizeof(Fq) << rx_len) + 64);
  Fq* ery = (Fq*)ws_get(ctx, Ws::R1csEvRy, (sizeof(Fq) << ry_len) + 64);
  std::vector<MatDesc> md(Pm);
  std::vector<uint32_t> rr(2 * Pm);
  size_t maxrows = 1;
  double visits = 0, rows = 0;
  for (size_t p = 0; p < Pm; p++) {
    for (int m = 0; m < 3; m++) md[p].rp[m] = inst->rp_off[3 * p + m];
    md[p].cp = inst->cp_off[p];
    rr[2 * p] = (uint32_t)shard_begin(inst->num_cons[p], sh.n, sh.rank);
    rr[2 * p + 1] = (uint32_t)shard_begin(inst->num_cons[p], sh.n, sh.rank + 1);
    maxrows = std::max<size_t>(maxrows, rr[2 * p + 1] - rr[2 * p]);
    const double frac = (double)(rr[2 * p + 1] - rr[2 * p]) / (double)std::max<size_t>(1, inst->num_cons[p]);
    visits += frac * (inst->nnz[3 * p] + inst->nnz[3 * p + 1] + inst->nnz[3 * p + 2]);
    rows += 3.0 * (rr[2 * p + 1] - rr[2 * p]);
  }
  const unsigned nblk = blocks_for(maxrows);
  Fq* part = (Fq*)ws_get(ctx, Ws::R1csEvPart, 3 * Pm * nblk * sizeof(Fq) + 64);
  Fq* dout = (Fq*)ws_get(ctx, Ws::R1csEvOut, 3 * Pm * sizeof(Fq) + 64);
  uint8_t* ddesc = (uint8_t*)ws_get(ctx, Ws::R1csEvDesc, Pm * (sizeof(MatDesc) + 8) + 64);
  if (!erx || !ery || !part || !dout || !ddesc) {
    int rc = set_err(ctx, SPG_E_NOMEM, "multi_evaluate");
    FqV none(3 * Pm);
    return comm_sum_fq(ctx, sh, rc, none.data(), 3 * Pm);
  }
  MatDesc* dmd = (MatDesc*)ddesc;
  uint32_t* drr = (uint32_t*)(ddesc + Pm * sizeof(MatDesc));
  {  // matrix descriptors and row ranges in one copy
    std::vector<uint8_t> h(Pm * sizeof(MatDesc) + 2 * Pm * 4);
    memcpy(h.data(), md.data(), Pm * sizeof(MatDesc));
    memcpy(h.data() + Pm * sizeof(MatDesc), rr.data(), 2 * Pm * 4);
    SPG_HIP(ctx, hipMemcpyAsync(dmd, h.data(), h.size(), hipMemcpyHostToDevice, s));
  }
  timer_start(ctx);
  int rc = eq_tables(ctx, {{vx, erx}, {vy, ery}});
  if (rc) return rc;
  {
    KScope ks(ctx, "sparse_eval", 68.0 * visits + 40.0 * rows);
    hipLaunchKernelGGL(k_sparse_eval, dim3(nblk, (unsigned)(3 * Pm)), dim3(256), 0, s, dmd, drr, inst->d_rowptr,
                       inst->d_col, inst->d_val, erx, ery, part);
    hipLaunchKernelGGL(k_sum_segments, dim3((unsigned)(3 * Pm)), dim3(256), 0, s, part, (int)nblk, dout);
  }
  SPG_HIP(ctx, hipGetLastError());
  timer_stop(ctx);
  std::vector<Fq> h(3 * Pm);
  SPG_HIP(ctx, hipMemcpyAsync(h.data(), dout, 3 * Pm * sizeof(Fq), hipMemcpyDeviceToHost, s));
  SPG_HIP(ctx, hipStreamSynchronize(s));
  float ms = 0.f;
  hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  ctx->last_us = ms * 1000.0;
  rc = comm_sum_fq(ctx, sh, 0, h.data(), 3 * Pm);
  if (rc) return rc;
  for (size_t i = 0; i < 3 * Pm; i++) st_fq(out + 4 * i, h[i]);
  return SPG_OK;
}

// R1CSInstance::multiply_vec_block (src/r1csinstance.rs:363-436; per (p, q): multiply_vec_disjoint_rounds,
// src/sparse_mlpoly.rs:454-472) as a seam: z_mat (p, q, w, x) -- instance p's num_proofs[p] x num_witness_secs x
// num_inputs[p] scalars, instances one after another, column c of a matrix reading z[p][q][c / max_num_inputs]
// [c % max_num_inputs] (zero past num_inputs[p]) -- into Az, Bz, Cz as new spg_pqx tables in
// DensePolynomialPqx::new_rev order (p, q_rev, x_rev: num_proofs, max_num_proofs, num_cons, max_num_cons; one w
// section). The prover's own k_spmv does the work, over section descriptors pointing into one upload of z.
extern "C" int spg_r1cs_multiply_vec_block(spg_ctx* ctx, const spg_r1cs_inst* inst, size_t num_instances,
                                           const size_t* num_proofs, size_t max_num_proofs, const size_t* num_inputs,
                                           size_t max_num_inputs, size_t num_witness_secs, const uint64_t* z_mont,
                                           spg_pqx** Az, spg_pqx** Bz, spg_pqx** Cz) {
  if (!ctx || !inst || !num_proofs || !num_inputs || !z_mont || !Az || !Bz || !Cz || num_instances == 0)
    return SPG_E_ARG;
  auto pow2 = [](size_t v) { return v && !(v & (v - 1)); };
  // r1csinstance.rs:375-376: one matrix for every instance, or one per instance
  if (!(inst->num_instances == 1 || inst->num_instances == num_instances))
    return set_err(ctx, SPG_E_ARG, "multiply_vec_block: the instance holds 1 or num_instances matrices");
  if (num_witness_secs == 0 || num_witness_secs > 8)  // (k_spmv keeps one block's section descriptors in LDS)
    return set_err(ctx, SPG_E_ARG, "multiply_vec_block: 1..8 witness sections");
  if (!pow2(max_num_proofs) || max_num_inputs == 0 || max_num_inputs > 0xffffffffu)
    return set_err(ctx, SPG_E_ARG, "multiply_vec_block: max_num_proofs a power of two, max_num_inputs > 0");
  const size_t P = num_instances;
  std::vector<size_t> ncons(P);
  size_t zt = 0, total = 0;
  for (size_t p = 0; p < P; p++) {
    const size_t pi = inst->num_instances == 1 ? 0 : p;
    ncons[p] = inst->num_cons[pi];
    if (!pow2(num_proofs[p]) || num_proofs[p] > max_num_proofs || num_inputs[p] > max_num_inputs || !pow2(ncons[p]))
      return set_err(ctx, SPG_E_ARG, "multiply_vec_block: num_proofs[p] (<= max) and num_cons powers of two, "
                                     "num_inputs[p] <= max_num_inputs");
    zt += num_proofs[p] * num_witness_secs * num_inputs[p];
    total += num_proofs[p] * ncons[p];
  }
  if (total >= ((size_t)1 << 31)) return set_err(ctx, SPG_E_ARG, "multiply_vec_block: at most 2^31 outputs");
  // z section-major on the device: section w of instance p as its own (q, x) matrix, as a witness section lies
  std::vector<Fq> zs(zt);
  std::vector<SecDesc> sd(num_witness_secs * P);
  std::vector<size_t> soff(num_witness_secs * P);
  {
    size_t o = 0;
    for (size_t w = 0; w < num_witness_secs; w++)
      for (size_t p = 0; p < P; p++) {
        soff[w * P + p] = o;
        o += num_proofs[p] * num_inputs[p];
      }
    const uint64_t* src = z_mont;
    for (size_t p = 0; p < P; p++)
      for (size_t q = 0; q < num_proofs[p]; q++)
        for (size_t w = 0; w < num_witness_secs; w++)
          for (size_t x = 0; x < num_inputs[p]; x++, src += 4)
            zs[soff[w * P + p] + q * num_inputs[p] + x] = ld_fq(src);
  }
  Fq* d_z = nullptr;
  void* d_desc = nullptr;
  std::vector<SpDesc> spd(P);
  std::vector<MatDesc> md(inst->num_instances);
  for (size_t p = 0; p < inst->num_instances; p++) {
    for (int m = 0; m < 3; m++) md[p].rp[m] = inst->rp_off[3 * p + m];
    md[p].cp = inst->cp_off[p];
  }
  size_t off = 0;
  for (size_t p = 0; p < P; p++) {
    spd[p].dom_off = spd[p].out_off = off;
    spd[p].pi = (uint32_t)(inst->num_instances == 1 ? 0 : p);
    spd[p].lg_q = (uint32_t)lg2(num_proofs[p]);
    spd[p].nrows = (uint32_t)ncons[p];
    spd[p].lg_rows = (uint32_t)lg2(ncons[p]);
    spd[p].ni = (uint32_t)num_inputs[p];
    spd[p].lg_ni = 0;
    off += num_proofs[p] * ncons[p];
  }
  const size_t b_sec = sd.size() * sizeof(SecDesc), b_sp = spd.size() * sizeof(SpDesc),
               b_md = md.size() * sizeof(MatDesc);
  spg_pqx* outs[3] = {new spg_pqx(), new spg_pqx(), new spg_pqx()};
  int rc = 0;
  auto fail = [&](int code, const char* msg) {
    rc = set_err(ctx, code, msg);
  };
  if (hipMalloc(&d_z, zt * sizeof(Fq) + 64) != hipSuccess || hipMalloc(&d_desc, b_sec + b_sp + b_md + 64) != hipSuccess)
    fail(SPG_E_NOMEM, "multiply_vec_block");
  for (int k = 0; k < 3 && !rc; k++) {
    PqxDev& T = outs[k]->T;
    T.zlen = P;
    size_t o = 0;
    for (size_t p = 0; p < P; p++) {
      T.off.push_back(o);
      T.anp.push_back(num_proofs[p]);
      T.anw.push_back(1);
      T.ani.push_back(ncons[p]);
      o += num_proofs[p] * ncons[p];
    }
    T.total = total;
    T.num_instances = 1;
    while (T.num_instances < P) T.num_instances *= 2;
    T.max_num_proofs = max_num_proofs;
    T.num_witness_secs = 1;
    T.max_num_inputs = inst->max_num_cons;
    T.num_proofs.assign(num_proofs, num_proofs + P);
    T.num_inputs = ncons;
    if (hipMalloc(&T.d, total * sizeof(Fq) + 64) != hipSuccess) fail(SPG_E_NOMEM, "multiply_vec_block outputs");
  }
  if (!rc) {
    for (size_t w = 0; w < num_witness_secs; w++)
      for (size_t p = 0; p < P; p++) {
        SecDesc& s = sd[w * P + p];
        s.w = d_z + soff[w * P + p];
        s.np = (uint32_t)num_proofs[p];
        s.ni = (uint32_t)num_inputs[p];
      }
    std::vector<uint8_t> blob(b_sec + b_sp + b_md);
    memcpy(blob.data(), sd.data(), b_sec);
    memcpy(blob.data() + b_sec, spd.data(), b_sp);
    memcpy(blob.data() + b_sec + b_sp, md.data(), b_md);
    uint8_t* dd = (uint8_t*)d_desc;
    if (hipMemcpy(d_z, zs.data(), zt * sizeof(Fq), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dd, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess)
      fail(SPG_E_HIP, "multiply_vec_block upload");
    if (!rc && total) {
      hipLaunchKernelGGL(k_spmv<false>, dim3(blocks_for(total)), dim3(256), 0, ctx->stream, (const SpDesc*)(dd + b_sec),
                         (int)P, (const MatDesc*)(dd + b_sec + b_sp), inst->d_rowptr, inst->d_col, inst->d_val,
                         (const SecDesc*)dd, (int)num_witness_secs, (uint32_t)max_num_inputs, outs[0]->T.d,
                         outs[1]->T.d, outs[2]->T.d, (uint64_t)total);
      if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
        fail(SPG_E_HIP, "multiply_vec_block launch");
    }
  }
  hipFree(d_z);
  hipFree(d_desc);
  if (rc) {
    for (spg_pqx* h : outs) {
      hipFree(h->T.d);
      delete h;
    }
    return rc;
  }
  *Az = outs[0];
  *Bz = outs[1];
  *Cz = outs[2];
  return SPG_OK;
}

// R1CSInstance::compute_eval_table_sparse_disjoint_rounds (src/r1csinstance.rs:484-534, src/sparse_mlpoly.rs:524-541)
// and prove_abc_gen (src/r1csproof.rs:430-465) as seams on a caller's eq(rx): k_abc over the handle's own matrices,
// into new spg_pqx tables of one proof row. split: A, B, C apart, x in natural order (DensePolynomialPqx::new);
// else r_A A + r_B B + r_C C in new_rev order, what the prover's phase2_prep builds.
static int abc_tables(spg_ctx* ctx, const char* what, const spg_r1cs_inst* inst, size_t num_instances,
                      size_t num_witness_secs, size_t max_num_inputs, const size_t* num_inputs, const spg_buf* evals_rx,
                      bool split, const Fq& rA, const Fq& rB, const Fq& rC, spg_pqx** outs) {
  const std::string w(what);
  // r1csinstance.rs:498-500, sparse_mlpoly.rs:532
  if (num_instances == 0 || !(inst->num_instances == 1 || inst->num_instances == num_instances))
    return set_err(ctx, SPG_E_ARG, w + ": the instance holds 1 or num_instances matrices");
  if (num_witness_secs == 0 || num_witness_secs > 8) return set_err(ctx, SPG_E_ARG, w + ": 1..8 witness sections");
  if (!is_pow2(max_num_inputs) || npow2(num_witness_secs) * max_num_inputs != inst->num_vars)
    return set_err(ctx, SPG_E_ARG, w + ": next_pow2(num_witness_secs) * max_num_inputs must equal num_vars");
  if (evals_rx->n < inst->max_num_cons) return set_err(ctx, SPG_E_ARG, w + ": evals_rx shorter than max_num_cons");
  const size_t Pm = inst->num_instances;
  for (size_t p = 0; p < Pm; p++)
    if (!is_pow2(num_inputs[p]) || num_inputs[p] > max_num_inputs)
      return set_err(ctx, SPG_E_ARG, w + ": num_inputs[p] must be powers of two <= max_num_inputs");
  const std::vector<size_t> cols(num_inputs, num_inputs + Pm);
  PqxDev shape = pqx_shape(std::vector<size_t>(Pm, 1), num_witness_secs, cols, npow2(Pm), 1, npow2(num_witness_secs),
                           max_num_inputs);
  const size_t total = shape.total;
  if (total >= ((size_t)1 << 31)) return set_err(ctx, SPG_E_ARG, w + ": at most 2^31 entries");
  std::vector<AbcDesc> ad(Pm);
  std::vector<MatDesc> md(Pm);
  for (size_t p = 0; p < Pm; p++) {
    ad[p].dom_off = ad[p].out_off = shape.off[p];
    ad[p].pi = (uint32_t)p;
    ad[p].ni = (uint32_t)num_inputs[p];
    ad[p].lg_ni = (uint32_t)lg2(num_inputs[p]);
    ad[p].pad = 0;
    for (int m = 0; m < 3; m++) md[p].rp[m] = inst->rp_off[3 * p + m];
    md[p].cp = inst->cp_off[p];
  }
  const int n_out = split ? 3 : 1;
  spg_pqx* h[3] = {nullptr, nullptr, nullptr};
  void* d_desc = nullptr;
  const size_t b_ad = Pm * sizeof(AbcDesc), b_md = Pm * sizeof(MatDesc);
  int rc = 0;
  if (hipMalloc(&d_desc, b_ad + b_md + 64) != hipSuccess) rc = set_err(ctx, SPG_E_NOMEM, w);
  for (int k = 0; k < n_out && !rc; k++) {
    h[k] = new spg_pqx();
    h[k]->T = shape;
    if (hipMalloc(&h[k]->T.d, total * sizeof(Fq) + 64) != hipSuccess) rc = set_err(ctx, SPG_E_NOMEM, w + " outputs");
  }
  if (!rc) {
    std::vector<uint8_t> blob(b_ad + b_md);
    memcpy(blob.data(), ad.data(), b_ad);
    memcpy(blob.data() + b_ad, md.data(), b_md);
    uint8_t* dd = (uint8_t*)d_desc;
    if (hipMemcpy(dd, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess)
      rc = set_err(ctx, SPG_E_HIP, w + " upload");
    if (!rc && total) {
      timer_start(ctx);
      const dim3 grid(blocks_for(total));
      if (split)
        hipLaunchKernelGGL(k_abc<true>, grid, dim3(256), 0, ctx->stream, (const AbcDesc*)dd, (int)Pm,
                           (const MatDesc*)(dd + b_ad), inst->d_colptr, inst->d_crow, inst->d_cval, evals_rx->d,
                           (uint32_t)max_num_inputs, rA, rB, rC, h[0]->T.d, h[1]->T.d, h[2]->T.d, (uint64_t)total);
      else
        hipLaunchKernelGGL(k_abc<false>, grid, dim3(256), 0, ctx->stream, (const AbcDesc*)dd, (int)Pm,
                           (const MatDesc*)(dd + b_ad), inst->d_colptr, inst->d_crow, inst->d_cval, evals_rx->d,
                           (uint32_t)max_num_inputs, rA, rB, rC, h[0]->T.d, (Fq*)nullptr, (Fq*)nullptr,
                           (uint64_t)total);
      timer_stop(ctx);
      if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
        rc = set_err(ctx, SPG_E_HIP, w + " launch");
      float ms = 0.f;
      if (!rc && hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) ctx->last_us = ms * 1000.0;
    }
  }
  hipFree(d_desc);
  if (rc) {
    for (spg_pqx* x : h)
      if (x) {
        hipFree(x->T.d);
        delete x;
      }
    return rc;
  }
  for (int k = 0; k < n_out; k++) outs[k] = h[k];
  return SPG_OK;
}

extern "C" int spg_r1cs_eval_tables(spg_ctx* ctx, const spg_r1cs_inst* inst, size_t num_instances,
                                    size_t num_witness_secs, size_t max_num_inputs, const size_t* num_inputs,
                                    const spg_buf* evals_rx, spg_pqx** A, spg_pqx** B, spg_pqx** C) {
  if (!ctx || !inst || !num_inputs || !evals_rx || !A || !B || !C) return SPG_E_ARG;
  spg_pqx* outs[3];
  const int rc = abc_tables(ctx, "r1cs_eval_tables", inst, num_instances, num_witness_secs, max_num_inputs, num_inputs,
                            evals_rx, true, fq_zero(), fq_zero(), fq_zero(), outs);
  if (rc) return rc;
  *A = outs[0];
  *B = outs[1];
  *C = outs[2];
  return SPG_OK;
}

extern "C" int spg_r1cs_abc_poly(spg_ctx* ctx, const spg_r1cs_inst* inst, size_t num_instances, size_t num_witness_secs,
                                 size_t max_num_inputs, const size_t* num_inputs, const spg_buf* evals_rx,
                                 const uint64_t* rA, const uint64_t* rB, const uint64_t* rC, spg_pqx** ABC) {
  if (!ctx || !inst || !num_inputs || !evals_rx || !rA || !rB || !rC || !ABC) return SPG_E_ARG;
  spg_pqx* outs[3];
  const int rc = abc_tables(ctx, "r1cs_abc_poly", inst, num_instances, num_witness_secs, max_num_inputs, num_inputs,
                            evals_rx, false, ld_fq(rA), ld_fq(rB), ld_fq(rC), outs);
  if (rc) return rc;
  *ABC = outs[0];
  return SPG_OK;
}
