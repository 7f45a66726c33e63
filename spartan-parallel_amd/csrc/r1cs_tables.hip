// spg — the device tables of R1CSProof::prove: every kernel that builds them, the only host code that launches those
// kernels, and the table setup the prover, spg_r1cs_sat_check and the seams share (r1cs_tables.hpp).
//   z_mat assembly into the (p, q_rev, w, x_rev) Z layout        r1csproof.rs:278-293, custom_dense_mlpoly.rs:67-111
//   multiply_vec_block (CSR SpMV for A, B, C at once)             r1csinstance.rs:363-436, sparse_mlpoly.rs:454-472
//   compute_eval_table_sparse_disjoint_rounds (CSC, eq-weighted)  r1csinstance.rs:484-534, sparse_mlpoly.rs:524-541
//   SparseMatPolynomial::evaluate_with_tables                     sparse_mlpoly.rs:427-436
//   DensePolynomial::bound of the witness sections                dense_mlpoly.rs:258-265
#include <optional>

#include "comm.hpp"
#include "hostpoly.hpp"
#include "knobs.hpp"
#include "lds.hpp"
#include "r1cs_tables.hpp"
#include "satcheck.hpp"

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

// ------------------------------------------------------------------------------------ launches
void launch_z_fill(spg_ctx* ctx, bool tiled, const ZDesc* dz, int n, const SecDesc* dsec, int nws, Fq* Z, size_t total) {
  KScope ks(ctx, "z_fill", 64.0 * total);
  if (tiled)  // (total is a multiple of 256 then, and so is every instance's offset)
    hipLaunchKernelGGL(k_z_fill_tiled, dim3((uint32_t)(total / 256)), dim3(256), 0, ctx->stream, dz, n, dsec, nws, Z);
  else
    hipLaunchKernelGGL(k_z_fill, dim3(blocks_for(total)), dim3(256), 0, ctx->stream, dz, n, dsec, nws, Z,
                       (uint64_t)total);
}

void launch_spmv(spg_ctx* ctx, bool scope, bool tiled, const SpDesc* dsd, int n, const MatDesc* dmd,
                 const spg_r1cs_inst& inst, const SecDesc* dsec, int nws, uint32_t Y, Fq* Az, Fq* Bz, Fq* Cz,
                 size_t total, double visits) {
  std::optional<KScope> ks;
  if (scope) ks.emplace(ctx, "spmv_block", 96.0 * total + 12.0 * total + 68.0 * visits);
  hipLaunchKernelGGL(tiled ? k_spmv<true> : k_spmv<false>, dim3(blocks_for(total)), dim3(256), 0, ctx->stream, dsd, n,
                     dmd, inst.d_rowptr, inst.d_col, inst.d_val, dsec, nws, Y, Az, Bz, Cz, (uint64_t)total);
}

void launch_abc(spg_ctx* ctx, bool scope, bool split, const AbcDesc* dad, int n, const MatDesc* dmd,
                const spg_r1cs_inst& inst, const Fq* eq, uint32_t Y, const Fq& rA, const Fq& rB, const Fq& rC, Fq* ABC,
                Fq* outB, Fq* outC, size_t total, double visits) {
  std::optional<KScope> ks;
  if (scope) ks.emplace(ctx, "eval_table_abc", 32.0 * total + 4.0 * total + 68.0 * visits);
  hipLaunchKernelGGL(split ? k_abc<true> : k_abc<false>, dim3(blocks_for(total)), dim3(256), 0, ctx->stream, dad, n, dmd,
                     inst.d_colptr, inst.d_crow, inst.d_cval, eq, Y, rA, rB, rC, ABC, outB, outC, (uint64_t)total);
}

void launch_sparse_eval(spg_ctx* ctx, const MatDesc* dmd, const uint32_t* drows, const spg_r1cs_inst& inst,
                        const Fq* eq_rx, const Fq* eq_ry, Fq* part, unsigned nblk, Fq* out, double visits, double rows) {
  const unsigned segs = (unsigned)(3 * inst.num_instances);
  KScope ks(ctx, "sparse_eval", 68.0 * visits + 40.0 * rows);
  hipLaunchKernelGGL(k_sparse_eval, dim3(nblk, segs), dim3(256), 0, ctx->stream, dmd, drows, inst.d_rowptr, inst.d_col,
                     inst.d_val, eq_rx, eq_ry, part);
  hipLaunchKernelGGL(k_sum_segments, dim3(segs), dim3(256), 0, ctx->stream, part, (int)nblk, out);
}

void launch_bound(spg_ctx* ctx, const std::vector<BoundBatch>& batches, const Fq* L, Fq* part, Fq* out) {
  double bytes = 0;
  for (const BoundBatch& b : batches)
    for (int k = 0; k < b.jobs.n; k++) {
      const BoundDesc& d = b.jobs.d[k];
      bytes += 32.0 * d.Ls * d.Rs + 32.0 * d.Ls + 64.0 * d.S * d.Rs;
    }
  KScope ks(ctx, "poly_bound", bytes);
  for (const BoundBatch& b : batches) {  // two launches per kBoundMax polynomials
    hipLaunchKernelGGL(k_bound_part_multi, dim3(b.nb), dim3(256), 0, ctx->stream, b.jobs, L, part);
    hipLaunchKernelGGL(k_sum_cols_multi, dim3(b.nc), dim3(256), 0, ctx->stream, b.jobs, part, out);
  }
}

int ZFill::queue() {
  if (queued) return 0;
  queued = true;
  const hipStream_t main_stream = c->stream;
  if (side) {
    SPG_HIP(c, hipEventRecord(c->ev_pre, main_stream));
    SPG_HIP(c, hipStreamWaitEvent(c->stream2, c->ev_pre, 0));
    c->stream = c->stream2;
  }
  launch_z_fill(c, tiled, dz, n, dsec, nws, Z, total);
  c->stream = main_stream;
  SPG_HIP(c, hipGetLastError());
  if (side) {
    SPG_HIP(c, hipEventRecord(c->ev_side, c->stream2));
    armed = true;
  }
  return 0;
}
int ZFill::join() {
  if (!armed) return 0;
  armed = false;
  return hipStreamWaitEvent(c->stream, c->ev_side, 0) == hipSuccess ? 0 : set_err(c, SPG_E_HIP, "z_fill join");
}

// ------------------------------------------------------------------------------------ the table setup
// the sizes of the prove and this rank's instances, from the arguments
R1csTables::R1csTables(spg_ctx* c, const spg_r1cs_inst& in, const spg_r1cs_witness& w, const R1csSizes& s)
    : ctx(c), inst(in), wit(w), sz(s) {
  sh.num_cons = inst.max_num_cons;
  sh.single = inst.num_instances == 1;
  std::vector<size_t> block_num_cons(sz.P);
  for (size_t p = 0; p < sz.P; p++) block_num_cons[p] = inst.num_cons[sh.single ? 0 : p];
  sh.np = lg2(npow2(sz.P)), sh.nq = lg2(sz.max_np), sh.nx = lg2(sh.num_cons), sh.nw = lg2(sz.nws), sh.ny = lg2(sz.Y);
  // this rank's instances [p0, p1): everything O(N) lives only here; nranks == 1 -> all of them
  sh.PLn = sz.p1 - sz.p0;
  sh.l_proofs.assign(sz.num_proofs.begin() + sz.p0, sz.num_proofs.begin() + sz.p1);
  sh.l_inputs.assign(sz.num_inputs.begin() + sz.p0, sz.num_inputs.begin() + sz.p1);
  sh.l_cons.assign(block_num_cons.begin() + sz.p0, block_num_cons.begin() + sz.p1);
}

template <class D>
int R1csTables::stage_desc(const std::vector<D>& v, D** dptr) {
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
int R1csTables::flush_desc() {
  if (desc_cur > desc_done)
    SPG_HIP(ctx, hipMemcpyAsync(desc_dev + desc_done, desc_host.data() + desc_done, desc_cur - desc_done,
                                hipMemcpyHostToDevice, ctx->stream));
  desc_done = desc_cur;
  return 0;
}

int R1csTables::setup_desc(ZFill& zf, bool want_z) {
  const size_t PLn = sh.PLn, P = sz.P, nws = sz.nws, p0 = sz.p0;
  Zp = pqx_shape(sh.l_proofs, nws, sh.l_inputs, npow2(P), sz.max_np, npow2(nws), sz.Y);
  const size_t ztot = Zp.total;
  if (want_z) {
    Zp.d = (Fq*)ws_get(ctx, Ws::R1csZ, ztot * sizeof(Fq) + 64);
    if (!Zp.d) return set_err(ctx, SPG_E_NOMEM, "Z table");
  }
  Az = pqx_shape(sh.l_proofs, 1, sh.l_cons, npow2(P), sz.max_np, 1, sh.num_cons);
  const size_t atot = Az.total;
  Az.d = (Fq*)ws_get(ctx, Ws::R1csAz, atot * sizeof(Fq) + 64);
  Bz = (Fq*)ws_get(ctx, Ws::R1csBz, atot * sizeof(Fq) + 64);
  Cz = (Fq*)ws_get(ctx, Ws::R1csCz, atot * sizeof(Fq) + 64);
  if (!Az.d || !Bz || !Cz) return set_err(ctx, SPG_E_NOMEM, "Az/Bz/Cz");
  // every descriptor of the setup kernels (Z fill, Az/Bz/Cz) goes up in one host-to-device copy
  ZDesc* dz = nullptr;
  bool z_tiled = knob::z_tiled();
  spmv_tiled_ = knob::spmv_tiled();
  visits_ = 0;
  std::vector<ZDesc> zd(PLn);
  std::vector<SecDesc> sd(nws * PLn);
  for (size_t p = 0; p < PLn; p++) {
    zd[p].dom_off = Zp.off[p];
    zd[p].z_off = Zp.off[p];
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
  const std::vector<SpDesc> spd = sp_descs(sh.l_proofs, sh.l_cons, sh.l_inputs, Az.off, p0, sh.single, true);
  for (size_t p = 0; p < PLn; p++) {
    const size_t pi = spd[p].pi;
    visits_ += (double)sh.l_proofs[p] * (inst.nnz[3 * pi] + inst.nnz[3 * pi + 1] + inst.nnz[3 * pi + 2]);
  }
  int rc = stage_desc(zd, &dz);
  if (!rc) rc = stage_desc(sd, &dsec_);
  if (!rc) rc = stage_desc(mat_descs(inst), &dmd);
  if (!rc) rc = stage_desc(spd, &dsd_);
  if (!rc) rc = flush_desc();
  if (rc) return rc;
  zf.c = ctx, zf.dz = dz, zf.dsec = dsec_, zf.n = (int)PLn, zf.nws = (int)nws;
  zf.Z = Zp.d, zf.total = ztot, zf.tiled = z_tiled, zf.side = knob::z_side();
  return 0;
}

int R1csTables::launch_spmv() {
  spg::launch_spmv(ctx, true, spmv_tiled_, dsd_, (int)sh.PLn, dmd, inst, dsec_, (int)sz.nws, (uint32_t)sz.Y, Az.d, Bz,
                   Cz, Az.total, visits_);
  SPG_HIP(ctx, hipGetLastError());
  return 0;
}

int R1csTables::launch_abc(const PqxDev& ABC, size_t pi0, const Fq* eq_rx, const Fq& rA, const Fq& rB, const Fq& rC) {
  const std::vector<AbcDesc> ad = abc_descs(ABC.ani, ABC.off, pi0);
  double visits = 0;
  for (const AbcDesc& d : ad) visits += inst.nnz[3 * d.pi] + inst.nnz[3 * d.pi + 1] + inst.nnz[3 * d.pi + 2];
  AbcDesc* dad;
  int rc = stage_desc(ad, &dad);
  if (!rc) rc = flush_desc();
  if (rc) return rc;
  spg::launch_abc(ctx, true, false, dad, (int)ad.size(), dmd, inst, eq_rx, (uint32_t)sz.Y, rA, rB, rC, ABC.d, nullptr,
                  nullptr, ABC.total, visits);
  SPG_HIP(ctx, hipGetLastError());
  return 0;
}

int R1csTables::sat_check(int rc, spg_sat_report* out) {
  std::vector<SatDesc> d;
  uint64_t total = 0;
  spg_sat_report mine;
  memset(&mine, 0, sizeof(mine));
  memset(out, 0, sizeof(*out));
  if (rc) {
  } else if (const char* why = sat_descs(sh.l_proofs.data(), sh.l_cons.data(), sh.PLn, &d, &total))
    rc = set_err(ctx, SPG_E_ARG, std::string("sat_check: ") + why);
  else if (total != Az.total)
    rc = set_err(ctx, SPG_E_ARG, "sat_check: descriptors do not cover the tables");
  else
    rc = sat_check_run(ctx, d, total, Az.d, Bz, Cz, &mine);
  if (mine.violations) mine.p += sz.p0;
  if (ctx->nranks == 1) {
    *out = mine;
    return rc;
  }
  // one framed allgather, outside the round plan: a rank whose check failed to run fails every rank with it
  std::vector<uint8_t> all;
  rc = comm_allgather(ctx, ctx_shard(ctx), rc, &mine, sizeof(mine), all);
  if (rc) return rc;
  sat_merge((const spg_sat_report*)all.data(), ctx->nranks, out);
  return 0;
}

}  // namespace spg
