// spg — the memory-checking and grand-product seams (include/spg.h "per-operation seams") on caller-owned device
// vectors (spg_buf), for a caller that runs its own protocol around them:
//   spg_hash_layer            Layers::build_hash_layer                    src/sparse_mlpoly.rs:612-687
//   spg_prodc_new / evaluate  ProductCircuit::new / evaluate              src/product_tree.rs:18-108
//   spg_prove_cubic_batched   SumcheckInstanceProof::prove_cubic_batched  src/sumcheck.rs:264-434
//   spg_prodc_prove_batched   ProductCircuitEvalProofBatched::prove       src/product_tree.rs:260-396
// The trees, the layer rounds and their launch forms are the SPARK prover's (layers.hip through prodc.hpp); this file
// hashes field-element operands, arranges caller vectors into the prover's tree layout and moves results back.
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "hostpoly.hpp"
#include "hpool.hpp"
#include "prodc.hpp"
#include "proto.hpp"
#include "sumcheck.hpp"

struct spg_prodc {
  size_t nc = 0, M = 0;
  spg::Fq* tree = nullptr;  // circuit c at c * 2M, level k at 2M - 2(M >> k)
  spg::FqV evals;           // ProductCircuit::evaluate of every circuit
  bool consumed = false;    // spg_prodc_prove_batched bound the layers
};

namespace spg {
namespace {

// a scalar as two 16-byte accesses (spg_buf data is hipMalloc'd: 32 i bytes in is 16-byte aligned)
__device__ __forceinline__ Fq ld_wide(const Fq* p) {
  const uint4 lo = ((const uint4*)p)[0], hi = ((const uint4*)p)[1];
  Fq r;
  r.l[0] = lo.x, r.l[1] = lo.y, r.l[2] = lo.z, r.l[3] = lo.w;
  r.l[4] = hi.x, r.l[5] = hi.y, r.l[6] = hi.z, r.l[7] = hi.w;
  return r;
}
__device__ __forceinline__ void st_wide(Fq* p, const Fq& v) {
  ((uint4*)p)[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  ((uint4*)p)[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// hash(addr, val, ts) = ts r_hash^2 + val r_hash + addr - r_multiset (sparse_mlpoly.rs:621-626) of the memory cells:
// init[i] = hash(i, table[i], 0), audit[i] = init[i] + audit_ts[i] r_hash^2; each cell read once, one pass
__global__ void __launch_bounds__(256) k_hash_mem_fq(const Fq* __restrict__ table, const Fq* __restrict__ audit_ts,
                                                     size_t cells, Fq rh, Fq rh2, Fq rms, Fq* __restrict__ init,
                                                     Fq* __restrict__ audit) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  const Fq v = ld_wide(table + i), ts = ld_wide(audit_ts + i);
  const Fq h0 = fq_sub(fq_add(fq_mul(v, rh), fq_from_u64(i)), rms);
  st_wide(init + i, h0);
  st_wide(audit + i, fq_add(fq_mul(ts, rh2), h0));
}
// instance k = blockIdx.y: reads[k][i] = hash(addr, val, ts), writes[k][i] = hash(addr, val, ts + 1) = reads + r_hash^2
struct HashOps {
  const Fq *addr, *val, *ts;
  Fq *rd, *wr;
};
__global__ void __launch_bounds__(256) k_hash_ops_fq(const HashOps* __restrict__ ops, size_t n_ops, Fq rh, Fq rh2,
                                                     Fq rms) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_ops) return;
  const HashOps o = ops[blockIdx.y];
  const Fq a = ld_wide(o.addr + i), v = ld_wide(o.val + i), ts = ld_wide(o.ts + i);
  const Fq rd = fq_sub(fq_add(fq_add(fq_mul(ts, rh2), fq_mul(v, rh)), a), rms);
  st_wide(o.rd + i, rd);
  st_wide(o.wr + i, fq_add(rd, rh2));
}

// vector b = blockIdx.y: dst[b * dst_stride + j * per + i] = src[b][i * s + j] for i < per, j < s (s = 1: a copy;
// s > 1: the s interleaved sub-vectors of src[b] one after another)
__global__ void __launch_bounds__(256) k_gather_vecs(const Fq* const* __restrict__ src, Fq* __restrict__ dst,
                                                     size_t dst_stride, size_t per, size_t s) {
  const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= per * s) return;
  const size_t j = u / per, i = u - j * per;
  st_wide(dst + blockIdx.y * dst_stride + u, ld_wide(src[blockIdx.y] + i * s + j));
}
// dst[b][j] = vals[b * s + j], j < s, b < nb
__global__ void __launch_bounds__(256) k_put_prefix(Fq* const* __restrict__ dst, const Fq* __restrict__ vals, size_t s,
                                                    size_t nb) {
  const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= nb * s) return;
  dst[u / s][u % s] = vals[u];
}

// host bytes into workspace slot `slot` (synchronous: `h` may be a temporary)
void* upload_desc(spg_ctx* ctx, Ws slot, const void* h, size_t bytes) {
  void* d = ws_get(ctx, slot, bytes + 64);
  if (!d) return nullptr;
  if (hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess)
    return nullptr;
  return d;
}

// n gathers of `per * s` scalars each (k_gather_vecs) in launches of at most 65535 vectors
int gather_vecs(spg_ctx* ctx, const std::vector<const Fq*>& src, Fq* dst, size_t dst_stride, size_t per, size_t s) {
  const Fq* const* d = (const Fq* const*)upload_desc(ctx, Ws::ProdcDesc, src.data(), src.size() * sizeof(Fq*));
  if (!d) return set_err(ctx, SPG_E_NOMEM, "vector descriptors");
  for (size_t b0 = 0; b0 < src.size(); b0 += 65535) {
    const size_t nb = std::min<size_t>(65535, src.size() - b0);
    hipLaunchKernelGGL(k_gather_vecs, dim3(nblk(per * s), (unsigned)nb), dim3(256), 0, ctx->stream, d + b0,
                       dst + b0 * dst_stride, dst_stride, per, s);
  }
  SPG_HIP(ctx, hipGetLastError());
  return 0;
}

// the first s scalars of every dst[b] = vals[b s ..], then waits: the bound values a layer's launches left on the host
int put_prefix(spg_ctx* ctx, const std::vector<Fq*>& dst, const FqV& vals, size_t s) {
  const size_t nb = dst.size(), pb = (nb * sizeof(Fq*) + 63) & ~(size_t)63;
  std::vector<uint8_t> h(pb + vals.size() * sizeof(Fq));
  memcpy(h.data(), dst.data(), nb * sizeof(Fq*));
  memcpy(h.data() + pb, vals.data(), vals.size() * sizeof(Fq));
  uint8_t* d = (uint8_t*)upload_desc(ctx, Ws::ProdcDesc, h.data(), h.size());
  if (!d) return set_err(ctx, SPG_E_NOMEM, "bound values upload");
  hipLaunchKernelGGL(k_put_prefix, dim3(nblk(nb * s)), dim3(256), 0, ctx->stream, (Fq* const*)d, (const Fq*)(d + pb), s,
                     nb);
  SPG_HIP(ctx, hipGetLastError());
  SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

bool pow2(size_t n) { return n && !(n & (n - 1)); }

void free_bufs(spg_ctx* ctx, std::vector<spg_buf*>& v) {
  for (spg_buf* b : v) spg_buf_free(ctx, b);
  v.clear();
}
spg_buf* new_buf(size_t n) {
  spg_buf* b = new spg_buf();
  b->n = n;
  if (hipMalloc(&b->d, n * sizeof(Fq)) != hipSuccess) {
    delete b;
    return nullptr;
  }
  return b;
}

}  // namespace
}  // namespace spg

using spg::Fq;
using spg::FqV;
using spg::Triple;

extern "C" int spg_hash_layer(spg_ctx* ctx, const spg_buf* eval_table, const spg_buf* const* addrs,
                              const spg_buf* const* derefs, const spg_buf* const* read_ts, size_t n,
                              const spg_buf* audit_ts, const uint64_t* r_hash_mont, const uint64_t* r_multiset_mont,
                              spg_buf** init, spg_buf** reads, spg_buf** writes, spg_buf** audit) {
  if (!ctx || !eval_table || !addrs || !derefs || !read_ts || !n || !audit_ts || !r_hash_mont || !r_multiset_mont ||
      !init || !reads || !writes || !audit)
    return SPG_E_ARG;
  for (size_t k = 0; k < n; k++)
    if (!addrs[k] || !derefs[k] || !read_ts[k]) return spg::set_err(ctx, SPG_E_ARG, "spg_hash_layer: null operand vector");
  const size_t cells = eval_table->n, ops = addrs[0]->n;
  if (!spg::pow2(cells) || audit_ts->n != cells)
    return spg::set_err(ctx, SPG_E_ARG, "spg_hash_layer: eval_table and audit_ts must hold one power-of-two number of cells");
  for (size_t k = 0; k < n; k++)
    if (!spg::pow2(ops) || addrs[k]->n != ops || derefs[k]->n != ops || read_ts[k]->n != ops)
      return spg::set_err(ctx, SPG_E_ARG, "spg_hash_layer: addrs, derefs, read_ts must hold one power-of-two number of ops");
  const Fq rh = spg::ld_fq(r_hash_mont), rh2 = spg::fq_mul(rh, rh), rms = spg::ld_fq(r_multiset_mont);
  std::vector<spg_buf*> made;
  auto fail = [&](int code, const char* msg) {
    spg::free_bufs(ctx, made);
    return spg::set_err(ctx, code, msg);
  };
  for (size_t k = 0; k < 2 + 2 * n; k++) {
    spg_buf* b = spg::new_buf(k < 2 ? cells : ops);
    if (!b) return fail(SPG_E_NOMEM, "spg_hash_layer: outputs");
    made.push_back(b);
  }
  std::vector<spg::HashOps> h(n);
  for (size_t k = 0; k < n; k++)
    h[k] = {addrs[k]->d, derefs[k]->d, read_ts[k]->d, made[2 + k]->d, made[2 + n + k]->d};
  const spg::HashOps* dops = (const spg::HashOps*)spg::upload_desc(ctx, spg::Ws::ProdcDesc, h.data(), n * sizeof(spg::HashOps));
  if (!dops) return fail(SPG_E_NOMEM, "spg_hash_layer: descriptors");
  {
    // algorithmic bytes: 2 scalars read and 2 written per cell, 3 read and 2 written per op
    spg::KScope ks(ctx, "seam_hash_layer", 128.0 * cells + 160.0 * n * ops);
    hipLaunchKernelGGL(spg::k_hash_mem_fq, dim3(spg::nblk(cells)), dim3(256), 0, ctx->stream, eval_table->d, audit_ts->d,
                       cells, rh, rh2, rms, made[0]->d, made[1]->d);
    for (size_t k0 = 0; k0 < n; k0 += 65535)
      hipLaunchKernelGGL(spg::k_hash_ops_fq, dim3(spg::nblk(ops), (unsigned)std::min<size_t>(65535, n - k0)), dim3(256), 0,
                         ctx->stream, dops + k0, ops, rh, rh2, rms);
  }
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
    return fail(SPG_E_HIP, "spg_hash_layer");
  *init = made[0];
  *audit = made[1];
  for (size_t k = 0; k < n; k++) {
    reads[k] = made[2 + k];
    writes[k] = made[2 + n + k];
  }
  return SPG_OK;
}

extern "C" int spg_prodc_new(spg_ctx* ctx, const spg_buf* const* polys, size_t nc, spg_prodc** out) {
  if (!ctx || !polys || !nc || !out) return SPG_E_ARG;
  for (size_t c = 0; c < nc; c++)
    if (!polys[c]) return spg::set_err(ctx, SPG_E_ARG, "spg_prodc_new: null polynomial");
  const size_t M = polys[0]->n;
  if (M < 2 || !spg::pow2(M)) return spg::set_err(ctx, SPG_E_ARG, "spg_prodc_new: M must be a power of two >= 2");
  for (size_t c = 0; c < nc; c++)
    if (polys[c]->n != M) return spg::set_err(ctx, SPG_E_ARG, "spg_prodc_new: the polynomials must have one length");
  if (nc > (size_t)0x7fffffff) return spg::set_err(ctx, SPG_E_ARG, "spg_prodc_new: too many circuits");
  spg_prodc* P = new spg_prodc();
  P->nc = nc;
  P->M = M;
  P->evals.resize(nc);
  auto fail = [&](int code, const char* msg) {
    spg_prodc_free(ctx, P);
    return spg::set_err(ctx, code, msg);
  };
  if (hipMalloc(&P->tree, nc * 2 * M * sizeof(Fq) + 64) != hipSuccess) return fail(SPG_E_NOMEM, "spg_prodc_new: trees");
  Fq* dtops = (Fq*)spg::ws_get(ctx, spg::Ws::ProdcTops, nc * sizeof(Fq) + 64);
  if (!dtops) return fail(SPG_E_NOMEM, "spg_prodc_new: tops");
  std::vector<const Fq*> src(nc);
  for (size_t c = 0; c < nc; c++) src[c] = polys[c]->d;
  int rc = spg::gather_vecs(ctx, src, P->tree, 2 * M, M, 1);  // the leaf level of every circuit, one launch
  if (!rc) rc = spg::tree_build(ctx, P->tree, nc, M, dtops);  // (k_tree_top: one workgroup per circuit, nc < 2^31)
  for (size_t c0 = 0; !rc && c0 < nc; c0 += spg::kResScalars)  // a result page of evaluations per download
    rc = spg::d2h_fq(ctx, dtops + c0, P->evals.data() + c0, std::min<size_t>(spg::kResScalars, nc - c0));
  if (rc) {
    spg_prodc_free(ctx, P);
    return rc;
  }
  *out = P;
  return SPG_OK;
}

extern "C" int spg_prodc_free(spg_ctx* ctx, spg_prodc* P) {
  (void)ctx;
  if (!P) return SPG_OK;
  if (P->tree) hipFree(P->tree);
  delete P;
  return SPG_OK;
}

extern "C" int spg_prodc_shape(const spg_prodc* P, size_t* nc, size_t* num_leaves) {
  if (!P) return SPG_E_ARG;
  if (nc) *nc = P->nc;
  if (num_leaves) *num_leaves = P->M;
  return SPG_OK;
}

extern "C" int spg_prodc_evaluate(spg_ctx* ctx, const spg_prodc* P, uint64_t* out_mont) {
  if (!ctx || !P || !out_mont) return SPG_E_ARG;
  if (P->consumed) return spg::set_err(ctx, SPG_E_ARG, "spg_prodc_evaluate: the circuits were consumed by a prove");
  for (size_t c = 0; c < P->nc; c++) spg::st_fq(out_mont + 4 * c, P->evals[c]);
  return SPG_OK;
}

extern "C" int spg_prodc_layer(spg_ctx* ctx, const spg_prodc* P, size_t c, size_t layer, uint64_t* left_mont,
                               uint64_t* right_mont) {
  if (!ctx || !P || !left_mont || !right_mont) return SPG_E_ARG;
  if (P->consumed) return spg::set_err(ctx, SPG_E_ARG, "spg_prodc_layer: the circuits were consumed by a prove");
  if (c >= P->nc || layer >= spg::lg2(P->M)) return spg::set_err(ctx, SPG_E_ARG, "spg_prodc_layer: no such circuit layer");
  const size_t M = P->M, half = M >> (layer + 1);
  const Fq* v = P->tree + c * 2 * M + (2 * M - 2 * (M >> layer));
  SPG_HIP(ctx, hipMemcpyAsync(left_mont, v, half * sizeof(Fq), hipMemcpyDeviceToHost, ctx->stream));
  SPG_HIP(ctx, hipMemcpyAsync(right_mont, v + half, half * sizeof(Fq), hipMemcpyDeviceToHost, ctx->stream));
  SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SPG_OK;
}

// One layer of the prover (layers.hip cubic_layer: its descriptors, launch plan and kernels) over the caller's vectors.
// With num_rounds = k the triples point at the caller's buffers. With num_rounds < k the s = 2^(k - num_rounds) entries
// that stay are the low index bits, which no round binds: the sumcheck is that of the s interleaved sub-vectors
// x[i s + j] (i < 2^num_rounds) of every vector side by side, each with its triple's coefficient, so the vectors are
// gathered into s sub-vectors each (every pair with a copy of C_par's) and run as s triples. Either way the layer's
// final entries are the bound values, written to the front of the caller's buffers.
static int prove_cubic_batched_impl(spg_ctx* ctx, const uint64_t* claim_mont, size_t num_rounds, spg_buf* const* A_par,
                                    spg_buf* const* B_par, size_t n_par, spg_buf* C_par, spg_buf* const* A_seq,
                                    spg_buf* const* B_seq, spg_buf* const* C_seq, size_t n_seq,
                                    const uint64_t* coeffs_mont, spg_transcript* t, uint64_t* polys_mont,
                                    uint64_t* r_mont, uint64_t* claims_par_mont, uint64_t* claims_seq_mont) {
  const char* shape = "spg_prove_cubic_batched: every vector must hold 2^k scalars, one k >= num_rounds";
  if (!claim_mont || !coeffs_mont || !t || (num_rounds && (!polys_mont || !r_mont)) || !(n_par + n_seq) ||
      (n_par && (!A_par || !B_par || !C_par || !claims_par_mont)) ||
      (n_seq && (!A_seq || !B_seq || !C_seq || !claims_seq_mont)) || (C_par && !claims_par_mont))
    return SPG_E_ARG;
  std::vector<spg_buf*> bufs;  // A_par.., B_par.., A_seq.., B_seq.., C_seq..
  for (spg_buf* const* g : {A_par, B_par})
    for (size_t i = 0; i < n_par; i++) bufs.push_back(g[i]);
  for (spg_buf* const* g : {A_seq, B_seq, C_seq})
    for (size_t i = 0; i < n_seq; i++) bufs.push_back(g[i]);
  for (spg_buf* b : bufs)
    if (!b) return spg::set_err(ctx, SPG_E_ARG, "spg_prove_cubic_batched: null vector");
  const size_t len = bufs[0]->n, k = spg::lg2(len);
  if (!spg::pow2(len) || num_rounds > k || (C_par && C_par->n != len)) return spg::set_err(ctx, SPG_E_ARG, shape);
  for (spg_buf* b : bufs)
    if (b->n != len) return spg::set_err(ctx, SPG_E_ARG, shape);
  const size_t s = len >> num_rounds, per = (size_t)1 << num_rounds, nt = (n_par + n_seq) * s;
  if (3 * nt + 1 > spg::kMboxScalars)
    return spg::set_err(ctx, SPG_E_ARG, "spg_prove_cubic_batched: too many triples x unbound entries for the mailbox");
  FqV coeffs(nt);
  for (size_t i = 0; i < n_par + n_seq; i++)
    for (size_t j = 0; j < s; j++) coeffs[i * s + j] = spg::ld_fq(coeffs_mont + 4 * i);
  std::vector<Triple> tr(nt);
  size_t nc = 0;
  if (s == 1) {
    nc = n_par;
    for (size_t i = 0; i < n_par; i++) tr[i] = {A_par[i]->d, B_par[i]->d, nullptr};
    for (size_t i = 0; i < n_seq; i++) tr[n_par + i] = {A_seq[i]->d, B_seq[i]->d, C_seq[i]->d};
  } else {
    // scratch vector 3 i + v = vector v (A, B, C) of triple i as its s sub-vectors back to back
    Fq* tmp = (Fq*)spg::ws_get(ctx, spg::Ws::ProdcTmp, 3 * (n_par + n_seq) * len * sizeof(Fq) + 64);
    if (!tmp) return spg::set_err(ctx, SPG_E_NOMEM, "spg_prove_cubic_batched: scratch");
    std::vector<const Fq*> src;
    for (size_t i = 0; i < n_par; i++) src.insert(src.end(), {A_par[i]->d, B_par[i]->d, C_par->d});
    for (size_t i = 0; i < n_seq; i++) src.insert(src.end(), {A_seq[i]->d, B_seq[i]->d, C_seq[i]->d});
    if (int rc = spg::gather_vecs(ctx, src, tmp, len, per, s)) return rc;
    for (size_t i = 0; i < n_par + n_seq; i++)
      for (size_t j = 0; j < s; j++) {
        Fq* v = tmp + 3 * i * len + j * per;
        tr[i * s + j] = {v, v + len, v + 2 * len};
      }
  }
  spg::LayerProofP proof;
  FqV r, fin;
  int rc = spg::cubic_layer(ctx, tr, nc, C_par ? C_par->d : nullptr, num_rounds, coeffs, spg::ld_fq(claim_mont), t->t,
                            &proof, &r, &fin);
  if (rc) return rc;
  // C_par with no pair to carry it through the layer: bound as the reference binds it, round by round
  if (C_par && !n_par)
    for (size_t j = 0; j < num_rounds; j++)
      if ((rc = spg::dev_fold_top(ctx, C_par->d, len >> j, r[j]))) return rc;
  // the bound values: vector v of triple i holds fin[3 (i s + j) + v], j < s
  std::vector<Fq*> dst;
  FqV vals;
  auto bound = [&](spg_buf* b, size_t i, int v) {
    dst.push_back(b->d);
    for (size_t j = 0; j < s; j++) vals.push_back(fin[3 * (i * s + j) + v]);
  };
  for (size_t i = 0; i < n_par; i++) bound(A_par[i], i, 0), bound(B_par[i], i, 1);
  if (n_par) bound(C_par, 0, 2);
  for (size_t i = 0; i < n_seq; i++)
    bound(A_seq[i], n_par + i, 0), bound(B_seq[i], n_par + i, 1), bound(C_seq[i], n_par + i, 2);
  if ((rc = spg::put_prefix(ctx, dst, vals, s))) return rc;  // (waits: C_par's folds above included)
  for (spg_buf* b : bufs) b->n = s;
  if (C_par) C_par->n = s;
  for (size_t j = 0; j < num_rounds; j++) {
    for (int q = 0; q < 3; q++) spg::st_fq(polys_mont + 12 * j + 4 * q, proof.polys[j][q]);
    spg::st_fq(r_mont + 4 * j, r[j]);
  }
  for (size_t i = 0; i < n_par; i++) {
    spg::st_fq(claims_par_mont + 4 * i, fin[3 * i * s]);
    spg::st_fq(claims_par_mont + 4 * (n_par + i), fin[3 * i * s + 1]);
  }
  if (n_par) {
    spg::st_fq(claims_par_mont + 8 * n_par, fin[2]);
  } else if (C_par) {
    Fq c0;
    if ((rc = spg::d2h_fq(ctx, C_par->d, &c0))) return rc;
    spg::st_fq(claims_par_mont, c0);
  }
  for (size_t i = 0; i < n_seq; i++)
    for (int v = 0; v < 3; v++) spg::st_fq(claims_seq_mont + 4 * (v * n_seq + i), fin[3 * (n_par + i) * s + v]);
  return SPG_OK;
}

extern "C" int spg_prove_cubic_batched(spg_ctx* ctx, const uint64_t* claim_mont, size_t num_rounds,
                                       spg_buf* const* A_par, spg_buf* const* B_par, size_t n_par, spg_buf* C_par,
                                       spg_buf* const* A_seq, spg_buf* const* B_seq, spg_buf* const* C_seq, size_t n_seq,
                                       const uint64_t* coeffs_mont, spg_transcript* t, uint64_t* polys_mont,
                                       uint64_t* r_mont, uint64_t* claims_par_mont, uint64_t* claims_seq_mont) {
  if (!ctx || !t) return SPG_E_ARG;
  spg::HostPin pin;
  return spg::tr_status(ctx, t->t,
                        prove_cubic_batched_impl(ctx, claim_mont, num_rounds, A_par, B_par, n_par, C_par, A_seq, B_seq,
                                                 C_seq, n_seq, coeffs_mont, t, polys_mont, r_mont, claims_par_mont,
                                                 claims_seq_mont));
}

static int prodc_prove_batched_impl(spg_ctx* ctx, spg_prodc* P, spg_buf* const* dotp, size_t nd, spg_transcript* t,
                                    uint8_t* proof, size_t cap, size_t* len, uint64_t* rand_mont, size_t* rand_len) {
  if (!P || !len || !rand_mont || !rand_len || (nd && !dotp) || (cap && !proof)) return SPG_E_ARG;
  if (P->consumed) return spg::set_err(ctx, SPG_E_ARG, "spg_prodc_prove_batched: the circuits were already consumed");
  const size_t M = P->M, nc = P->nc, L = spg::lg2(M);
  for (size_t i = 0; i < 3 * nd; i++)
    if (!dotp[i] || dotp[i]->n != M / 2)
      return spg::set_err(ctx, SPG_E_ARG, "spg_prodc_prove_batched: dot-product vectors must hold M / 2 scalars");
  if (3 * (nc + nd) + 1 > spg::kMboxScalars)
    return spg::set_err(ctx, SPG_E_ARG, "spg_prodc_prove_batched: too many circuits for the mailbox");
  // the struct's bincode size is known from the shapes: layer of j rounds = 8 + j (8 + 96) + 2 (8 + 32 nc)
  size_t need = 8 + 3 * (8 + 32 * nd);
  for (size_t j = 0; j < L; j++) need += 8 + j * 104 + 2 * (8 + 32 * nc);
  *len = need;
  if (cap < need) return spg::set_err(ctx, SPG_E_ARG, "spg_prodc_prove_batched: proof buffer too small");
  std::vector<Triple> dtr(nd);
  for (size_t k = 0; k < nd; k++) dtr[k] = {dotp[3 * k]->d, dotp[3 * k + 1]->d, dotp[3 * k + 2]->d};
  FqV dclaims(nd);
  int rc = spg::dotp_evaluate(ctx, dtr, M / 2, dclaims.data());
  if (rc) return rc;
  spg::TreeSh ts;
  ts.loc = P->tree;
  ts.m = M;
  spg::BatchedProofP out;
  FqV rand;
  P->consumed = true;
  rc = spg::batched_prove(ctx, ts, nc, M, P->evals, dtr, dclaims, t->t, &out, &rand, spg::Shard());
  if (rc) return rc;
  if (nd) {  // the dot-product vectors' bound values (one entry each): the layer's final claims
    std::vector<Fq*> dst;
    FqV vals;
    for (size_t k = 0; k < nd; k++)
      for (int v = 0; v < 3; v++) {
        dst.push_back(dotp[3 * k + v]->d);
        vals.push_back(out.dotp[v][k]);
      }
    if ((rc = spg::put_prefix(ctx, dst, vals, 1))) return rc;
    for (size_t i = 0; i < 3 * nd; i++) dotp[i]->n = 1;
  }
  spg::Writer w;
  out.ser(w);
  if (w.out.size() != need) return spg::set_err(ctx, SPG_E_ARG, "spg_prodc_prove_batched: unexpected proof size");
  memcpy(proof, w.out.data(), need);
  for (size_t i = 0; i < rand.size(); i++) spg::st_fq(rand_mont + 4 * i, rand[i]);
  *rand_len = rand.size();
  return SPG_OK;
}

extern "C" int spg_prodc_prove_batched(spg_ctx* ctx, spg_prodc* P, spg_buf* const* dotp, size_t nd, spg_transcript* t,
                                       uint8_t* proof, size_t cap, size_t* len, uint64_t* rand_mont, size_t* rand_len) {
  if (!ctx || !t) return SPG_E_ARG;
  spg::HostPin pin;
  return spg::tr_status(ctx, t->t, prodc_prove_batched_impl(ctx, P, dotp, nd, t, proof, cap, len, rand_mont, rand_len));
}
