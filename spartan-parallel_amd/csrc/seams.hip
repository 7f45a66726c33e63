// spg — the reference's finer per-operation seams on device-resident vectors (spg_buf): a caller that
// drives its own protocol binds these instead of the whole-proof entries. Each call runs on the context stream and
// returns when its result is ready; the vectors stay in HBM between calls.
//   spg_buf_bound_top      DensePolynomial::bound_poly_var_top   src/dense_mlpoly.rs:267-275
//   spg_buf_bound_bot      DensePolynomial::bound_poly_var_bot   src/dense_mlpoly.rs:350-358
//   spg_buf_evaluate       DensePolynomial::evaluate             src/dense_mlpoly.rs:361-367
//   spg_cubic_round_evals  one round of prove_cubic, comb A B C  src/sumcheck.rs:207-236, src/product_tree.rs:185-189
//   spg_prove_cubic        SumcheckInstanceProof::prove_cubic    src/sumcheck.rs:193-262
//   spg_pqx_*              DensePolynomialPqx new / new_rev / bound_poly / bound_poly_vars_rq / evaluate
//                                                                src/custom_dense_mlpoly.rs:45-111, 180-333
//   spg_zk_phase1_prove    ZKSumcheckInstanceProof::prove_cubic_with_additive_term_disjoint_rounds  src/sumcheck.rs:1067-1380
//   spg_zk_phase2_prove    ZKSumcheckInstanceProof::prove_cubic_disjoint_rounds                     src/sumcheck.rs:788-1065
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "hostpoly.hpp"
#include "proto.hpp"
#include "zk_rounds.hpp"

namespace spg {
namespace {


// bound_poly_var_bot: out[i] = in[2i] + r (in[2i + 1] - in[2i]); out-of-place (in place, a workgroup's outputs would
// overwrite entries another workgroup still reads)
__global__ void k_fold_bot(const Fq* __restrict__ in, Fq* __restrict__ out, size_t n, Fq r) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fq lo = in[2 * i];
  out[i] = fq_add(lo, fq_mul(r, fq_sub(in[2 * i + 1], lo)));
}

// the three tables of a prove_cubic round bound to the same r (bound_poly_var_top of each) in one launch
__global__ void k_fold_top3(Fq* __restrict__ A, Fq* __restrict__ B, Fq* __restrict__ C, size_t n, Fq r) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fq a = A[i], b = B[i], c = C[i];
  A[i] = fq_add(a, fq_mul(r, fq_sub(A[i + n], a)));
  B[i] = fq_add(b, fq_mul(r, fq_sub(B[i + n], b)));
  C[i] = fq_add(c, fq_mul(r, fq_sub(C[i + n], c)));
}

// DensePolynomialPqx::new_rev (src/custom_dense_mlpoly.rs:67-111) of one caller buffer: instance p's (q, w, x) block
// keeps its place and size, Z[p][rev(q)][w][rev(x)] = z[p][q][w][x] with rev over lg num_proofs[p] / lg num_inputs[p]
// bits (rev_bits(q, max_num_proofs) / step_q of the reference). One element per lane, reads in order.
struct RevDesc {
  uint32_t off, lg_q, lg_ni, nws;  // element offset of the instance (totals stay below 2^31)
};
__device__ __forceinline__ uint32_t brev_lg(uint32_t v, uint32_t lg) { return lg ? (__brev(v) >> (32 - lg)) : 0u; }
__global__ void __launch_bounds__(256) k_pqx_new_rev(const RevDesc* __restrict__ rd, int P, const Fq* __restrict__ z,
                                                     Fq* __restrict__ Z, uint32_t total) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  int lo = 0, hi = P - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rd[mid].off <= t) lo = mid;
    else hi = mid - 1;
  }
  const RevDesc d = rd[lo];
  const uint32_t loc = t - d.off;
  const uint32_t x = loc & ((1u << d.lg_ni) - 1), rest = loc >> d.lg_ni;
  const uint32_t w = rest % d.nws, q = rest / d.nws;
  Z[d.off + (((size_t)brev_lg(q, d.lg_q) * d.nws + w) << d.lg_ni) + brev_lg(x, d.lg_ni)] = z[t];
}

bool pow2(size_t n) { return n && !(n & (n - 1)); }

int d2h(spg_ctx* ctx, void* dst, const void* src, size_t bytes) {
  SPG_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

// (e0, e2, e3) of a prove_cubic round over A, B, C of equal even length
int cubic_round(spg_ctx* ctx, const spg_buf* A, const spg_buf* B, const spg_buf* C, Fq out3[3]) {
  const size_t half = A->n / 2;
  Fq* partials = (Fq*)ws_get(ctx, Ws::SeamPart, 3 * kScGridMax * sizeof(Fq) + 64);
  if (!partials) return set_err(ctx, SPG_E_NOMEM, "cubic round partials");
  return cubic_eval(ctx, A->d, B->d, C->d, half, partials, out3);
}

}  // namespace
}  // namespace spg

using spg::Fq;

extern "C" int spg_buf_bound_top(spg_ctx* ctx, spg_buf* b, const uint64_t* r_mont) {
  if (!ctx || !b || !r_mont) return SPG_E_ARG;
  if (b->n < 2 || (b->n & 1)) return spg::set_err(ctx, SPG_E_ARG, "spg_buf_bound_top: length must be even and >= 2");
  int rc = spg::dev_fold_top(ctx, b->d, b->n, spg::ld_fq(r_mont));
  if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = spg::set_err(ctx, SPG_E_HIP, "spg_buf_bound_top");
  if (!rc) b->n /= 2;  // Z.truncate(n): the device allocation keeps its size
  return rc;
}

extern "C" int spg_buf_bound_bot(spg_ctx* ctx, spg_buf* b, const uint64_t* r_mont) {
  if (!ctx || !b || !r_mont) return SPG_E_ARG;
  if (b->n < 2 || (b->n & 1)) return spg::set_err(ctx, SPG_E_ARG, "spg_buf_bound_bot: length must be even and >= 2");
  const size_t n = b->n / 2;
  Fq* tmp = (Fq*)spg::ws_get(ctx, spg::Ws::SeamTmp, n * sizeof(Fq) + 64);
  if (!tmp) return spg::set_err(ctx, SPG_E_NOMEM, "spg_buf_bound_bot");
  hipLaunchKernelGGL(spg::k_fold_bot, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, b->d, tmp, n,
                     spg::ld_fq(r_mont));
  SPG_HIP(ctx, hipGetLastError());
  SPG_HIP(ctx, hipMemcpyAsync(b->d, tmp, n * sizeof(Fq), hipMemcpyDeviceToDevice, ctx->stream));
  SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  b->n = n;
  return SPG_OK;
}

// DensePolynomial::evaluate: <Z, chi(r)> with chi = EqPolynomial::evals(r), r[0] the index's most significant bit.
// On the device as ell successive bound_poly_var_top folds of a copy by r[0], r[1], ... : the fold by r_0 leaves
// Z'[i] = (1 - r_0) Z[i] + r_0 Z[i + n/2], so after all ell folds Z''[0] = sum_i chi_i(r) Z[i], the same field value
// as the reference's dot product (exact arithmetic, no rounding to differ).
extern "C" int spg_buf_evaluate(spg_ctx* ctx, const spg_buf* b, const uint64_t* r_mont, size_t ell, uint64_t* out_mont) {
  if (!ctx || !b || !out_mont || (!r_mont && ell)) return SPG_E_ARG;
  if (ell >= 64 || b->n != ((size_t)1 << ell))
    return spg::set_err(ctx, SPG_E_ARG, "spg_buf_evaluate: the vector must hold 2^ell scalars");
  Fq* tmp = (Fq*)spg::ws_get(ctx, spg::Ws::SeamTmp, b->n * sizeof(Fq) + 64);
  if (!tmp) return spg::set_err(ctx, SPG_E_NOMEM, "spg_buf_evaluate");
  SPG_HIP(ctx, hipMemcpyAsync(tmp, b->d, b->n * sizeof(Fq), hipMemcpyDeviceToDevice, ctx->stream));
  size_t len = b->n;
  for (size_t j = 0; j < ell; j++, len /= 2) {
    const int rc = spg::dev_fold_top(ctx, tmp, len, spg::ld_fq(r_mont + 4 * j));
    if (rc) return rc;
  }
  Fq v;
  if (int rc = spg::d2h(ctx, &v, tmp, sizeof(Fq))) return rc;
  spg::st_fq(out_mont, v);
  return SPG_OK;
}

extern "C" int spg_cubic_round_evals(spg_ctx* ctx, const spg_buf* A, const spg_buf* B, const spg_buf* C,
                                     uint64_t* out3_mont) {
  if (!ctx || !A || !B || !C || !out3_mont) return SPG_E_ARG;
  if (A->n < 2 || (A->n & 1) || B->n != A->n || C->n != A->n)
    return spg::set_err(ctx, SPG_E_ARG, "spg_cubic_round_evals: A, B, C must have one even length >= 2");
  Fq e[3];
  if (int rc = spg::cubic_round(ctx, A, B, C, e)) return rc;
  for (int k = 0; k < 3; k++) spg::st_fq(out3_mont + 4 * k, e[k]);
  return SPG_OK;
}

// per round: (e0, e2, e3) on the device, UniPoly::from_evals([e0, e - e0, e2, e3]) and its transcript append on the
// host, the challenge, then A, B, C bound in one launch (k_fold_top3) and e = poly(r_j)
extern "C" int spg_prove_cubic(spg_ctx* ctx, const uint64_t* claim_mont, size_t num_rounds, spg_buf* A, spg_buf* B,
                               spg_buf* C, spg_transcript* t, uint64_t* polys_mont, uint64_t* r_mont,
                               uint64_t* claims_mont) {
  if (!ctx || !claim_mont || !A || !B || !C || !t || !claims_mont || (num_rounds && (!polys_mont || !r_mont)))
    return SPG_E_ARG;
  size_t lg = 0;
  while (lg < 63 && ((size_t)1 << lg) < A->n) lg++;
  if (B->n != A->n || C->n != A->n || !spg::pow2(A->n) || num_rounds > lg)
    return spg::set_err(ctx, SPG_E_ARG, "spg_prove_cubic: A, B, C must hold 2^k scalars each, k >= num_rounds");
  Fq e = spg::ld_fq(claim_mont);
  for (size_t j = 0; j < num_rounds; j++) {
    Fq ev[4];
    if (int rc = spg::cubic_round(ctx, A, B, C, ev)) return spg::tr_status(ctx, t->t, rc);
    const Fq evals[4] = {ev[0], spg::fq_sub(e, ev[0]), ev[1], ev[2]};
    const spg::FqV c = spg::uni_from_evals3(evals);
    t->t.msg("poly", "UniPoly_begin");  // UniPoly::append_to_transcript (src/unipoly.rs:112-120)
    for (const Fq& x : c) t->t.scalar("coeff", x);
    t->t.msg("poly", "UniPoly_end");
    const Fq r = t->t.challenge("challenge_nextround");
    const size_t n = A->n / 2;
    hipLaunchKernelGGL(spg::k_fold_top3, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, A->d, B->d,
                       C->d, n, r);
    SPG_HIP(ctx, hipGetLastError());
    A->n = B->n = C->n = n;
    e = spg::uni_eval(c, r);
    // CompressedUniPoly: the coefficients without the linear term (src/unipoly.rs:82-87)
    spg::st_fq(polys_mont + 12 * j, c[0]);
    spg::st_fq(polys_mont + 12 * j + 4, c[2]);
    spg::st_fq(polys_mont + 12 * j + 8, c[3]);
    spg::st_fq(r_mont + 4 * j, r);
  }
  Fq fin[3];
  for (int k = 0; k < 3; k++) {
    const spg_buf* v = k == 0 ? A : k == 1 ? B : C;
    SPG_HIP(ctx, hipMemcpyAsync(&fin[k], v->d, sizeof(Fq), hipMemcpyDeviceToHost, ctx->stream));
  }
  SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 3; k++) spg::st_fq(claims_mont + 4 * k, fin[k]);
  return spg::tr_status(ctx, t->t, SPG_OK);
}

// ---- DensePolynomialPqx (src/custom_dense_mlpoly.rs:22-359) as a handle over the prover's own ragged HBM layout
// (pqx.hpp: instance p owns num_proofs[p] x nws x num_inputs[p] scalars at off[p]; folds rewrite the low halves in
// place and shrink the current sizes, the allocation stays, so index() keeps the reference's bounds semantics)

namespace {
int pqx_bind_one(spg_ctx* ctx, spg::PqxDev& T, const Fq& r, int mode) {
  if (mode < spg::MODE_P || mode > spg::MODE_X) return spg::set_err(ctx, SPG_E_ARG, "DensePolynomialPqx: mode 1..4");
  // bound_poly_p's assert_eq!(max_num_proofs, 1), assert_eq!(max_num_inputs, 1) (custom_dense_mlpoly.rs:206-207)
  if (mode == spg::MODE_P && (T.max_num_proofs != 1 || T.max_num_inputs != 1))
    return spg::set_err(ctx, SPG_E_ARG, "DensePolynomialPqx::bound_poly_p: bind every q and x variable first");
  return spg::pqx_bound(ctx, T, nullptr, nullptr, r, mode);
}
}  // namespace

namespace {
// the checks, descriptors and allocation DensePolynomialPqx::new and ::new_rev share: all sizes powers of two within
// the maxima, fewer than 2^31 scalars (the fold kernels index the domain with 32-bit lanes)
int pqx_alloc(spg_ctx* ctx, const char* what, bool have_z, size_t num_instances, const size_t* num_proofs,
              size_t max_num_proofs, size_t num_witness_secs, const size_t* num_inputs, size_t max_num_inputs,
              spg_pqx** out) {
  const std::string w(what);
  if (!spg::pow2(max_num_proofs) || !spg::pow2(max_num_inputs))
    return spg::set_err(ctx, SPG_E_ARG, w + ": max_num_proofs / max_num_inputs must be powers of two");
  spg_pqx* h = new spg_pqx();
  spg::PqxDev& T = h->T;
  T.zlen = num_instances;
  size_t total = 0;
  for (size_t p = 0; p < num_instances; p++) {
    if (!spg::pow2(num_proofs[p]) || num_proofs[p] > max_num_proofs || !spg::pow2(num_inputs[p]) ||
        num_inputs[p] > max_num_inputs) {
      delete h;
      return spg::set_err(ctx, SPG_E_ARG, w + ": num_proofs[p] / num_inputs[p] must be powers of two <= max");
    }
    T.off.push_back(total);
    T.anp.push_back(num_proofs[p]);
    T.anw.push_back(num_witness_secs);
    T.ani.push_back(num_inputs[p]);
    total += num_proofs[p] * num_witness_secs * num_inputs[p];
  }
  if (total >= ((size_t)1 << 31) || !have_z) {
    delete h;
    return spg::set_err(ctx, SPG_E_ARG, w + ": at most 2^31 scalars, z required");
  }
  T.total = total;
  T.num_instances = 1;
  while (T.num_instances < num_instances) T.num_instances *= 2;
  T.num_witness_secs = 1;
  while (T.num_witness_secs < num_witness_secs) T.num_witness_secs *= 2;
  T.max_num_proofs = max_num_proofs;
  T.max_num_inputs = max_num_inputs;
  T.num_proofs.assign(num_proofs, num_proofs + num_instances);
  T.num_inputs.assign(num_inputs, num_inputs + num_instances);
  if (hipMalloc(&T.d, total * sizeof(Fq) + 64) != hipSuccess) {
    delete h;
    return spg::set_err(ctx, SPG_E_NOMEM, w);
  }
  *out = h;
  return SPG_OK;
}

// new_rev of `z` (device, the table's total scalars in (p, q, w, x) order) into a new handle
int pqx_new_rev_dev(spg_ctx* ctx, const char* what, const Fq* z, bool have_z, size_t num_instances,
                    const size_t* num_proofs, size_t max_num_proofs, size_t num_witness_secs, const size_t* num_inputs,
                    size_t max_num_inputs, const uint64_t* z_host, spg_pqx** out) {
  spg_pqx* h = nullptr;
  if (int rc = pqx_alloc(ctx, what, have_z, num_instances, num_proofs, max_num_proofs, num_witness_secs, num_inputs,
                         max_num_inputs, &h))
    return rc;
  const spg::PqxDev& T = h->T;
  int rc = 0;
  auto fail = [&](int code, const char* msg) {
    if (!rc) rc = spg::set_err(ctx, code, std::string(what) + ": " + msg);
  };
  std::vector<spg::RevDesc> rd(num_instances);
  for (size_t p = 0; p < num_instances; p++) {
    size_t lq = 0, li = 0;
    while (((size_t)1 << lq) < num_proofs[p]) lq++;
    while (((size_t)1 << li) < num_inputs[p]) li++;
    rd[p] = spg::RevDesc{(uint32_t)T.off[p], (uint32_t)lq, (uint32_t)li, (uint32_t)num_witness_secs};
  }
  spg::RevDesc* d_rd = (spg::RevDesc*)spg::ws_get(ctx, spg::Ws::SeamRevDesc, rd.size() * sizeof(spg::RevDesc) + 64);
  if (!d_rd) fail(SPG_E_NOMEM, "descriptors");
  if (!rc && z_host) {  // the host form: one upload in the caller's order, reordered on the device
    Fq* up = (Fq*)spg::ws_get(ctx, spg::Ws::SeamRev, T.total * sizeof(Fq) + 64);
    if (!up) fail(SPG_E_NOMEM, "upload buffer");
    else if (hipMemcpyAsync(up, z_host, T.total * sizeof(Fq), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
      fail(SPG_E_HIP, "upload");
    z = up;
  }
  if (!rc && hipMemcpyAsync(d_rd, rd.data(), rd.size() * sizeof(spg::RevDesc), hipMemcpyHostToDevice, ctx->stream) !=
                 hipSuccess)
    fail(SPG_E_HIP, "descriptor upload");
  if (!rc) {
    spg::timer_start(ctx);
    hipLaunchKernelGGL(spg::k_pqx_new_rev, dim3((unsigned)((T.total + 255) / 256)), dim3(256), 0, ctx->stream, d_rd,
                       (int)num_instances, z, T.d, (uint32_t)T.total);
    spg::timer_stop(ctx);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) fail(SPG_E_HIP, "launch");
    float ms = 0.f;
    if (!rc && hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) ctx->last_us = ms * 1000.0;
  }
  if (rc) {
    hipStreamSynchronize(ctx->stream);  // (rd and the upload must not be read after this returns)
    hipFree(h->T.d);
    delete h;
    return rc;
  }
  *out = h;
  return SPG_OK;
}
}  // namespace

extern "C" int spg_pqx_new(spg_ctx* ctx, const uint64_t* z_mont, size_t num_instances, const size_t* num_proofs,
                           size_t max_num_proofs, size_t num_witness_secs, const size_t* num_inputs,
                           size_t max_num_inputs, spg_pqx** out) {
  if (!ctx || !out || !num_proofs || !num_inputs || num_instances == 0 || num_witness_secs == 0) return SPG_E_ARG;
  spg_pqx* h = nullptr;
  if (int rc = pqx_alloc(ctx, "spg_pqx_new", z_mont != nullptr, num_instances, num_proofs, max_num_proofs,
                         num_witness_secs, num_inputs, max_num_inputs, &h))
    return rc;
  if (hipMemcpy(h->T.d, z_mont, h->T.total * sizeof(Fq), hipMemcpyHostToDevice) != hipSuccess) {
    hipFree(h->T.d);
    delete h;
    return spg::set_err(ctx, SPG_E_HIP, "spg_pqx_new: upload");
  }
  *out = h;
  return SPG_OK;
}

extern "C" int spg_pqx_new_rev(spg_ctx* ctx, const uint64_t* z_mont, size_t num_instances, const size_t* num_proofs,
                               size_t max_num_proofs, size_t num_witness_secs, const size_t* num_inputs,
                               size_t max_num_inputs, spg_pqx** out) {
  if (!ctx || !out || !num_proofs || !num_inputs || num_instances == 0 || num_witness_secs == 0) return SPG_E_ARG;
  return pqx_new_rev_dev(ctx, "spg_pqx_new_rev", nullptr, z_mont != nullptr, num_instances, num_proofs, max_num_proofs,
                         num_witness_secs, num_inputs, max_num_inputs, z_mont, out);
}

extern "C" int spg_pqx_new_rev_buf(spg_ctx* ctx, const spg_buf* z, size_t offset, size_t num_instances,
                                   const size_t* num_proofs, size_t max_num_proofs, size_t num_witness_secs,
                                   const size_t* num_inputs, size_t max_num_inputs, spg_pqx** out) {
  if (!ctx || !out || !num_proofs || !num_inputs || num_instances == 0 || num_witness_secs == 0) return SPG_E_ARG;
  if (z) {  // the shape's total must lie inside the buffer
    const size_t lim = (size_t)1 << 31;  // (pqx_alloc refuses a larger table; the products below cannot wrap)
    size_t total = 0;
    for (size_t p = 0; p < num_instances && total < lim; p++) {
      const size_t rows = num_proofs[p] < lim && num_witness_secs < lim ? num_proofs[p] * num_witness_secs : lim;
      total += rows < lim && num_inputs[p] < lim ? rows * num_inputs[p] : lim;
    }
    if (total < lim && (offset > z->n || total > z->n - offset))
      return spg::set_err(ctx, SPG_E_ARG, "spg_pqx_new_rev_buf: offset + the shape's total exceeds the buffer");
  }
  return pqx_new_rev_dev(ctx, "spg_pqx_new_rev_buf", z ? z->d + offset : nullptr, z != nullptr, num_instances,
                         num_proofs, max_num_proofs, num_witness_secs, num_inputs, max_num_inputs, nullptr, out);
}

extern "C" int spg_pqx_free(spg_ctx* ctx, spg_pqx* h) {
  (void)ctx;
  if (!h) return SPG_OK;
  hipFree(h->T.d);
  delete h;
  return SPG_OK;
}

// the current sizes: dims = (num_instances, max_num_proofs, num_witness_secs, max_num_inputs); num_proofs /
// num_inputs (optional) receive Z.len() entries each
extern "C" int spg_pqx_shape(const spg_pqx* h, size_t* dims, size_t* num_proofs, size_t* num_inputs) {
  if (!h || !dims) return SPG_E_ARG;
  const spg::PqxDev& T = h->T;
  dims[0] = T.num_instances;
  dims[1] = T.max_num_proofs;
  dims[2] = T.num_witness_secs;
  dims[3] = T.max_num_inputs;
  for (size_t p = 0; p < T.zlen; p++) {
    if (num_proofs) num_proofs[p] = T.num_proofs[p];
    if (num_inputs) num_inputs[p] = T.num_inputs[p];
  }
  return SPG_OK;
}

// Z in spg_pqx_new's layout (every allocated entry, folded or not)
extern "C" int spg_pqx_download(spg_ctx* ctx, const spg_pqx* h, uint64_t* z_mont) {
  if (!ctx || !h || !z_mont) return SPG_E_ARG;
  SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  SPG_HIP(ctx, hipMemcpy(z_mont, h->T.d, h->T.total * sizeof(Fq), hipMemcpyDeviceToHost));
  return SPG_OK;
}

// DensePolynomialPqx::bound_poly (custom_dense_mlpoly.rs:180-199): mode 1 p, 2 q, 3 w, 4 x
extern "C" int spg_pqx_bound(spg_ctx* ctx, spg_pqx* h, const uint64_t* r_mont, int mode) {
  if (!ctx || !h || !r_mont) return SPG_E_ARG;
  int rc = pqx_bind_one(ctx, h->T, spg::ld_fq(r_mont), mode);
  if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = spg::set_err(ctx, SPG_E_HIP, "spg_pqx_bound");
  return rc;
}

// DensePolynomialPqx::bound_poly_vars_rq (custom_dense_mlpoly.rs:300-304): n q binds in order, in one pass against
// eq(rq) when n >= 2. When they bind every q variable an instance still has (every instance's rows <= 2^n) that pass
// is the prover's own before phase 2 (k_pqx_bound_q, row groups per output); a shorter prefix leaves rows behind and
// takes k_pqx_bound_q_prefix, one lane per remaining entry. One challenge is one fold.
extern "C" int spg_pqx_bound_rq(spg_ctx* ctx, spg_pqx* h, const uint64_t* rq_mont, size_t n) {
  if (!ctx || !h || (!rq_mont && n)) return SPG_E_ARG;
  spg::PqxDev& T = h->T;
  size_t left = 0;
  while (((size_t)1 << left) < T.max_num_proofs) left++;
  if (n > left) return spg::set_err(ctx, SPG_E_ARG, "spg_pqx_bound_rq: more challenges than q variables left");
  if (n == 0) return SPG_OK;
  bool all = n >= 2;
  for (size_t p = 0; p < std::min(T.num_instances, T.zlen); p++) all = all && T.num_proofs[p] <= ((size_t)1 << n);
  int rc = 0;
  spg::timer_start(ctx);
  if (n >= 2) {
    Fq* E = (Fq*)spg::ws_get(ctx, spg::Ws::SeamEq, (sizeof(Fq) << n) + 64);
    if (!E) return spg::set_err(ctx, SPG_E_NOMEM, "spg_pqx_bound_rq");
    std::vector<Fq> r(n);
    for (size_t k = 0; k < n; k++) r[k] = spg::ld_fq(rq_mont + 4 * k);
    rc = spg::dev_eq_table(ctx, r.data(), (int)n, E);
    if (!rc) rc = all ? spg::pqx_bound_q_all(ctx, T, E, n) : spg::pqx_bound_q_prefix(ctx, T, E, n);
  } else {
    rc = pqx_bind_one(ctx, T, spg::ld_fq(rq_mont), spg::MODE_Q);
  }
  spg::timer_stop(ctx);
  if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = spg::set_err(ctx, SPG_E_HIP, "spg_pqx_bound_rq");
  float ms = 0.f;
  if (!rc && hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) ctx->last_us = ms * 1000.0;
  return rc;
}

// DensePolynomialPqx::evaluate (custom_dense_mlpoly.rs:320-333): a clone bound by r_x, r_w, r_q, r_p in that order,
// then index(0, 0, 0, 0); h is left unchanged
extern "C" int spg_pqx_evaluate(spg_ctx* ctx, const spg_pqx* h, const uint64_t* rp, size_t np, const uint64_t* rq,
                                size_t nq, const uint64_t* rw, size_t nw, const uint64_t* rx, size_t nx,
                                uint64_t* out_mont) {
  if (!ctx || !h || !out_mont || (np && !rp) || (nq && !rq) || (nw && !rw) || (nx && !rx)) return SPG_E_ARG;
  spg::PqxDev C = h->T;  // the clone: same descriptors and sizes, its own copy of the entries
  C.d = (Fq*)spg::ws_get(ctx, spg::Ws::SeamTmp, C.total * sizeof(Fq) + 64);
  if (!C.d) return spg::set_err(ctx, SPG_E_NOMEM, "spg_pqx_evaluate");
  SPG_HIP(ctx, hipMemcpyAsync(C.d, h->T.d, C.total * sizeof(Fq), hipMemcpyDeviceToDevice, ctx->stream));
  const struct {
    const uint64_t* r;
    size_t n;
    int mode;
  } secs[4] = {{rx, nx, spg::MODE_X}, {rw, nw, spg::MODE_W}, {rq, nq, spg::MODE_Q}, {rp, np, spg::MODE_P}};
  for (const auto& s : secs)
    for (size_t i = 0; i < s.n; i++)
      if (int rc = pqx_bind_one(ctx, C, spg::ld_fq(s.r + 4 * i), s.mode)) return rc;
  // index(0, 0, 0, 0): Z[0][0][0][0] when that entry is allocated (custom_dense_mlpoly.rs:118-128)
  Fq v = spg::fq_zero();
  if (C.zlen && C.anp[0] && C.anw[0] && C.ani[0])
    if (int rc = spg::d2h(ctx, &v, C.d, sizeof(Fq))) return rc;
  spg::st_fq(out_mont, v);
  return SPG_OK;
}

// One round of SumcheckInstanceProof::prove_cubic_with_additive_term_disjoint_rounds (src/sumcheck.rs:1067-1380,
// round loop :1173-1245; comb A (B C - D), src/r1csproof.rs) in an x, q or p round: (e0, e2, e3) over the eq factors
// Ap, Aq, Ax (dense, their current lengths: the round's instance_len = |Ap| (/ 2 in a p round), proof_len = |Aq| (/ 2 in a q round),
// cons_len = |Ax| (/ 2 in an x round)) and B, C, D (Pqx tables of one shape, one witness section) in their current
// state -- the reference's local num_proofs / num_cons are the tables' own sizes, halved at the round start as there.
// The prover's phase-1 evaluation kernels do the work.
extern "C" int spg_phase1_round_evals(spg_ctx* ctx, const spg_buf* Ap, const spg_buf* Aq, const spg_buf* Ax,
                                      const spg_pqx* B, const spg_pqx* C, const spg_pqx* D, int mode,
                                      uint64_t* out3_mont) {
  if (!ctx || !Ap || !Aq || !Ax || !B || !C || !D || !out3_mont) return SPG_E_ARG;
  const spg::PqxDev& T = B->T;
  for (const spg_pqx* o : {C, D})
    if (o->T.zlen != T.zlen || o->T.anp != T.anp || o->T.anw != T.anw || o->T.ani != T.ani ||
        o->T.num_proofs != T.num_proofs || o->T.num_inputs != T.num_inputs)
      return spg::set_err(ctx, SPG_E_ARG, "phase-1 round: B, C, D must share one shape");
  if (T.num_witness_secs != 1)  // sumcheck.rs:1099-1102 assert_eq!(poly_B.num_witness_secs, 1)
    return spg::set_err(ctx, SPG_E_ARG, "phase-1 round: one witness section");
  if (mode != spg::MODE_X && mode != spg::MODE_Q && mode != spg::MODE_P)
    return spg::set_err(ctx, SPG_E_ARG, "phase-1 round: mode 4 (x), 2 (q) or 1 (p)");
  // (a p round halves |Ap| below the instance count: the loop then runs over p < min(instance_len, instances))
  if (!spg::pow2(Ap->n) || !spg::pow2(Aq->n) || !spg::pow2(Ax->n) || (mode != spg::MODE_P && Ap->n < T.zlen))
    return spg::set_err(ctx, SPG_E_ARG, "phase-1 round: eq tables of power-of-two lengths, |Ap| >= instances");
  if (mode == spg::MODE_P) {
    if (Ax->n != 1 || Aq->n != 1 || Ap->n < 2)
      return spg::set_err(ctx, SPG_E_ARG, "phase-1 round: p rounds once |Ax| = |Aq| = 1, with |Ap| >= 2");
  } else if (mode == spg::MODE_X ? Ax->n < 2 : (Ax->n != 1 || Aq->n < 2)) {
    return spg::set_err(ctx, SPG_E_ARG, "phase-1 round: x rounds first (|Ax| >= 2), q rounds once |Ax| = 1");
  }
  const size_t instance_len = mode == spg::MODE_P ? Ap->n / 2 : Ap->n,
               proof_len = mode == spg::MODE_Q ? Aq->n / 2 : Aq->n, cons_len = mode == spg::MODE_X ? Ax->n / 2 : 1;
  std::vector<size_t> sc_np = T.num_proofs, sc_nc = T.num_inputs;
  for (size_t p = 0; p < T.zlen; p++) {
    if (mode == spg::MODE_X && sc_nc[p] > 1) sc_nc[p] /= 2;
    if (mode == spg::MODE_Q && sc_np[p] > 1) sc_np[p] /= 2;
    if (proof_len % sc_np[p] || cons_len % sc_nc[p])
      return spg::set_err(ctx, SPG_E_ARG, "phase-1 round: table sizes exceed the eq tables");
  }
  Fq* partials = (Fq*)spg::ws_get(ctx, spg::Ws::SeamPart,
                                  std::max(3 * (size_t)spg::kScGridMax, spg::kP1PairMax) * sizeof(Fq) + 64);
  if (!partials) return spg::set_err(ctx, SPG_E_NOMEM, "phase-1 round partials");
  Fq e[3];
  const int rc = spg::phase1_eval(ctx, T, mode, proof_len, cons_len, instance_len, sc_np, sc_nc, Ap->d, Aq->d, Ax->d,
                                  T.d, C->T.d, D->T.d, partials, e);
  if (rc) return rc;
  for (int k = 0; k < 3; k++) spg::st_fq(out3_mont + 4 * k, e[k]);
  return SPG_OK;
}

// One round of the R1CS proof's phase-2 sumcheck (SumcheckInstanceProof::prove_cubic_disjoint_rounds,
// src/sumcheck.rs:788-1065, round loop :881-941; comb A B C): (e0, e2, e3) over eq(r_p) (A, current length:
// instance_len = |A|, / 2 in a p round), ABC (one instance when single_inst, else one per instance) and Z in their
// current state, in a y (mode 4), w (mode 3) or p (mode 1) round; num_witness_secs: the reference's argument (the
// sections that exist); witness_secs_len and the local num_inputs are Z's own sizes, halved at the round start.
extern "C" int spg_phase2_round_evals(spg_ctx* ctx, const spg_buf* A, const spg_pqx* ABC, const spg_pqx* Z, int mode,
                                      int single_inst, size_t num_witness_secs, uint64_t* out3_mont) {
  if (!ctx || !A || !ABC || !Z || !out3_mont || num_witness_secs == 0) return SPG_E_ARG;
  const spg::PqxDev &TA = ABC->T, &TZ = Z->T;
  if (mode != spg::MODE_X && mode != spg::MODE_W && mode != spg::MODE_P)
    return spg::set_err(ctx, SPG_E_ARG, "phase-2 round: mode 4 (y), 3 (w) or 1 (p)");
  if (single_inst ? TA.zlen != 1 : TA.zlen != TZ.zlen)
    return spg::set_err(ctx, SPG_E_ARG, "phase-2 round: ABC holds one instance (single_inst) or one per instance");
  if (!spg::pow2(A->n) || (mode == spg::MODE_P && A->n < 2))  // (the loop runs p < min(instance_len, instances))
    return spg::set_err(ctx, SPG_E_ARG, "phase-2 round: eq(r_p) of power-of-two length (>= 2 in a p round)");
  if ((mode == spg::MODE_X && TZ.max_num_inputs < 2) ||
      (mode == spg::MODE_W && (TZ.max_num_inputs != 1 || TZ.num_witness_secs < 2)) ||
      (mode == spg::MODE_P && (TZ.max_num_inputs != 1 || TZ.num_witness_secs != 1)))
    return spg::set_err(ctx, SPG_E_ARG, "phase-2 round: y rounds, then w rounds, then p rounds");
  // (one live proof row: allocated so, or every q variable bound -- spg_pqx_bound_rq -- as the prover's own Z is)
  for (const spg::PqxDev* T : {&TA, &TZ})
    for (size_t p = 0; p < T->zlen; p++)
      if (T->num_proofs[p] != 1 || T->max_num_proofs != 1)
        return spg::set_err(ctx, SPG_E_ARG, "phase-2 round: tables of one proof row (q bound)");
  const size_t instance_len = mode == spg::MODE_P ? A->n / 2 : A->n;
  const size_t ws_len = mode == spg::MODE_W ? TZ.num_witness_secs / 2 : TZ.num_witness_secs;
  std::vector<size_t> sc_ni = TZ.num_inputs;
  for (size_t p = 0; p < sc_ni.size(); p++)
    if (mode == spg::MODE_X && sc_ni[p] > 1) sc_ni[p] /= 2;
  Fq* partials = (Fq*)spg::ws_get(ctx, spg::Ws::SeamPart,
                                  std::max(3 * (size_t)spg::kScGridMax, spg::kP1PairMax) * sizeof(Fq) + 64);
  if (!partials) return spg::set_err(ctx, SPG_E_NOMEM, "phase-2 round partials");
  Fq e[3];
  const int rc = spg::phase2_eval(ctx, TA, TZ, mode, instance_len, ws_len, num_witness_secs, single_inst != 0, sc_ni,
                                  A->d, partials, e);
  if (rc) return rc;
  for (int k = 0; k < 3; k++) spg::st_fq(out3_mont + 4 * k, e[k]);
  return SPG_OK;
}

// ---- the two ZK sumchecks of R1CSProof::prove on caller tables: the round seams above for (e0, e2, e3), ZKRounds
// (zk_rounds.hpp, the prover's own) for the per-round sigma protocol and the tape order, the fold seams between rounds.
// One launch per evaluation and per fold; the proof is the reference's bincode of ZKSumcheckInstanceProof.
namespace {
// bincode(ZKSumcheckInstanceProof) of `rounds` cubic rounds: three Vec lengths, then per round comm_poly, comm_eval
// and a DotProductProof over 4 coefficients (delta, beta, Vec z of 4, z_delta, z_beta)
size_t zk_proof_len(size_t rounds) { return 24 + rounds * (64 + 64 + 8 + 4 * 32 + 64); }

bool same_shape(const spg::PqxDev& a, const spg::PqxDev& b) {
  return a.zlen == b.zlen && a.anp == b.anp && a.anw == b.anw && a.ani == b.ani && a.num_proofs == b.num_proofs &&
         a.num_inputs == b.num_inputs && a.num_instances == b.num_instances && a.max_num_proofs == b.max_num_proofs &&
         a.num_witness_secs == b.num_witness_secs && a.max_num_inputs == b.max_num_inputs;
}
bool unbound(const spg::PqxDev& T) { return T.num_proofs == T.anp && T.num_inputs == T.ani; }

struct ZkOut {
  uint8_t* proof;
  size_t cap;
  uint64_t *r, *claims, *blind_post;
};
// the proof bytes, challenges, final claims (read from the device: `fin`, one scalar each) and the last blind
int zk_finish(spg_ctx* ctx, spg::ZKRounds& zk, const spg::FqV& r, const std::vector<const Fq*>& fin, size_t n_eq,
              const ZkOut& o) {
  std::vector<Fq> v(fin.size());
  for (size_t k = 0; k < fin.size(); k++)
    SPG_HIP(ctx, hipMemcpyAsync(&v[k], fin[k], sizeof(Fq), hipMemcpyDeviceToHost, ctx->stream));
  SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  Fq a = v[0];  // the eq factors' product, then the tables
  for (size_t k = 1; k < n_eq; k++) a = spg::fq_mul(a, v[k]);
  spg::st_fq(o.claims, a);
  for (size_t k = n_eq; k < v.size(); k++) spg::st_fq(o.claims + 4 * (1 + k - n_eq), v[k]);
  for (size_t j = 0; j < r.size(); j++) spg::st_fq(o.r + 4 * j, r[j]);
  spg::st_fq(o.blind_post, zk.blinds_evals.back());
  spg::Writer w;
  zk.out.ser(w);
  if (w.out.size() != zk_proof_len(r.size()) || w.out.size() > o.cap)
    return spg::set_err(ctx, SPG_E_HIP, "ZK sumcheck proof size");
  memcpy(o.proof, w.out.data(), w.out.size());
  return SPG_OK;
}
}  // namespace

extern "C" int spg_zk_phase1_prove(spg_ctx* ctx, const spg_r1cs_gens* gens, const uint64_t* claim,
                                   const uint64_t* blind_claim, size_t nx, size_t nq, size_t np, spg_buf* Ap,
                                   spg_buf* Aq, spg_buf* Ax, spg_pqx* B, spg_pqx* C, spg_pqx* D, spg_transcript* t,
                                   spg_random_tape* tape, uint8_t* proof, size_t cap, size_t* len, uint64_t* r_mont,
                                   uint64_t* claims4_mont, uint64_t* blind_post_mont) {
  if (!ctx || !gens || !Ap || !Aq || !Ax || !B || !C || !D || !t || !tape || !len || !r_mont || !claims4_mont ||
      !blind_post_mont)
    return SPG_E_ARG;
  const size_t rounds = nx + nq + np;
  if (rounds == 0 || nx > 30 || nq > 30 || np > 30)  // (no round: the reference indexes blinds_evals[-1])
    return spg::set_err(ctx, SPG_E_ARG, "spg_zk_phase1_prove: 1 or more rounds, at most 30 variables each");
  const spg::PqxDev& T = B->T;
  if (!same_shape(T, C->T) || !same_shape(T, D->T) || T.num_witness_secs != 1 || !unbound(T))
    return spg::set_err(ctx, SPG_E_ARG, "spg_zk_phase1_prove: B, C, D of one shape, one witness section, unbound");
  if (Ax->n != ((size_t)1 << nx) || Aq->n != ((size_t)1 << nq) || Ap->n != ((size_t)1 << np) || Ap->n < T.zlen ||
      T.max_num_inputs != Ax->n || T.max_num_proofs != Aq->n)
    return spg::set_err(ctx, SPG_E_ARG, "spg_zk_phase1_prove: |Ax| = 2^nx = max_num_inputs, |Aq| = 2^nq = "
                                        "max_num_proofs, |Ap| = 2^np >= instances");
  if (gens->g.gens_4.G.size() != 4 || gens->g.gens_1.G.empty())
    return spg::set_err(ctx, SPG_E_ARG, "spg_zk_phase1_prove: generators without gens_1 / gens_4");
  *len = zk_proof_len(rounds);
  if (!proof || cap < *len) return spg::set_err(ctx, SPG_E_ARG, "spg_zk_phase1_prove: proof buffer too small");
  spg::HostPin pin;
  spg::ProverGens& g = const_cast<spg_r1cs_gens*>(gens)->g;
  spg::ZKRounds zk;
  zk.init(g, tape->t, rounds, claim ? spg::ld_fq(claim) : spg::fq_zero(),
          blind_claim ? spg::ld_fq(blind_claim) : spg::fq_zero());
  spg::FqV r;
  spg::timer_start(ctx);
  for (size_t j = 0; j < rounds; j++) {
    const int mode = j < nx ? spg::MODE_X : (j < nx + nq ? spg::MODE_Q : spg::MODE_P);
    uint64_t e_m[12];
    if (int rc = spg_phase1_round_evals(ctx, Ap, Aq, Ax, B, C, D, mode, e_m)) return spg::tr_status(ctx, t->t, rc);
    const Fq e[3] = {spg::ld_fq(e_m), spg::ld_fq(e_m + 4), spg::ld_fq(e_m + 8)};
    const Fq r_j = zk.begin(g, t->t, j, e);
    // the round's eq factor (bound_poly_var_top) and B, C, D in one launch
    spg_buf* side = mode == spg::MODE_X ? Ax : (mode == spg::MODE_Q ? Aq : Ap);
    if (int rc = spg::pqx_bound(ctx, B->T, C->T.d, D->T.d, r_j, mode, side->d, side->n))
      return spg::tr_status(ctx, t->t, rc);
    side->n /= 2;
    for (spg_pqx* o : {C, D}) {  // the same size bookkeeping as B's
      o->T.num_instances = B->T.num_instances;
      o->T.max_num_proofs = B->T.max_num_proofs;
      o->T.max_num_inputs = B->T.max_num_inputs;
      o->T.num_proofs = B->T.num_proofs;
      o->T.num_inputs = B->T.num_inputs;
    }
    zk.finish(g, t->t, tape->t, j, r_j);
    r.push_back(r_j);
  }
  spg::timer_stop(ctx);
  const int rc = zk_finish(ctx, zk, r, {Ap->d, Aq->d, Ax->d, B->T.d, C->T.d, D->T.d}, 3,
                           ZkOut{proof, cap, r_mont, claims4_mont, blind_post_mont});
  float ms = 0.f;
  if (!rc && hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) ctx->last_us = ms * 1000.0;
  return spg::tr_status(ctx, t->t, rc);
}

extern "C" int spg_zk_phase2_prove(spg_ctx* ctx, const spg_r1cs_gens* gens, const uint64_t* claim,
                                   const uint64_t* blind_claim, size_t ny, size_t nw, size_t np, int single_inst,
                                   size_t num_witness_secs, spg_buf* eq, spg_pqx* ABC, spg_pqx* Z, spg_transcript* t,
                                   spg_random_tape* tape, uint8_t* proof, size_t cap, size_t* len, uint64_t* r_mont,
                                   uint64_t* claims3_mont, uint64_t* blind_post_mont) {
  if (!ctx || !gens || !eq || !ABC || !Z || !t || !tape || !len || !r_mont || !claims3_mont || !blind_post_mont ||
      num_witness_secs == 0)
    return SPG_E_ARG;
  const size_t rounds = ny + nw + np;
  if (rounds == 0 || ny > 30 || nw > 30 || np > 30)
    return spg::set_err(ctx, SPG_E_ARG, "spg_zk_phase2_prove: 1 or more rounds, at most 30 variables each");
  spg::PqxDev &TA = ABC->T, &TZ = Z->T;
  if (single_inst ? TA.zlen != 1 : TA.zlen != TZ.zlen)
    return spg::set_err(ctx, SPG_E_ARG, "spg_zk_phase2_prove: ABC holds one instance (single_inst) or one per instance");
  if (eq->n != ((size_t)1 << np) || eq->n < TZ.zlen)
    return spg::set_err(ctx, SPG_E_ARG, "spg_zk_phase2_prove: |eq| = 2^np >= instances");
  for (const spg::PqxDev* T : {&TA, &TZ}) {
    bool ok = T->max_num_proofs == 1 && T->max_num_inputs == ((size_t)1 << ny) &&
              T->num_witness_secs == ((size_t)1 << nw) && T->num_inputs == T->ani;
    for (size_t p = 0; p < T->zlen && ok; p++) ok = T->num_proofs[p] == 1;
    if (!ok)
      return spg::set_err(ctx, SPG_E_ARG, "spg_zk_phase2_prove: ABC and Z with q bound, y and w unbound: "
                                          "max_num_inputs = 2^ny, num_witness_secs = 2^nw");
  }
  for (size_t p = 0; p < TZ.zlen; p++)  // (the round kernels read ABC at Z's current widths)
    if (TA.ani[single_inst ? 0 : p] < TZ.ani[p])
      return spg::set_err(ctx, SPG_E_ARG, "spg_zk_phase2_prove: ABC narrower than Z");
  if (gens->g.gens_4.G.size() != 4 || gens->g.gens_1.G.empty())
    return spg::set_err(ctx, SPG_E_ARG, "spg_zk_phase2_prove: generators without gens_1 / gens_4");
  *len = zk_proof_len(rounds);
  if (!proof || cap < *len) return spg::set_err(ctx, SPG_E_ARG, "spg_zk_phase2_prove: proof buffer too small");
  spg::HostPin pin;
  spg::ProverGens& g = const_cast<spg_r1cs_gens*>(gens)->g;
  spg::ZKRounds zk;
  zk.init(g, tape->t, rounds, claim ? spg::ld_fq(claim) : spg::fq_zero(),
          blind_claim ? spg::ld_fq(blind_claim) : spg::fq_zero());
  spg::FqV r;
  spg::timer_start(ctx);
  for (size_t j = 0; j < rounds; j++) {
    const int mode = j < ny ? spg::MODE_X : (j < ny + nw ? spg::MODE_W : spg::MODE_P);
    uint64_t e_m[12];
    if (int rc = spg_phase2_round_evals(ctx, eq, ABC, Z, mode, single_inst, num_witness_secs, e_m))
      return spg::tr_status(ctx, t->t, rc);
    const Fq e[3] = {spg::ld_fq(e_m), spg::ld_fq(e_m + 4), spg::ld_fq(e_m + 8)};
    const Fq r_j = zk.begin(g, t->t, j, e);
    int rc = 0;
    if (mode == spg::MODE_P) {  // sumcheck.rs:961-967: eq always, ABC unless it is the one shared instance
      rc = spg::dev_fold_top(ctx, eq->d, eq->n, r_j);
      eq->n /= 2;
    }
    if (!rc) rc = mode != spg::MODE_P || !single_inst ? spg::pqx_bound2(ctx, TA, TZ, r_j, mode)
                                                      : spg::pqx_bound(ctx, TZ, nullptr, nullptr, r_j, mode);
    if (rc) return spg::tr_status(ctx, t->t, rc);
    zk.finish(g, t->t, tape->t, j, r_j);
    r.push_back(r_j);
  }
  spg::timer_stop(ctx);
  const int rc = zk_finish(ctx, zk, r, {eq->d, TA.d, TZ.d}, 1, ZkOut{proof, cap, r_mont, claims3_mont, blind_post_mont});
  float ms = 0.f;
  if (!rc && hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) ctx->last_us = ms * 1000.0;
  return spg::tr_status(ctx, t->t, rc);
}
