// spg — many short group equations in one launch (spg_eqs_check): E independent sums sum_i s_i P_i over proof points,
// a few generators and points the caller already holds, each tested against the ristretto255 identity. This is the
// shape of a verifier's sigma-protocol checks (KnowledgeProof, EqualityProof, ProductProof, DotProductProof, the tail
// of DotProductProofLog: src/nizk/mod.rs:50-570): a few hundred equations of 2-25 terms whose scalars all come from
// the transcript. msm_var.hip's sort / bucket pipeline does not pay off at five points, and the host does them one
// 256-step double-and-add after another.
//   k_eqs_term   one lane per term: the operand (RFC 9496 DECODE of a 32-byte encoding, a 128-byte extended point, or
//                an affine Niels point of the caller's spg_points), the scalar out of Montgomery form, then a plain
//                binary double-and-add with a fixed trip count of 253 (every scalar is < q < 2^253) and a select per
//                bit, so a wavefront never diverges on scalar bits. The product goes to HBM as an extended point;
//                a rejected encoding marks its term and posts its index by atomicMin.
//   k_eqs_sum    one wavefront per equation: lane l adds terms l, l + 64, ..; a shuffle tree over the 64 lane sums (only
//                the levels the equation's length needs); lane 0 tests X = 0 or Y = 0 (RFC 9496 4.3.3 against (0, 1))
//                and, when asked, encodes the sum.
// Equation boundaries never meet the term kernel's lanes, so a length that straddles a wavefront or a workgroup is no
// special case; a long equation costs its length / 64 serial additions in the sum kernel (every length stays in these
// two kernels, nothing is routed to the msm_var pipeline). Inputs go up in one copy from page-locked staging, results
// come back in one plain copy. Single-rank.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include "ctx.hpp"
#include "eqcheck.hpp"

namespace spg {

namespace {

struct EqsArgs {
  const uint8_t* kinds;
  const uint32_t* refs;
  const Fq* scalars;
  const uint32_t* comp;  // nc x 8 words
  const Ext* ext;        // ne
  const Niels* base;     // nb
  uint32_t T, nc, ne, nb;
  Ext* prod;      // T products s_i P_i
  uint8_t* tbad;  // T: 1 where the term's encoding was rejected
  int* bad;       // the lowest such term (INT_MAX: none)
};

// P's cached form for repeated additions: (Y - X, Y + X, 2 Z, 2 d T)
struct PNiels {
  Fp ymx, ypx, z2, t2d;
};
__device__ __forceinline__ Ext ext_add_pn(const Ext& p, const PNiels& q) {  // add-2008-hwcd-3, 8M
  const Fp A = fp_mul(fp_sub(p.Y, p.X), q.ymx);
  const Fp B = fp_mul(fp_add(p.Y, p.X), q.ypx);
  const Fp C = fp_mul(p.T, q.t2d);
  const Fp D = fp_mul(p.Z, q.z2);
  const Fp E = fp_sub(B, A), F = fp_sub(D, C), G = fp_add(D, C), H = fp_add(B, A);
  Ext r;
  r.X = fp_mul(E, F); r.Y = fp_mul(G, H); r.T = fp_mul(E, H); r.Z = fp_mul(F, G);
  return r;
}
__device__ __forceinline__ Fp fp_sel(const Fp& a, const Fp& b, bool on) {  // on ? a : b, limb by limb (no struct select)
  Fp r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.l[i] = on ? a.l[i] : b.l[i];
  return r;
}

__global__ void __launch_bounds__(kEqsTermBS, 2) k_eqs_term(EqsArgs a) {
  const uint32_t i = blockIdx.x * kEqsTermBS + threadIdx.x;
  if (i >= a.T) return;
  const uint32_t kind = a.kinds[i], ref = a.refs[i];
#ifdef SPG_CHECKED
  if (kind > kEqsIndex || ref >= (kind == kEqsCompressed ? a.nc : kind == kEqsExtended ? a.ne : a.nb)) {
    printf("k_eqs_term: term %u form %u operand %u past its pool (%u / %u / %u)\n", i, kind, ref, a.nc, a.ne, a.nb);
    a.prod[i] = ext_identity();
    a.tbad[i] = 1;
    atomicMin(a.bad, (int)i);
    return;
  }
#endif
  Ext P;
  bool ok = true;
  if (kind == kEqsCompressed) {
    uint8_t c[32];
#pragma unroll
    for (int w = 0; w < 8; w++) {
      const uint32_t v = a.comp[8 * (size_t)ref + w];
      c[4 * w] = (uint8_t)v;
      c[4 * w + 1] = (uint8_t)(v >> 8);
      c[4 * w + 2] = (uint8_t)(v >> 16);
      c[4 * w + 3] = (uint8_t)(v >> 24);
    }
    ok = ext_decompress(c, P);
    if (!ok) P = ext_identity();
  } else if (kind == kEqsExtended) {
    P = a.ext[ref];
  } else {
    P = niels_to_ext(a.base[ref]);
  }
  PNiels Q;
  Q.ymx = fp_sub(P.Y, P.X);
  Q.ypx = fp_add(P.Y, P.X);
  Q.z2 = fp_add(P.Z, P.Z);
  Q.t2d = fp_mul(P.T, c_d2());
  // Scalar::to_bytes (src/scalar/mod.rs:32-36); k < q < 2^253: bit 252 moves to the top, then one bit per step leaves
  // there (constant limb indices: a runtime-indexed limb would put k in a private segment)
  Fq k = fq_from_mont(a.scalars[i]);
#pragma unroll
  for (int w = 7; w >= 1; w--) k.l[w] = (k.l[w] << 3) | (k.l[w - 1] >> 29);
  k.l[0] <<= 3;
  Ext acc = ext_identity();
  for (int b = 0; b < 253; b++) {
    const bool on = (k.l[7] >> 31) != 0;
#pragma unroll
    for (int w = 7; w >= 1; w--) k.l[w] = (k.l[w] << 1) | (k.l[w - 1] >> 31);
    k.l[0] <<= 1;
    acc = ext_dbl(acc);
    const Ext s = ext_add_pn(acc, Q);
    acc.X = fp_sel(s.X, acc.X, on);
    acc.Y = fp_sel(s.Y, acc.Y, on);
    acc.Z = fp_sel(s.Z, acc.Z, on);
    acc.T = fp_sel(s.T, acc.T, on);
  }
  a.prod[i] = acc;
  a.tbad[i] = ok ? 0 : 1;
  if (!ok) atomicMin(a.bad, (int)i);
}

__device__ __forceinline__ Fp fp_shfl_down(const Fp& a, int d) {
  Fp r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.l[i] = __shfl_down(a.l[i], d, 64);
  return r;
}

__global__ void __launch_bounds__(kEqsSumBS) k_eqs_sum(const Ext* __restrict__ prod, const uint8_t* __restrict__ tbad,
                                                       const uint32_t* __restrict__ first, uint32_t E, uint32_t T,
                                                       uint8_t* __restrict__ sums, uint8_t* __restrict__ status) {
  const uint32_t e = blockIdx.x * kEqsSumPerWG + (threadIdx.x >> 6);  // uniform per wavefront
  const int lane = threadIdx.x & 63;
  if (e >= E) return;
  uint32_t t0 = first[e], t1 = first[e + 1];
#ifdef SPG_CHECKED
  if (t0 > t1 || t1 > T) {
    if (lane == 0) printf("k_eqs_sum: equation %u terms [%u, %u) past %u\n", e, t0, t1, T);
    t0 = t1 = 0;
  }
#endif
  Ext acc = ext_identity();
  int rejected = 0;
  for (uint32_t t = t0 + lane; t < t1; t += 64) {
    rejected |= tbad[t];
    acc = ext_add(acc, prod[t]);
  }
  const uint32_t len = t1 - t0;
  for (int d = 32; d >= 1; d >>= 1) {
    if (len <= (uint32_t)d) continue;  // lanes d .. 2d - 1 hold the identity (uniform per wavefront)
    Ext o;
    o.X = fp_shfl_down(acc.X, d);
    o.Y = fp_shfl_down(acc.Y, d);
    o.Z = fp_shfl_down(acc.Z, d);
    o.T = fp_shfl_down(acc.T, d);
    acc = ext_add(acc, o);
  }
  rejected = __any(rejected);
  if (lane != 0) return;
  // the ristretto255 identity: X = 0 or Y = 0 (RFC 9496 4.3.3 with (0, 1) on the other side)
  status[e] = rejected ? kEqsBadPoint : (fp_is_zero(acc.X) || fp_is_zero(acc.Y)) ? kEqsIdentity : kEqsNonzero;
  if (sums) {
    if (rejected) {
      for (int k = 0; k < 32; k++) sums[32 * (size_t)e + k] = 0;
    } else {
      ext_compress(acc, sums + 32 * (size_t)e);
    }
  }
}

}  // namespace

// (eqcheck.hpp) spg_last_kernel_us covers the two kernels
int eqs_check_run(spg_ctx* ctx, const EqsView& v, const Niels* base, uint8_t* sums, uint8_t* status, long* bad_term) {
  if (const char* why = eqs_validate(v)) return set_err(ctx, SPG_E_ARG, std::string("spg_eqs_check: ") + why);
  const size_t E = v.E, T = v.T();
  if (bad_term) *bad_term = -1;
  ctx->eqs_equations = E;
  ctx->eqs_terms = T;
  if (!E) return SPG_OK;
  if (!T) {  // empty sums only: the identity, whose encoding is 32 zero bytes
    memset(status, kEqsIdentity, E);
    if (sums) memset(sums, 0, 32 * E);
    return SPG_OK;
  }
  SPG_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // one upload: scalars, extended pool, compressed pool, first (u32), refs, kinds -- each part 32-byte aligned
  auto al = [](size_t x) { return (x + 31) & ~(size_t)31; };
  const size_t o_s = 0, o_x = o_s + 32 * T, o_c = o_x + 128 * v.ne, o_f = o_c + al(32 * v.nc),
               o_r = o_f + al(4 * (E + 1)), o_k = o_r + al(4 * T), in_bytes = o_k + al(T);
  // results: status, the lowest rejected term, the encodings
  const size_t r_bad = al(E), r_sums = r_bad + 32, out_bytes = r_sums + (sums ? 32 * E : 0);
  uint8_t* d_in = (uint8_t*)ws_get(ctx, Ws::EqsIn, in_bytes + 64);
  Ext* d_prod = (Ext*)ws_get(ctx, Ws::EqsProd, T * sizeof(Ext) + al(T) + 64);
  uint8_t* d_out = (uint8_t*)ws_get(ctx, Ws::EqsOut, out_bytes + 64);
  uint8_t* hp = (uint8_t*)pinned_get(ctx, in_bytes + out_bytes);
  if (!d_in || !d_prod || !d_out || !hp) return set_err(ctx, SPG_E_NOMEM, "spg_eqs_check workspace");
  uint8_t* h_out = hp + in_bytes;
  memcpy(hp + o_s, v.scalars, 32 * T);
  if (v.ne) memcpy(hp + o_x, v.extended, 128 * v.ne);
  if (v.nc) memcpy(hp + o_c, v.compressed, 32 * v.nc);
  uint32_t* f32 = (uint32_t*)(hp + o_f);
  for (size_t e = 0; e <= E; e++) f32[e] = (uint32_t)v.first[e];
  memcpy(hp + o_r, v.refs, 4 * T);
  memcpy(hp + o_k, v.kinds, T);
  const int none = INT_MAX;
  memcpy(h_out + r_bad, &none, sizeof(int));
  SPG_HIP(ctx, hipMemcpyAsync(d_in, hp, in_bytes, hipMemcpyHostToDevice, s));
  SPG_HIP(ctx, hipMemcpyAsync(d_out + r_bad, h_out + r_bad, sizeof(int), hipMemcpyHostToDevice, s));
  EqsArgs a{};
  a.kinds = d_in + o_k;
  a.refs = (const uint32_t*)(d_in + o_r);
  a.scalars = (const Fq*)(d_in + o_s);
  a.comp = (const uint32_t*)(d_in + o_c);
  a.ext = (const Ext*)(d_in + o_x);
  a.base = base;
  a.T = (uint32_t)T;
  a.nc = (uint32_t)v.nc;
  a.ne = (uint32_t)v.ne;
  a.nb = (uint32_t)v.nb;
  a.prod = d_prod;
  a.tbad = (uint8_t*)(d_prod + T);
  a.bad = (int*)(d_out + r_bad);
  const EqsPlan p = eqs_plan(T, E);
  timer_start(ctx);
  {
    // modelled: 253 doublings and additions per term, in mixed-addition units (~2 each)
    KScope ks(ctx, "eqs_check", (double)in_bytes + (double)T * 2 * sizeof(Ext), (double)T * 253 * 2);
    hipLaunchKernelGGL(k_eqs_term, dim3(p.term_grid), dim3(kEqsTermBS), 0, s, a);
    hipLaunchKernelGGL(k_eqs_sum, dim3(p.sum_grid), dim3(kEqsSumBS), 0, s, (const Ext*)d_prod, (const uint8_t*)a.tbad,
                       (const uint32_t*)(d_in + o_f), (uint32_t)E, (uint32_t)T, sums ? d_out + r_sums : nullptr, d_out);
  }
  SPG_HIP(ctx, hipGetLastError());
  timer_stop(ctx);
  SPG_HIP(ctx, hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
  SPG_HIP(ctx, hipStreamSynchronize(s));
  memcpy(status, h_out, E);
  if (sums) memcpy(sums, h_out + r_sums, 32 * E);
  int bad;
  memcpy(&bad, h_out + r_bad, sizeof(int));
  if (bad_term) *bad_term = bad == INT_MAX ? -1 : (long)bad;
  float ms = 0.f;
  hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  ctx->last_us = ms * 1000.0;
  return SPG_OK;
}

}  // namespace spg

using namespace spg;

extern "C" int spg_eqs_check(spg_ctx* ctx, const spg_points* base, const uint8_t* compressed, size_t n_compressed,
                             const uint8_t* extended, size_t n_extended, const uint8_t* forms, const uint32_t* operands,
                             const uint64_t* scalars_mont, const size_t* first, size_t E, uint8_t* sums,
                             uint8_t* status, long* bad_term) {
  if (!ctx || (E && (!first || !status))) return SPG_E_ARG;
  EqsView v;
  v.kinds = forms;
  v.refs = operands;
  v.scalars = (const Fq*)scalars_mont;
  v.first = first;
  v.E = E;
  v.compressed = compressed;
  v.nc = n_compressed;
  v.extended = extended;
  v.ne = n_extended;
  v.nb = base ? base->n : 0;
  return eqs_check_run(ctx, v, base ? base->niels : nullptr, sums, status, bad_term);
}

extern "C" int spg_eqs_last_counts(const spg_ctx* ctx, size_t* equations, size_t* terms) {
  if (!ctx) return SPG_E_ARG;
  if (equations) *equations = ctx->eqs_equations;
  if (terms) *terms = ctx->eqs_terms;
  return SPG_OK;
}

extern "C" int spg_set_verify_device(spg_ctx* ctx, int on) {
  if (!ctx) return SPG_E_ARG;
  ctx->verify_device = on != 0;
  return SPG_OK;
}
