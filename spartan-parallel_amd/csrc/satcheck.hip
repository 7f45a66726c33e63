// spg — k_sat_check: Az[i] Bz[i] == Cz[i] over the flat domain of three (p, q_rev, 0, x_rev) tables, the check of the
// reference's R1CSInstance::is_sat (src/r1csinstance.rs:322-357) as one streaming pass over what k_spmv wrote
// (r1cs_tables.hip). A lane takes one stored position: three 32-byte loads, one product, a comparison of canonical residues.
// Only a violating lane looks its descriptor up, to turn the stored position back into the natural key (q and row
// bit-reversed back); a wavefront that found one adds its count and min-reduces its key into the 16-byte record with
// two 64-bit atomics. A satisfying table performs none. Modelled traffic: 96 bytes per row.
#include "satcheck.hpp"

#include "ctx.hpp"
#include "hostmath.hpp"
#include "pqx.hpp"

namespace spg {

namespace {


__device__ __forceinline__ Fq sat_ld(const Fq* p) {  // two 16-byte accesses (the tables are 32-byte aligned)
  const uint4 lo = ((const uint4*)p)[0], hi = ((const uint4*)p)[1];
  Fq r;
  r.l[0] = lo.x, r.l[1] = lo.y, r.l[2] = lo.z, r.l[3] = lo.w;
  r.l[4] = hi.x, r.l[5] = hi.y, r.l[6] = hi.z, r.l[7] = hi.w;
  return r;
}
inline uint64_t blocks_needed(uint64_t n) { return (n + 255) / 256; }
__device__ __forceinline__ uint32_t sat_dbrev(uint32_t v, uint32_t lg) { return lg ? (__brev(v) >> (32 - lg)) : 0u; }

__global__ void __launch_bounds__(256) k_sat_check(const SatArgs a, const Fq* __restrict__ Az,
                                                   const Fq* __restrict__ Bz, const Fq* __restrict__ Cz,
                                                   uint64_t total, unsigned long long* __restrict__ rec) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (t < total) bad = !fq_eq(fq_mul(sat_ld(Az + t), sat_ld(Bz + t)), sat_ld(Cz + t));
  const unsigned long long m = __ballot(bad);
  if (!m) return;  // (uniform over the wavefront)
  unsigned long long key = kSatNoKey;
  if (bad) {  // t < total: the descriptor found owns t, so the key stays inside the instance's own range
    int lo = 0, hi = a.P - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((a.ext ? a.ext[mid].dom_off : a.in[mid].dom_off) <= t) lo = mid;
      else hi = mid - 1;
    }
    const SatDesc d = a.ext ? a.ext[lo] : a.in[lo];
    const uint64_t off = d.dom_off, loc = t - off;
    const uint32_t lgq = d.lg_q, lgx = d.lg_rows;
    const uint32_t qr = (uint32_t)(loc >> lgx), xr = (uint32_t)(loc & (((uint64_t)1 << lgx) - 1));
    key = off + ((uint64_t)sat_dbrev(qr, lgq) << lgx) + sat_dbrev(xr, lgx);
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const unsigned long long o = __shfl_xor(key, s, 64);
    key = o < key ? o : key;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(rec, (unsigned long long)__popcll(m));
    atomicMin(rec + 1, key);
  }
}

}  // namespace

int sat_check_run(spg_ctx* ctx, const std::vector<SatDesc>& d, uint64_t total, const Fq* Az, const Fq* Bz,
                  const Fq* Cz, spg_sat_report* out) {
  memset(out, 0, sizeof(*out));
  out->rows = total;
  if (!total) return SPG_OK;
  if (d.empty() || d.size() >= 0x7fffffffULL || blocks_needed(total) > 0x7fffffffULL)
    return set_err(ctx, SPG_E_ARG, "sat_check: domain too large");
  hipStream_t s = ctx->stream;
  unsigned long long* rec = (unsigned long long*)ws_get(ctx, Ws::SatRec, 64);
  if (!rec) return set_err(ctx, SPG_E_NOMEM, "sat_check record");
  SatArgs a{};
  a.P = (int)d.size();
  if (d.size() > (size_t)kSatMaxP) {
    SatDesc* dd = (SatDesc*)ws_get(ctx, Ws::SatDesc, d.size() * sizeof(SatDesc) + 64);
    if (!dd) return set_err(ctx, SPG_E_NOMEM, "sat_check descriptors");
    // (d outlives the synchronisation below)
    SPG_HIP(ctx, hipMemcpyAsync(dd, d.data(), d.size() * sizeof(SatDesc), hipMemcpyHostToDevice, s));
    a.ext = dd;
  } else {
    for (size_t p = 0; p < d.size(); p++) a.in[p] = d[p];
  }
  // the record cleared: no violations, no key
  SPG_HIP(ctx, hipMemsetAsync(rec, 0, 8, s));
  SPG_HIP(ctx, hipMemsetAsync(rec + 1, 0xff, 8, s));
  {
    KScope ks(ctx, "sat_check", 96.0 * (double)total, 0.0, (double)total);
    hipLaunchKernelGGL(k_sat_check, dim3((unsigned)blocks_needed(total)), dim3(256), 0, s, a, Az, Bz, Cz, total, rec);
  }
  SPG_HIP(ctx, hipGetLastError());
  SatRecord r{0, kSatNoKey};
  SPG_HIP(ctx, hipMemcpyAsync(&r, rec, sizeof(r), hipMemcpyDeviceToHost, s));
  SPG_HIP(ctx, hipStreamSynchronize(s));
  out->violations = r.count;
  if (!r.count) return SPG_OK;
  if (r.key >= total) return set_err(ctx, SPG_E_HIP, "sat_check: the device record holds no row of the domain");
  uint64_t stored = 0;
  sat_decode(d, r.key, &out->p, &out->q, &out->row, &stored);
  Fq v[3];
  if (int rc = d2h_multi(ctx, {{Az + stored, 1}, {Bz + stored, 1}, {Cz + stored, 1}}, v)) return rc;
  memcpy(out->az, &v[0], 32);
  memcpy(out->bz, &v[1], 32);
  memcpy(out->cz, &v[2], 32);
  return SPG_OK;
}

}  // namespace spg

using namespace spg;

extern "C" int spg_pqx_sat_check(spg_ctx* ctx, const spg_pqx* Az, const spg_pqx* Bz, const spg_pqx* Cz,
                                 spg_sat_report* out) {
  if (!ctx || !Az || !Bz || !Cz || !out) return SPG_E_ARG;
  const PqxDev* T[3] = {&Az->T, &Bz->T, &Cz->T};
  const PqxDev& A = *T[0];
  const size_t P = A.zlen;
  if (!P || !A.d) return set_err(ctx, SPG_E_ARG, "spg_pqx_sat_check: empty table");
  size_t off = 0, max_np = 0, max_ni = 0;
  for (const PqxDev* t : T) {
    if (t->zlen != P || t->off.size() != P || t->anp.size() != P || t->anw.size() != P || t->ani.size() != P ||
        t->num_proofs.size() < P || t->num_inputs.size() < P || !t->d)
      return set_err(ctx, SPG_E_ARG, "spg_pqx_sat_check: the three tables differ in shape");
    if (t->num_witness_secs != 1 || t->num_instances != npow2(P))
      return set_err(ctx, SPG_E_ARG, "spg_pqx_sat_check: tables of one witness section, no variable bound");
  }
  for (size_t p = 0; p < P; p++) {
    for (const PqxDev* t : T) {
      if (t->anp[p] != A.anp[p] || t->ani[p] != A.ani[p] || t->max_num_proofs != A.max_num_proofs ||
          t->max_num_inputs != A.max_num_inputs)
        return set_err(ctx, SPG_E_ARG, "spg_pqx_sat_check: the three tables differ in shape");
      if (t->anw[p] != 1 || t->off[p] != off || t->num_proofs[p] != t->anp[p] || t->num_inputs[p] != t->ani[p])
        return set_err(ctx, SPG_E_ARG, "spg_pqx_sat_check: tables of one witness section, no variable bound");
    }
    off += A.anp[p] * A.ani[p];
    max_np = std::max(max_np, A.anp[p]);
    max_ni = std::max(max_ni, A.ani[p]);
  }
  for (const PqxDev* t : T)
    if (t->total != off || t->max_num_proofs < max_np || t->max_num_inputs < max_ni)
      return set_err(ctx, SPG_E_ARG, "spg_pqx_sat_check: tables of one witness section, no variable bound");
  std::vector<SatDesc> d;
  uint64_t total = 0;
  if (const char* why = sat_descs(A.anp.data(), A.ani.data(), P, &d, &total))
    return set_err(ctx, SPG_E_ARG, std::string("spg_pqx_sat_check: ") + why);
  SPG_HIP(ctx, hipSetDevice(ctx->device));
  return sat_check_run(ctx, d, total, A.d, T[1]->d, T[2]->d, out);
}

extern "C" int spg_set_check_sat(spg_ctx* ctx, int on) {
  if (!ctx) return SPG_E_ARG;
  ctx->check_sat = on != 0;
  return SPG_OK;
}
