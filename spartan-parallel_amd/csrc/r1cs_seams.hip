// spg — single operations of R1CSProof::prove as seams on an uploaded instance: the matrix evaluations, multiply_vec_block
// and the eq-weighted tables of phase 2. Each seam checks its arguments, builds its descriptors with the prover's own
// builders (r1cs_desc.hpp) and launches through the prover's own launch functions (r1cs_tables.hpp); only what it
// allocates and when it synchronises is its own.
#include <memory>

#include "comm.hpp"
#include "hostpoly.hpp"
#include "r1cs_tables.hpp"

using namespace spg;

namespace {

// device blocks and result handles under construction: freed on every early return, handles released to the caller
struct DevFree {
  void operator()(void* p) const { hipFree(p); }
};
template <class T>
using DevPtr = std::unique_ptr<T, DevFree>;
template <class T>
DevPtr<T> dev_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) p = nullptr;
  return DevPtr<T>((T*)p);
}
struct PqxFree {
  void operator()(spg_pqx* h) const { spg_pqx_free(nullptr, h); }
};
using PqxPtr = std::unique_ptr<spg_pqx, PqxFree>;
// a handle of `shape` over a device block of its own; null when the block cannot be allocated
PqxPtr pqx_new(const PqxDev& shape) {
  PqxPtr h(new spg_pqx());
  h->T = shape;
  if (hipMalloc(&h->T.d, shape.total * sizeof(Fq) + 64) != hipSuccess) return PqxPtr();
  return h;
}

}  // namespace

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
  const std::vector<MatDesc> md = mat_descs(*inst);
  std::vector<uint32_t> rr(2 * Pm);
  size_t maxrows = 1;
  double visits = 0, rows = 0;
  for (size_t p = 0; p < Pm; p++) {
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
  launch_sparse_eval(ctx, dmd, drr, *inst, erx, ery, part, nblk, dout, visits, rows);
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
// section). The prover's k_spmv launch with the prover's SpDesc list; what differs from the prover's setup: the section
// descriptors point into one upload of z, lg_ni = 0 (sp_descs), never the tiled form, no profiling scope, and the call
// synchronises.
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
  const bool single = inst->num_instances == 1;
  std::vector<size_t> ncons(P);
  size_t zt = 0, total = 0;
  for (size_t p = 0; p < P; p++) {
    ncons[p] = inst->num_cons[single ? 0 : p];
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
  const std::vector<size_t> proofs(num_proofs, num_proofs + P), inputs(num_inputs, num_inputs + P);
  const PqxDev shape = pqx_shape(proofs, 1, ncons, npow2(P), max_num_proofs, 1, inst->max_num_cons);
  const std::vector<SpDesc> spd = sp_descs(proofs, ncons, inputs, shape.off, 0, single, false);
  const std::vector<MatDesc> md = mat_descs(*inst);
  const size_t b_sec = sd.size() * sizeof(SecDesc), b_sp = spd.size() * sizeof(SpDesc),
               b_md = md.size() * sizeof(MatDesc);
  const DevPtr<Fq> d_z = dev_alloc<Fq>(zt * sizeof(Fq) + 64);
  DevPtr<uint8_t> dd;
  if (d_z) dd = dev_alloc<uint8_t>(b_sec + b_sp + b_md + 64);
  if (!dd) return set_err(ctx, SPG_E_NOMEM, "multiply_vec_block");
  PqxPtr outs[3];
  for (PqxPtr& h : outs)
    if (!(h = pqx_new(shape))) return set_err(ctx, SPG_E_NOMEM, "multiply_vec_block outputs");
  for (size_t w = 0; w < num_witness_secs; w++)
    for (size_t p = 0; p < P; p++) {
      SecDesc& s = sd[w * P + p];
      s.w = d_z.get() + soff[w * P + p];
      s.np = (uint32_t)num_proofs[p];
      s.ni = (uint32_t)num_inputs[p];
    }
  std::vector<uint8_t> blob(b_sec + b_sp + b_md);
  memcpy(blob.data(), sd.data(), b_sec);
  memcpy(blob.data() + b_sec, spd.data(), b_sp);
  memcpy(blob.data() + b_sec + b_sp, md.data(), b_md);
  if (hipMemcpy(d_z.get(), zs.data(), zt * sizeof(Fq), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dd.get(), blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess)
    return set_err(ctx, SPG_E_HIP, "multiply_vec_block upload");
  if (total) {
    launch_spmv(ctx, false, false, (const SpDesc*)(dd.get() + b_sec), (int)P, (const MatDesc*)(dd.get() + b_sec + b_sp),
                *inst, (const SecDesc*)dd.get(), (int)num_witness_secs, (uint32_t)max_num_inputs, outs[0]->T.d,
                outs[1]->T.d, outs[2]->T.d, total, 0.0);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
      return set_err(ctx, SPG_E_HIP, "multiply_vec_block launch");
  }
  *Az = outs[0].release();
  *Bz = outs[1].release();
  *Cz = outs[2].release();
  return SPG_OK;
}

// R1CSInstance::compute_eval_table_sparse_disjoint_rounds (src/r1csinstance.rs:484-534, src/sparse_mlpoly.rs:524-541)
// and prove_abc_gen (src/r1csproof.rs:430-465) as seams on a caller's eq(rx): k_abc over the handle's own matrices,
// into new spg_pqx tables of one proof row. split: A, B, C apart, x in natural order (DensePolynomialPqx::new);
// else r_A A + r_B B + r_C C in new_rev order, what the prover's phase2_prep builds. The launch is timed by the
// context's events (spg_last_kernel_us), so it opens no profiling scope.
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
  const std::vector<AbcDesc> ad = abc_descs(cols, shape.off, 0);
  const std::vector<MatDesc> md = mat_descs(*inst);
  const int n_out = split ? 3 : 1;
  const size_t b_ad = Pm * sizeof(AbcDesc), b_md = Pm * sizeof(MatDesc);
  const DevPtr<uint8_t> dd = dev_alloc<uint8_t>(b_ad + b_md + 64);
  if (!dd) return set_err(ctx, SPG_E_NOMEM, w);
  PqxPtr h[3];
  for (int k = 0; k < n_out; k++)
    if (!(h[k] = pqx_new(shape))) return set_err(ctx, SPG_E_NOMEM, w + " outputs");
  std::vector<uint8_t> blob(b_ad + b_md);
  memcpy(blob.data(), ad.data(), b_ad);
  memcpy(blob.data() + b_ad, md.data(), b_md);
  if (hipMemcpy(dd.get(), blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess)
    return set_err(ctx, SPG_E_HIP, w + " upload");
  if (total) {
    timer_start(ctx);
    launch_abc(ctx, false, split, (const AbcDesc*)dd.get(), (int)Pm, (const MatDesc*)(dd.get() + b_ad), *inst,
               evals_rx->d, (uint32_t)max_num_inputs, rA, rB, rC, h[0]->T.d, split ? h[1]->T.d : nullptr,
               split ? h[2]->T.d : nullptr, total, 0.0);
    timer_stop(ctx);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
      return set_err(ctx, SPG_E_HIP, w + " launch");
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) ctx->last_us = ms * 1000.0;
  }
  for (int k = 0; k < n_out; k++) outs[k] = h[k].release();
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
