// spg — the Hyrax dense polynomial commitment scheme on device-resident vectors, one call at a time.
//
//   PolyCommitmentGens::new                        src/dense_mlpoly.rs:31-38    spg_poly_gens_new
//   DensePolynomial::commit / commit_with_blind    :184-256                      spg_poly_commit
//   PolyEvalProof::prove / verify / verify_plain   :437-528                      spg_poly_eval_prove / _verify(_plain)
//   prove_batched_points / verify_plain_..         :531-685                      spg_poly_eval_*_batched_points
//   prove_batched_instances / verify_plain_..      :689-857                      spg_poly_eval_*_batched_instances
//   .._disjoint_rounds / verify_..                 :861-1044                     spg_pe_prove_disjoint / _verify_disjoint
//   prove_uni_batched_instances / verify_..        :1046-1203                    spg_pe_prove_uni / _verify_uni, spg_pe_uni_evals
//
// The prover's O(2^num_vars) work is the bound L.Z of every polynomial of a call (DensePolynomial::bound, :258-265).
// One launch pair computes them all from the plan of pe_plan.hpp:
//   k_pe_part   out of job (Z, L'_0 .. L'_{kt-1}): part_k[y][col] = sum_{j in row range y} L'_k[j] Z[j Rs + col]
//   k_pe_sum    out_g[col] = sum of the S_g slabs of group g (the slabs of a group's terms are contiguous)
// L'_i = c_i L_i is the eq table already scaled by the term's batching coefficient, so the random linear combination
// sum_k c^k L_k.Z_k of the instances form comes out of the second launch; in the points form one read of Z can feed
// up to kPeKTMax accumulators (the plan gives it kPeKT = 1: the measured tile did not pay, pe_plan.hpp). Job and
// group descriptors live in device memory: a call's polynomial count is limited by memory alone. Fq sums are exact
// and canonical, so the result does not depend on the summation order.
// The univariate form adds polynomials of different widths into one vector; its second launch is k_pe_sum_ragged over
// per-term slab descriptors (pe_bound_ragged, pe_plan_uni).
// The Bullet reductions (dotproduct_log_prove) and the verifier's checks (verify.hip) are the whole-proof paths'.
//
// SNARK::prove's PolyEvalProof provers on host polynomials live here too (pe_prove.hpp): prove_batched_points,
// prove_batched_instances, uni_bounds / prove_uni_batched (:1046-1130). They bind on the host pool (host_bounds) and
// take their slots and exponents from the same walk (pe_plan.hpp) as the entries above.
#include <string.h>

#include <algorithm>
#include <string>

#include "hostpoly.hpp"
#include "pe_bound.hpp"
#include "pe_plan.hpp"
#include "pe_prove.hpp"
#include "pe_verify.hpp"
#include "proto.hpp"

struct spg_poly_gens {  // PolyCommitmentGens: gens_n = G_0 .. G_{n-1} with h, gens_1 = G_n with the same h
  spg::ProverGens g;
};

namespace spg {


// Every L.Z vector of a plan in one launch pair and one download. Z: the polynomial of every term (points form: of
// term 0, shared by all). Lp: the scaled eq table of every bound term, in term order. out: plan.out_len scalars, group g
// at its out_off.
static int pe_bound(spg_ctx* ctx, const PePlan& plan, bool points, const std::vector<const Fq*>& Z,
                    const std::vector<FqV>& Lp, FqV* out) {
  std::vector<size_t> offL;  // per bound term, in term order
  FqV Lall;
  for (const FqV& l : Lp) {
    offL.push_back(Lall.size());
    Lall.insert(Lall.end(), l.begin(), l.end());
  }
  std::vector<PeJob> jobs;
  uint32_t b0 = 0, Smax = 1;
  double zbytes = 0;
  auto close_job = [&](PeJob& j) {
    j.b0 = b0;
    b0 += (uint32_t)((j.Rs + 255) / 256);
    Smax = std::max(Smax, j.S);
    zbytes += 32.0 * (double)j.Ls * (double)j.Rs;
    jobs.push_back(j);
  };
  size_t bi = 0;  // bound terms met so far
  if (points) {
    const size_t D = plan.groups.size();
    for (size_t p0 = 0; p0 < D; p0 += kPeKT) {
      PeJob j;
      memset(&j, 0, sizeof(j));
      const PeGroup& g0 = plan.groups[p0];
      const PeTerm& t0 = plan.terms[g0.first];
      j.Z = Z[0], j.Rs = g0.Rs, j.Ls = (uint32_t)g0.Ls, j.chunk = (uint32_t)t0.chunk, j.S = (uint32_t)t0.S;
      j.kt = (uint32_t)std::min<size_t>(kPeKT, D - p0);
      for (uint32_t k = 0; k < j.kt; k++) {  // group p0 + k is the (p0 + k)-th bound term
        j.offL[k] = offL[p0 + k];
        j.offP[k] = plan.groups[p0 + k].part_off;
      }
      close_job(j);
    }
  } else {
    for (size_t i = 0; i < plan.terms.size(); i++) {
      const PeTerm& t = plan.terms[i];
      const PeGroup& g = plan.groups[t.group];
      PeJob j;
      memset(&j, 0, sizeof(j));
      j.Z = Z[i], j.Rs = g.Rs, j.Ls = (uint32_t)g.Ls, j.chunk = (uint32_t)t.chunk, j.S = (uint32_t)t.S, j.kt = 1;
      j.offL[0] = offL[bi++];
      j.offP[0] = g.part_off + t.slab * g.Rs;
      close_job(j);
    }
  }
  std::vector<PeSum> sums;
  uint32_t c0 = 0;
  for (const PeGroup& g : plan.groups) {
    sums.push_back(PeSum{g.part_off, g.out_off, g.Rs, (uint32_t)g.S, c0});
    c0 += (uint32_t)((g.Rs + kPeSumCols - 1) / kPeSumCols);
  }
  if (b0 != plan.xblocks) return set_err(ctx, SPG_E_ARG, "poly eval: plan and jobs disagree");
  PeJob* dj = (PeJob*)ws_get(ctx, Ws::PeJobs, jobs.size() * sizeof(PeJob) + 64);
  PeSum* ds = (PeSum*)ws_get(ctx, Ws::PeSums, sums.size() * sizeof(PeSum) + 64);
  Fq* dL = (Fq*)ws_get(ctx, Ws::PeL, Lall.size() * sizeof(Fq) + 64);
  Fq* dpart = (Fq*)ws_get(ctx, Ws::PePart, plan.part_len * sizeof(Fq) + 64);
  Fq* dout = (Fq*)ws_get(ctx, Ws::PeOut, plan.out_len * sizeof(Fq) + 64);
  if (!dj || !ds || !dL || !dpart || !dout) return set_err(ctx, SPG_E_NOMEM, "poly eval: bound workspace");
  hipStream_t s = ctx->stream;
  SPG_HIP(ctx, hipMemcpyAsync(dj, jobs.data(), jobs.size() * sizeof(PeJob), hipMemcpyHostToDevice, s));
  SPG_HIP(ctx, hipMemcpyAsync(ds, sums.data(), sums.size() * sizeof(PeSum), hipMemcpyHostToDevice, s));
  SPG_HIP(ctx, hipMemcpyAsync(dL, Lall.data(), Lall.size() * sizeof(Fq), hipMemcpyHostToDevice, s));
  {
    // Z once per job (the points form: once per kPeKT distinct L vectors), the partials written and read back
    KScope ks(ctx, "pe_bound", zbytes + 64.0 * (double)plan.part_len);
    hipLaunchKernelGGL(k_pe_part, dim3(b0, Smax), dim3(256), 0, s, dj, (uint32_t)jobs.size(), dL, dpart, plan.part_len);
    hipLaunchKernelGGL(k_pe_sum, dim3(c0), dim3(256), 0, s, ds, (uint32_t)sums.size(), dpart, dout, plan.out_len);
    if (hipGetLastError() != hipSuccess) return set_err(ctx, SPG_E_HIP, "poly eval: bound launch");
  }
  out->assign(plan.out_len, fq_zero());
  return d2h_fq(ctx, dout, out->data(), plan.out_len);  // synchronises: the host vectors above outlive their copies
}

// The univariate plan's bound, likewise one launch pair and one download whatever the polynomial count: k_pe_part with
// one kt = 1 job per term, then k_pe_sum_ragged over the plan's groups (all terms into one vector of R_size, or one
// group per term). Lp: the scaled power table of every term.
static int pe_bound_ragged(spg_ctx* ctx, const PeUniPlan& plan, const std::vector<const Fq*>& Z,
                           const std::vector<FqV>& Lp, FqV* out) {
  const size_t n = plan.terms.size();
  FqV Lall;
  std::vector<PeJob> jobs(n);
  std::vector<PeRagTerm> terms(n);
  uint32_t b0 = 0, Smax = 1;
  double zbytes = 0;
  for (size_t i = 0; i < n; i++) {
    const PeUniTerm& t = plan.terms[i];
    PeJob& j = jobs[i];
    memset(&j, 0, sizeof(j));
    j.Z = Z[i], j.Rs = t.Rs, j.Ls = (uint32_t)t.Ls, j.chunk = (uint32_t)t.chunk, j.S = (uint32_t)t.S, j.kt = 1;
    j.offL[0] = Lall.size();
    j.offP[0] = t.part_off;
    j.b0 = b0;
    b0 += (uint32_t)((t.Rs + 255) / 256);
    Smax = std::max(Smax, j.S);
    zbytes += 32.0 * (double)t.Ls * (double)t.Rs;
    Lall.insert(Lall.end(), Lp[i].begin(), Lp[i].end());
    terms[i] = PeRagTerm{t.part_off, t.Rs, (uint32_t)t.S};
  }
  std::vector<PeRagSum> sums;
  uint32_t c0 = 0;
  auto add_group = [&](size_t o, size_t Rs, size_t t0, size_t nt) {
    sums.push_back(PeRagSum{o, Rs, (uint32_t)t0, (uint32_t)nt, c0});
    c0 += (uint32_t)((Rs + kPeSumCols - 1) / kPeSumCols);
  };
  if (plan.per_term)
    for (size_t i = 0; i < n; i++) add_group(plan.terms[i].out_off, plan.terms[i].Rs, i, 1);
  else
    add_group(0, plan.R_size, 0, n);
  if (b0 != plan.xblocks) return set_err(ctx, SPG_E_ARG, "poly eval: plan and jobs disagree");
  PeJob* dj = (PeJob*)ws_get(ctx, Ws::PeJobs, jobs.size() * sizeof(PeJob) + 64);
  PeRagSum* ds = (PeRagSum*)ws_get(ctx, Ws::PeSums, sums.size() * sizeof(PeRagSum) + 64);
  PeRagTerm* dt = (PeRagTerm*)ws_get(ctx, Ws::PeRagTerms, terms.size() * sizeof(PeRagTerm) + 64);
  Fq* dL = (Fq*)ws_get(ctx, Ws::PeL, Lall.size() * sizeof(Fq) + 64);
  Fq* dpart = (Fq*)ws_get(ctx, Ws::PePart, plan.part_len * sizeof(Fq) + 64);
  Fq* dout = (Fq*)ws_get(ctx, Ws::PeOut, plan.out_len * sizeof(Fq) + 64);
  if (!dj || !ds || !dt || !dL || !dpart || !dout) return set_err(ctx, SPG_E_NOMEM, "poly eval: bound workspace");
  hipStream_t s = ctx->stream;
  SPG_HIP(ctx, hipMemcpyAsync(dj, jobs.data(), jobs.size() * sizeof(PeJob), hipMemcpyHostToDevice, s));
  SPG_HIP(ctx, hipMemcpyAsync(ds, sums.data(), sums.size() * sizeof(PeRagSum), hipMemcpyHostToDevice, s));
  SPG_HIP(ctx, hipMemcpyAsync(dt, terms.data(), terms.size() * sizeof(PeRagTerm), hipMemcpyHostToDevice, s));
  SPG_HIP(ctx, hipMemcpyAsync(dL, Lall.data(), Lall.size() * sizeof(Fq), hipMemcpyHostToDevice, s));
  {
    KScope ks(ctx, "pe_bound_ragged", zbytes + 64.0 * (double)plan.part_len);
    hipLaunchKernelGGL(k_pe_part, dim3(b0, Smax), dim3(256), 0, s, dj, (uint32_t)jobs.size(), dL, dpart, plan.part_len);
    hipLaunchKernelGGL(k_pe_sum_ragged, dim3(c0), dim3(256), 0, s, ds, (uint32_t)sums.size(), dt, dpart, plan.part_len,
                       dout, plan.out_len);
    if (hipGetLastError() != hipSuccess) return set_err(ctx, SPG_E_HIP, "poly eval: bound launch");
  }
  out->assign(plan.out_len, fq_zero());
  return d2h_fq(ctx, dout, out->data(), plan.out_len);  // synchronises: the host vectors above outlive their copies
}

static FqV lds(const uint64_t* p, size_t n) {
  FqV v(n);
  for (size_t i = 0; i < n; i++) v[i] = ld_fq(p + 4 * i);
  return v;
}
static bool nv_ok(size_t nv) { return nv >= 1 && nv <= kPeMaxVars; }
static size_t rs_of(size_t nv) { return (size_t)1 << (nv - nv / 2); }
static int put_bytes(spg_ctx* ctx, const Writer& w, uint8_t* proof, size_t cap, const char* what) {
  if (w.out.size() > cap) return set_err(ctx, SPG_E_ARG, std::string(what) + ": proof size differs from its shapes'");
  memcpy(proof, w.out.data(), w.out.size());
  return SPG_OK;
}

static int commit_impl(spg_ctx* ctx, const spg_poly_gens* pg, const spg_buf* Z, size_t offset, size_t nv,
                       const uint64_t* blinds, uint8_t* comm, size_t comm_cap, size_t* L_out) {
  if (!ctx || !pg || !Z || !comm || !L_out) return SPG_E_ARG;
  if (!nv_ok(nv)) return set_err(ctx, SPG_E_ARG, "poly commit: num_vars must be 1 .. 30");
  const size_t L = (size_t)1 << (nv / 2), R = rs_of(nv);
  if (R > pg->g.n_pc) return set_err(ctx, SPG_E_ARG, "poly commit: polynomial wider than the generators");
  if (offset > Z->n || ((size_t)1 << nv) > Z->n - offset) return set_err(ctx, SPG_E_ARG, "poly commit: Z too short");
  *L_out = L;
  if (32 * L > comm_cap) return set_err(ctx, SPG_E_ARG, "poly commit: output buffer too small");
  SPG_HIP(ctx, hipSetDevice(ctx->device));
  ProverGens& g = const_cast<ProverGens&>(pg->g);
  if (!blinds) return commit_rows(ctx, g, Z->d + offset, R, L, reinterpret_cast<Pt*>(comm));
  Fq* db = (Fq*)ws_get(ctx, Ws::PeBlinds, L * sizeof(Fq) + 64);
  if (!db) return set_err(ctx, SPG_E_NOMEM, "poly commit: blinds");
  const FqV hb = lds(blinds, L);
  SPG_HIP(ctx, hipMemcpyAsync(db, hb.data(), L * sizeof(Fq), hipMemcpyHostToDevice, ctx->stream));
  return msm_rows_host_enc(ctx, g.dev, Z->d + offset, R, L, db, -1, comm);  // synchronous: hb outlives its copy
}

static int prove_impl(spg_ctx* ctx, const spg_poly_gens* pg, const spg_buf* Z, size_t offset, const uint64_t* r_mont,
                      size_t nv, const uint64_t* Zr, const uint64_t* blinds, const uint64_t* blind_Zr,
                      spg_transcript* tr, spg_random_tape* tape, uint8_t* proof, size_t cap, size_t* len,
                      uint8_t* C_Zr) {
  if (!ctx || !pg || !Z || !r_mont || !Zr || !tr || !tape || !proof || !len) return SPG_E_ARG;
  if (!nv_ok(nv)) return set_err(ctx, SPG_E_ARG, "poly eval prove: num_vars must be 1 .. 30");
  const size_t Ls = (size_t)1 << (nv / 2), Rs = rs_of(nv);
  if (Rs > pg->g.n_pc) return set_err(ctx, SPG_E_ARG, "poly eval prove: polynomial wider than the generators");
  if (offset > Z->n || ((size_t)1 << nv) > Z->n - offset) return set_err(ctx, SPG_E_ARG, "poly eval prove: Z too short");
  *len = pe_proof_bytes(Rs);
  if (*len > cap) return set_err(ctx, SPG_E_ARG, "poly eval prove: proof buffer too small");
  SPG_HIP(ctx, hipSetDevice(ctx->device));
  ProverGens& g = const_cast<ProverGens&>(pg->g);
  Tr& t = tr->t;
  t.protocol("polynomial evaluation proof");
  const FqV r = lds(r_mont, nv);
  const PePlan plan = pe_plan_instances(&nv, r.data(), &nv, 1);
  FqV L, R, LZ;
  pe_eq_halves(r, &L, &R);
  int rc = pe_bound(ctx, plan, false, {Z->d + offset}, {L}, &LZ);
  if (rc) return rc;
  Fq LZ_blind = fq_zero();
  for (size_t i = 0; blinds && i < Ls; i++) LZ_blind = fq_add(LZ_blind, fq_mul(ld_fq(blinds + 4 * i), L[i]));
  DotProductProofLogP p;
  Pt cy;
  rc = dotproduct_log_prove(ctx, g, t, tape->t, LZ, LZ_blind, R, ld_fq(Zr), blind_Zr ? ld_fq(blind_Zr) : fq_zero(), &p,
                            &cy);
  if (rc) return rc;
  Writer w;
  p.ser(w);
  if (C_Zr) memcpy(C_Zr, cy.b, 32);
  return put_bytes(ctx, w, proof, cap, "poly eval prove");
}

// one DotProductProofLog per proof slot: bincode(Vec<PolyEvalProof>)
static int prove_slots(spg_ctx* ctx, ProverGens& g, const std::vector<FqV>& LZs, const std::vector<FqV>& Rs,
                       const FqV& Zc, Tr& t, Tape& tape, Writer& w) {
  w.u64(LZs.size());
  for (size_t k = 0; k < LZs.size(); k++) {
    DotProductProofLogP p;
    Pt cy;
    const int rc = dotproduct_log_prove(ctx, g, t, tape, LZs[k], fq_zero(), Rs[k], Zc[k], fq_zero(), &p, &cy);
    if (rc) return rc;
    p.ser(w);
  }
  return 0;
}
// the proofs of a plan's groups, in order, after their bounds
static int prove_groups(spg_ctx* ctx, ProverGens& g, const PePlan& plan, const FqV& LZ, const std::vector<FqV>& Rg,
                        const FqV& Zc, Tr& t, Tape& tape, Writer& w) {
  std::vector<FqV> x;
  for (const PeGroup& gr : plan.groups) x.emplace_back(LZ.begin() + gr.out_off, LZ.begin() + gr.out_off + gr.Rs);
  return prove_slots(ctx, g, x, Rg, Zc, t, tape, w);
}

static int prove_points_impl(spg_ctx* ctx, const spg_poly_gens* pg, const spg_buf* Z, size_t offset, size_t nv,
                             const uint64_t* r_list, size_t K, const uint64_t* Zr_list, spg_transcript* tr,
                             spg_random_tape* tape, uint8_t* proof, size_t cap, size_t* len) {
  if (!ctx || !pg || !Z || !r_list || !Zr_list || !tr || !tape || !proof || !len || K == 0) return SPG_E_ARG;
  if (!nv_ok(nv)) return set_err(ctx, SPG_E_ARG, "poly eval prove (points): num_vars must be 1 .. 30");
  if (rs_of(nv) > pg->g.n_pc) return set_err(ctx, SPG_E_ARG, "poly eval prove (points): polynomial wider than the generators");
  if (offset > Z->n || ((size_t)1 << nv) > Z->n - offset)
    return set_err(ctx, SPG_E_ARG, "poly eval prove (points): Z too short");
  const FqV rs = lds(r_list, K * nv), Zr = lds(Zr_list, K);
  const PePlan plan = pe_plan_points(rs.data(), K, nv);
  *len = pe_list_bytes(plan);
  if (*len > cap) return set_err(ctx, SPG_E_ARG, "poly eval prove (points): proof buffer too small");
  SPG_HIP(ctx, hipSetDevice(ctx->device));
  ProverGens& g = const_cast<ProverGens&>(pg->g);
  Tr& t = tr->t;
  t.protocol("polynomial evaluation proof");
  const FqV c = pe_coeff_powers(t.challenge("challenge_c"), plan.terms.size() - plan.groups.size());
  const size_t D = plan.groups.size();
  std::vector<FqV> Lp, Rg(D);
  FqV Zc(D, fq_zero());
  for (size_t i = 0; i < K; i++) {
    const PeTerm& tm = plan.terms[i];
    FqV L, R;
    pe_eq_halves(tm.r, &L, &R);
    if (tm.bound) {
      Lp.push_back(L);
      Rg[tm.group] = R;
      Zc[tm.group] = Zr[i];
    } else {  // R_idx += c R_i, Zc_idx += c Zr_i: Rs-sized host work
      FqV& dst = Rg[tm.group];
      for (size_t j = 0; j < R.size(); j++) dst[j] = fq_add(dst[j], fq_mul(c[tm.exp], R[j]));
      Zc[tm.group] = fq_add(Zc[tm.group], fq_mul(c[tm.exp], Zr[i]));
    }
  }
  FqV LZ;
  int rc = pe_bound(ctx, plan, true, {Z->d + offset}, Lp, &LZ);
  if (rc) return rc;
  Writer w;
  rc = prove_groups(ctx, g, plan, LZ, Rg, Zc, t, tape->t, w);
  return rc ? rc : put_bytes(ctx, w, proof, cap, "poly eval prove (points)");
}

// The instances and disjoint-rounds forms after their plan (whose shapes and polynomials the caller has checked): every
// term is bound with its eq table, a repeat's scaled by its coefficient, then one proof per group
static int prove_all_bound(spg_ctx* ctx, const spg_poly_gens* pg, const PePlan& plan, const spg_buf* const* polys,
                           const size_t* offsets, const FqV& Zr, spg_transcript* tr, spg_random_tape* tape,
                           uint8_t* proof, size_t cap, size_t* len, const char* what) {
  const size_t n = plan.terms.size();
  *len = pe_list_bytes(plan);
  if (*len > cap) return set_err(ctx, SPG_E_ARG, std::string(what) + ": proof buffer too small");
  SPG_HIP(ctx, hipSetDevice(ctx->device));
  ProverGens& g = const_cast<ProverGens&>(pg->g);
  Tr& t = tr->t;
  t.protocol("polynomial evaluation proof");
  const FqV c = pe_coeff_powers(t.challenge("challenge_c"), plan.terms.size() - plan.groups.size());
  const size_t D = plan.groups.size();
  std::vector<FqV> Lp(n), Rg(D);
  std::vector<const Fq*> Zs(n);
  FqV Zc(D, fq_zero());
  for (size_t i = 0; i < n; i++) {
    const PeTerm& tm = plan.terms[i];
    Zs[i] = polys[i]->d + offsets[i];
    const size_t ln = tm.nv / 2;
    Lp[i] = eq_evals_host(FqV(tm.r.begin(), tm.r.begin() + ln));
    if (tm.exp) {  // L'_i = c L_i: the kernel's group sum is then LZ_idx += c LZ_i
      for (Fq& x : Lp[i]) x = fq_mul(x, c[tm.exp]);
      Zc[tm.group] = fq_add(Zc[tm.group], fq_mul(c[tm.exp], Zr[i]));
    } else {
      Rg[tm.group] = eq_evals_host(FqV(tm.r.begin() + ln, tm.r.end()));
      Zc[tm.group] = Zr[i];
    }
  }
  FqV LZ;
  int rc = pe_bound(ctx, plan, false, Zs, Lp, &LZ);
  if (rc) return rc;
  Writer w;
  rc = prove_groups(ctx, g, plan, LZ, Rg, Zc, t, tape->t, w);
  return rc ? rc : put_bytes(ctx, w, proof, cap, what);
}

// the shapes of a disjoint-rounds list, checked before anything else reads them
static int disjoint_args(spg_ctx* ctx, const spg_poly_gens* pg, const size_t* np_list, const size_t* ni_list, size_t n,
                         size_t rq_len, const char* what) {
  auto pow2 = [](size_t x) { return x && !(x & (x - 1)); };
  for (size_t i = 0; i < n; i++) {
    if (!pow2(np_list[i]) || !pow2(ni_list[i]))
      return set_err(ctx, SPG_E_ARG, std::string(what) + ": num_proofs and num_inputs must be powers of two");
    const size_t nv = lg2(np_list[i]) + lg2(ni_list[i]);
    if (!nv_ok(nv)) return set_err(ctx, SPG_E_ARG, std::string(what) + ": num_vars must be 1 .. 30");
    if (lg2(np_list[i]) > rq_len) return set_err(ctx, SPG_E_ARG, std::string(what) + ": rq shorter than lg num_proofs");
    if (rs_of(nv) > pg->g.n_pc)
      return set_err(ctx, SPG_E_ARG, std::string(what) + ": polynomial wider than the generators");
  }
  return SPG_OK;
}

// the shapes of an instance list, checked before anything else reads them; *tot_r = scalars of r_list
static int instances_args(spg_ctx* ctx, const spg_poly_gens* pg, const size_t* nv_list, const size_t* r_lens, size_t n,
                          size_t* tot_r, const char* what) {
  *tot_r = 0;
  for (size_t i = 0; i < n; i++) {
    if (!nv_ok(nv_list[i])) return set_err(ctx, SPG_E_ARG, std::string(what) + ": num_vars must be 1 .. 30");
    if (rs_of(nv_list[i]) > pg->g.n_pc)
      return set_err(ctx, SPG_E_ARG, std::string(what) + ": polynomial wider than the generators");
    *tot_r += r_lens[i];
  }
  return SPG_OK;
}

static int prove_instances_impl(spg_ctx* ctx, const spg_poly_gens* pg, const spg_buf* const* polys,
                                const size_t* offsets, const size_t* nv_list, size_t n, const uint64_t* r_list,
                                const size_t* r_lens, const uint64_t* Zr_list, spg_transcript* tr,
                                spg_random_tape* tape, uint8_t* proof, size_t cap, size_t* len) {
  if (!ctx || !pg || !polys || !offsets || !nv_list || !r_list || !r_lens || !Zr_list || !tr || !tape || !proof ||
      !len || n == 0)
    return SPG_E_ARG;
  size_t tot_r = 0;
  int rc = instances_args(ctx, pg, nv_list, r_lens, n, &tot_r, "poly eval prove (instances)");
  if (rc) return rc;
  for (size_t i = 0; i < n; i++) {
    if (!polys[i]) return SPG_E_ARG;
    if (offsets[i] > polys[i]->n || ((size_t)1 << nv_list[i]) > polys[i]->n - offsets[i])
      return set_err(ctx, SPG_E_ARG, "poly eval prove (instances): Z too short");
  }
  const FqV rs = lds(r_list, tot_r);
  return prove_all_bound(ctx, pg, pe_plan_instances(nv_list, rs.data(), r_lens, n), polys, offsets, lds(Zr_list, n), tr,
                         tape, proof, cap, len, "poly eval prove (instances)");
}

// prove_batched_instances_disjoint_rounds (:861-960): the same prover over the plan of the (num_proofs, num_inputs) keys
static int prove_disjoint_impl(spg_ctx* ctx, const spg_poly_gens* pg, const spg_buf* const* polys,
                               const size_t* offsets, const size_t* np_list, const size_t* ni_list, size_t n,
                               const uint64_t* rq, size_t rq_len, const uint64_t* ry, size_t ry_len,
                               const uint64_t* Zr_list, spg_transcript* tr, spg_random_tape* tape, uint8_t* proof,
                               size_t cap, size_t* len) {
  if (!ctx || !pg || !polys || !offsets || !np_list || !ni_list || !rq || !ry || !Zr_list || !tr || !tape || !proof ||
      !len || n == 0)
    return SPG_E_ARG;
  int rc = disjoint_args(ctx, pg, np_list, ni_list, n, rq_len, "poly eval prove (disjoint)");
  if (rc) return rc;
  for (size_t i = 0; i < n; i++) {
    if (!polys[i]) return SPG_E_ARG;
    if (offsets[i] > polys[i]->n || np_list[i] * ni_list[i] > polys[i]->n - offsets[i])
      return set_err(ctx, SPG_E_ARG, "poly eval prove (disjoint): Z too short");
  }
  const FqV q = lds(rq, rq_len), y = lds(ry, ry_len);
  return prove_all_bound(ctx, pg, pe_plan_disjoint(np_list, ni_list, n, q.data(), rq_len, y.data(), ry_len), polys,
                         offsets, lds(Zr_list, n), tr, tape, proof, cap, len, "poly eval prove (disjoint)");
}

// the polynomials of a univariate call, checked before anything else reads them; *max_nv = the widest
static int uni_args(spg_ctx* ctx, const spg_poly_gens* pg, const spg_buf* const* polys, const size_t* offsets,
                    const size_t* nv_list, size_t n, size_t* max_nv, const char* what) {
  *max_nv = 0;
  for (size_t i = 0; i < n; i++) {
    if (!polys[i]) return SPG_E_ARG;
    if (!nv_ok(nv_list[i])) return set_err(ctx, SPG_E_ARG, std::string(what) + ": num_vars must be 1 .. 30");
    if (offsets[i] > polys[i]->n || ((size_t)1 << nv_list[i]) > polys[i]->n - offsets[i])
      return set_err(ctx, SPG_E_ARG, std::string(what) + ": Z too short");
    *max_nv = std::max(*max_nv, nv_list[i]);
  }
  if (pg && rs_of(*max_nv) > pg->g.n_pc)
    return set_err(ctx, SPG_E_ARG, std::string(what) + ": polynomial wider than the generators");
  return SPG_OK;
}

// the evaluations the univariate form opens: Z_i(r) = sum_k Z_i[k] r^k = sum_col (L_i.Z_i)[col] r^col with the
// unscaled power tables, one output per term
static int uni_evals_impl(spg_ctx* ctx, const spg_buf* const* polys, const size_t* offsets, const size_t* nv_list,
                          size_t n, const uint64_t* r_mont, uint64_t* Zr_out) {
  if (!ctx || !polys || !offsets || !nv_list || !r_mont || !Zr_out || n == 0) return SPG_E_ARG;
  size_t max_nv = 0;
  int rc = uni_args(ctx, nullptr, polys, offsets, nv_list, n, &max_nv, "poly uni evals");
  if (rc) return rc;
  SPG_HIP(ctx, hipSetDevice(ctx->device));
  const Fq r = ld_fq(r_mont);
  const std::vector<size_t> nvs(nv_list, nv_list + n);
  const PeUniPlan plan = pe_plan_uni(nv_list, n, true);
  const PeUniL u = pe_uni_Ls(r, nvs);
  std::vector<FqV> Lp(n);
  std::vector<const Fq*> Zs(n);
  for (size_t i = 0; i < n; i++) Lp[i] = u.L[u.of[i]], Zs[i] = polys[i]->d + offsets[i];
  FqV LZ;
  rc = pe_bound_ragged(ctx, plan, Zs, Lp, &LZ);
  if (rc) return rc;
  const FqV R = pe_uni_R(r, max_nv);
  for (size_t i = 0; i < n; i++) {
    const PeUniTerm& t = plan.terms[i];
    Fq e = fq_zero();
    for (size_t k = 0; k < t.Rs; k++) e = fq_add(e, fq_mul(LZ[t.out_off + k], R[k]));
    st_fq(Zr_out + 4 * i, e);
  }
  return SPG_OK;
}

// prove_uni_batched_instances (:1046-1130): term i joins with c^i (L'_i = c^i L_i), all into one vector of R_size
static int prove_uni_impl(spg_ctx* ctx, const spg_poly_gens* pg, const spg_buf* const* polys, const size_t* offsets,
                          const size_t* nv_list, size_t n, const uint64_t* r_mont, const uint64_t* Zr_list,
                          spg_transcript* tr, spg_random_tape* tape, uint8_t* proof, size_t cap, size_t* len,
                          uint8_t* C_Zr) {
  if (!ctx || !pg || !polys || !offsets || !nv_list || !r_mont || !Zr_list || !tr || !tape || !proof || !len || n == 0)
    return SPG_E_ARG;
  size_t max_nv = 0;
  int rc = uni_args(ctx, pg, polys, offsets, nv_list, n, &max_nv, "poly eval prove (uni)");
  if (rc) return rc;
  *len = pe_proof_bytes(rs_of(max_nv));
  if (*len > cap) return set_err(ctx, SPG_E_ARG, "poly eval prove (uni): proof buffer too small");
  SPG_HIP(ctx, hipSetDevice(ctx->device));
  ProverGens& g = const_cast<ProverGens&>(pg->g);
  Tr& t = tr->t;
  t.protocol("polynomial evaluation proof");
  const Fq r = ld_fq(r_mont);
  const FqV Zr = lds(Zr_list, n), R = pe_uni_R(r, max_nv);
  const Fq c_base = t.challenge("challenge_c");
  const PeUniPlan plan = pe_plan_uni(nv_list, n, false);
  const std::vector<FqV> Lp = pe_uni_scaled_Ls(r, std::vector<size_t>(nv_list, nv_list + n), c_base);
  std::vector<const Fq*> Zs(n);
  Fq Zrc = fq_zero(), c = fq_one();
  for (size_t i = 0; i < n; i++, c = fq_mul(c, c_base)) {
    Zs[i] = polys[i]->d + offsets[i];
    Zrc = fq_add(Zrc, fq_mul(c, Zr[i]));
  }
  FqV LZc;
  rc = pe_bound_ragged(ctx, plan, Zs, Lp, &LZc);
  if (rc) return rc;
  DotProductProofLogP p;
  Pt cy;
  rc = dotproduct_log_prove(ctx, g, t, tape->t, LZc, fq_zero(), R, Zrc, fq_zero(), &p, &cy);
  if (rc) return rc;
  Writer w;
  p.ser(w);
  if (C_Zr) memcpy(C_Zr, cy.b, 32);
  return put_bytes(ctx, w, proof, cap, "poly eval prove (uni)");
}

// ---- the whole-proof provers of SNARK::prove, on host polynomials (pe_prove.hpp)
// DensePolynomial::bound (dense_mlpoly.rs:258-265) of several host (Z, L) pairs in one pool burst: each job's columns
// are cut into slices of >= ~2048 products, all slices of all jobs go to the pool together (one wake-up instead of
// one per polynomial)
static std::vector<FqV> host_bounds(const std::vector<std::pair<const FqV*, const FqV*>>& jobs) {
  std::vector<FqV> out(jobs.size());
  struct Slice {
    size_t j, Ls, Rs, i0, i1;
  };
  std::vector<Slice> sl;
  for (size_t j = 0; j < jobs.size(); j++) {
    const size_t nv = lg2(jobs[j].first->size()), Ls = (size_t)1 << (nv / 2), Rs = (size_t)1 << (nv - nv / 2);
    out[j].assign(Rs, fq_zero());
    const size_t C = std::max<size_t>(1, std::min<size_t>({8, Rs, Ls * Rs / 2048}));
    for (size_t c = 0; c < C; c++) sl.push_back({j, Ls, Rs, Rs * c / C, Rs * (c + 1) / C});
  }
  auto run = [&](int k) {
    const Slice& s = sl[k];
    const FqV& Z = *jobs[s.j].first;
    const FqV& L = *jobs[s.j].second;
    FqV& o = out[s.j];
    for (size_t j = 0; j < s.Ls; j++)
      for (size_t i = s.i0; i < s.i1; i++) o[i] = fq_add(o[i], fq_mul(L[j], Z[j * s.Rs + i]));
  };
  if (sl.size() == 1)
    run(0);
  else if (!sl.empty())
    pool().parallel_for((int)sl.size(), run);
  return out;
}
int prove_batched_points(spg_ctx* ctx, ProverGens& g, const FqV& Z, const std::vector<FqV>& r_list, const FqV& Zr,
                         Tr& t, Tape& tape, Writer& w) {
  t.protocol("polynomial evaluation proof");
  const PeWalk wk = pe_walk_points(r_list);
  const FqV c = pe_coeff_powers(t.challenge("challenge_c"), wk.repeats());
  const size_t D = wk.first.size();
  std::vector<FqV> Ls(D), Rs(D), Rv(r_list.size());
  FqV Zc(D);
  std::vector<Axpy> ax;  // Rs[k] += c R_i
  for (size_t i = 0; i < r_list.size(); i++) {
    const size_t k = wk.group[i];
    FqV L;
    pe_eq_halves(r_list[i], &L, &Rv[i]);
    if (wk.opens(i)) {
      Ls[k] = L, Rs[k] = Rv[i], Zc[k] = Zr[i];
    } else {
      ax.push_back({&Rs[k], c[wk.exp[i]], &Rv[i]});
      Zc[k] = fq_add(Zc[k], fq_mul(c[wk.exp[i]], Zr[i]));
    }
  }
  axpy_pool(ax);
  // every distinct point's L.Z bound up front, in one pool burst
  std::vector<std::pair<const FqV*, const FqV*>> bj;
  for (const FqV& L : Ls) bj.push_back({&Z, &L});
  return prove_slots(ctx, g, host_bounds(bj), Rs, Zc, t, tape, w);
}

int prove_batched_instances(spg_ctx* ctx, ProverGens& g, const std::vector<const FqV*>& polys,
                            const std::vector<FqV>& r_list, const FqV& Zr, Tr& t, Tape& tape, Writer& w) {
  t.protocol("polynomial evaluation proof");
  const Fq c_base = t.challenge("challenge_c");
  // every polynomial's eq factors, then all L.Z bounds in one pool burst
  const size_t n = polys.size();
  std::vector<FqV> r(n), Lv(n), Rv(n);
  std::vector<std::pair<const FqV*, const FqV*>> bj;
  for (size_t i = 0; i < n; i++) {
    r[i] = pe_fit(r_list[i], lg2(polys[i]->size()));
    pe_eq_halves(r[i], &Lv[i], &Rv[i]);
    bj.push_back({polys[i], &Lv[i]});
  }
  std::vector<FqV> LZall = host_bounds(bj);
  const PeWalk wk = pe_walk_instances(r);
  const FqV c = pe_coeff_powers(c_base, wk.repeats());
  const size_t D = wk.first.size();
  std::vector<FqV> LZs(D), Rs(D);
  FqV Zc(D);
  std::vector<Axpy> ax;  // LZs[k] += c LZ_i
  for (size_t i = 0; i < n; i++) {
    const size_t k = wk.group[i];
    if (wk.opens(i)) {
      LZs[k] = LZall[i], Rs[k] = Rv[i], Zc[k] = Zr[i];
    } else {
      ax.push_back({&LZs[k], c[wk.exp[i]], &LZall[i]});
      Zc[k] = fq_add(Zc[k], fq_mul(c[wk.exp[i]], Zr[i]));
    }
  }
  axpy_pool(ax);
  return prove_slots(ctx, g, LZs, Rs, Zc, t, tape, w);
}

static std::vector<size_t> nvs_of(const std::vector<const FqV*>& polys) {
  std::vector<size_t> nv;
  for (const FqV* p : polys) nv.push_back(lg2(p->size()));
  return nv;
}
std::vector<FqV> uni_bounds(const std::vector<const FqV*>& polys, const Fq& r) {
  const PeUniL u = pe_uni_Ls(r, nvs_of(polys));
  std::vector<std::pair<const FqV*, const FqV*>> bj;
  for (size_t i = 0; i < polys.size(); i++) bj.push_back({polys[i], &u.L[u.of[i]]});
  return host_bounds(bj);
}

int prove_uni_batched(spg_ctx* ctx, ProverGens& g, const std::vector<const FqV*>& polys, const std::vector<FqV>& LZs,
                      const Fq& r, const FqV& Zr, Tr& t, Tape& tape, Writer& w) {
  t.protocol("polynomial evaluation proof");
  size_t max_nv = 0;
  for (size_t nv : nvs_of(polys)) max_nv = std::max(max_nv, nv);
  const FqV R = pe_uni_R(r, max_nv);
  Fq c_base = t.challenge("challenge_c"), c = fq_one();
  FqV LZc(R.size(), fq_zero());
  Fq Zrc = fq_zero();
  std::vector<Axpy> ax;
  for (size_t i = 0; i < polys.size(); i++) {  // no grouping in this form: c advances after every term
    ax.push_back({&LZc, c, &LZs[i]});
    Zrc = fq_add(Zrc, fq_mul(c, Zr[i]));
    c = fq_mul(c, c_base);
  }
  axpy_pool(ax);
  DotProductProofLogP p;
  Pt cy;
  int rc = dotproduct_log_prove(ctx, g, t, tape, LZc, fq_zero(), R, Zrc, fq_zero(), &p, &cy);
  if (rc) return rc;
  p.ser(w);
  return 0;
}

static std::vector<Pt> ldpts(const uint8_t* p, size_t n) {
  std::vector<Pt> v(n);
  for (size_t i = 0; i < n; i++) memcpy(v[i].b, p + 32 * i, 32);
  return v;
}

}  // namespace spg

using namespace spg;

extern "C" int spg_poly_gens_new(spg_ctx* ctx, const uint8_t* label, size_t label_len, size_t num_vars,
                                 spg_poly_gens** out) {
  if (!ctx || !label || !out) return SPG_E_ARG;
  if (!nv_ok(num_vars)) return set_err(ctx, SPG_E_ARG, "poly gens: num_vars must be 1 .. 30");
  const size_t n = rs_of(num_vars);
  spg_gens* dev = nullptr;
  const int rc = spg_gens_derive(ctx, label, label_len, n + 1, &dev);  // G_0 .. G_n, then h
  if (rc) return rc;
  spg_poly_gens* pg = new spg_poly_gens();
  pg->g = gens_view(dev, num_vars);
  for (size_t i : {n, n + 1}) pg->g.host.get(i);  // gens_1 and h: the host tables of every proof's Cy and beta
  *out = pg;
  return SPG_OK;
}
extern "C" size_t spg_poly_gens_n(const spg_poly_gens* g) { return g ? g->g.n_pc : 0; }
extern "C" int spg_poly_gens_download(spg_ctx* ctx, const spg_poly_gens* g, uint8_t* out) {
  if (!ctx || !g || !out) return SPG_E_ARG;
  memcpy(out, g->g.dev->compressed, 32 * (g->g.n_pc + 2));
  return SPG_OK;
}
extern "C" int spg_poly_gens_free(spg_ctx* ctx, spg_poly_gens* g) {
  if (!g) return SPG_OK;
  spg_gens_free(ctx, g->g.dev);
  delete g;
  return SPG_OK;
}

extern "C" int spg_poly_commit(spg_ctx* ctx, const spg_poly_gens* g, const spg_buf* Z, size_t offset, size_t num_vars,
                               const uint64_t* blinds_mont, uint8_t* comm, size_t comm_cap, size_t* L_out) {
  HostPin pin;
  return commit_impl(ctx, g, Z, offset, num_vars, blinds_mont, comm, comm_cap, L_out);
}

extern "C" int spg_poly_eval_prove(spg_ctx* ctx, const spg_poly_gens* g, const spg_buf* Z, size_t offset,
                                   const uint64_t* r_mont, size_t num_vars, const uint64_t* Zr_mont,
                                   const uint64_t* blinds_mont, const uint64_t* blind_Zr_mont, spg_transcript* t,
                                   spg_random_tape* tape, uint8_t* proof, size_t cap, size_t* len, uint8_t C_Zr[32]) {
  if (!ctx || !t) return SPG_E_ARG;
  HostPin pin;
  return tr_status(ctx, t->t, prove_impl(ctx, g, Z, offset, r_mont, num_vars, Zr_mont, blinds_mont, blind_Zr_mont, t,
                                         tape, proof, cap, len, C_Zr));
}
extern "C" int spg_poly_eval_prove_batched_points(spg_ctx* ctx, const spg_poly_gens* g, const spg_buf* Z, size_t offset,
                                                  size_t num_vars, const uint64_t* r_list_mont, size_t K,
                                                  const uint64_t* Zr_list_mont, spg_transcript* t,
                                                  spg_random_tape* tape, uint8_t* proof, size_t cap, size_t* len) {
  if (!ctx || !t) return SPG_E_ARG;
  HostPin pin;
  return tr_status(ctx, t->t, prove_points_impl(ctx, g, Z, offset, num_vars, r_list_mont, K, Zr_list_mont, t, tape,
                                                proof, cap, len));
}
extern "C" int spg_poly_eval_prove_batched_instances(spg_ctx* ctx, const spg_poly_gens* g, const spg_buf* const* polys,
                                                     const size_t* offsets, const size_t* num_vars_list, size_t n,
                                                     const uint64_t* r_list_mont, const size_t* r_lens,
                                                     const uint64_t* Zr_list_mont, spg_transcript* t,
                                                     spg_random_tape* tape, uint8_t* proof, size_t cap, size_t* len) {
  if (!ctx || !t) return SPG_E_ARG;
  HostPin pin;
  return tr_status(ctx, t->t, prove_instances_impl(ctx, g, polys, offsets, num_vars_list, n, r_list_mont, r_lens,
                                                   Zr_list_mont, t, tape, proof, cap, len));
}

// ---- verifiers: the Verifier members of verify.hip behind pe_verify.hpp
static int verify_one(spg_ctx* ctx, const spg_poly_gens* g, const uint64_t* r_mont, size_t nv, const uint8_t* C_Zr,
                      const uint64_t* Zr, const uint8_t* comm, size_t L, spg_transcript* t, const uint8_t* proof,
                      size_t proof_len) {
  if (!g || !r_mont || (!C_Zr && !Zr) || !comm || !proof) return SPG_E_ARG;
  if (!nv_ok(nv)) return set_err(ctx, SPG_E_ARG, "poly eval verify: num_vars must be 1 .. 30");
  if (rs_of(nv) > g->g.n_pc) return set_err(ctx, SPG_E_ARG, "poly eval verify: polynomial wider than the generators");
  SPG_HIP(ctx, hipSetDevice(ctx->device));
  Pt cz;
  if (C_Zr) memcpy(cz.b, C_Zr, 32);
  const Fq zr = Zr ? ld_fq(Zr) : fq_zero();
  return pe_verify_one(ctx, const_cast<ProverGens&>(g->g), t->t, lds(r_mont, nv), C_Zr ? &cz : nullptr,
                       Zr ? &zr : nullptr, ldpts(comm, L), proof, proof_len);
}
extern "C" int spg_poly_eval_verify(spg_ctx* ctx, const spg_poly_gens* g, const uint64_t* r_mont, size_t num_vars,
                                    const uint8_t C_Zr[32], const uint8_t* comm, size_t L, spg_transcript* t,
                                    const uint8_t* proof, size_t proof_len) {
  if (!ctx || !t || !C_Zr) return SPG_E_ARG;
  HostPin pin;
  return tr_status(ctx, t->t, verify_one(ctx, g, r_mont, num_vars, C_Zr, nullptr, comm, L, t, proof, proof_len));
}
extern "C" int spg_poly_eval_verify_plain(spg_ctx* ctx, const spg_poly_gens* g, const uint64_t* r_mont, size_t num_vars,
                                          const uint64_t* Zr_mont, const uint8_t* comm, size_t L, spg_transcript* t,
                                          const uint8_t* proof, size_t proof_len) {
  if (!ctx || !t || !Zr_mont) return SPG_E_ARG;
  HostPin pin;
  return tr_status(ctx, t->t, verify_one(ctx, g, r_mont, num_vars, nullptr, Zr_mont, comm, L, t, proof, proof_len));
}
extern "C" int spg_poly_eval_verify_plain_batched_points(spg_ctx* ctx, const spg_poly_gens* g, size_t num_vars,
                                                         const uint64_t* r_list_mont, size_t K,
                                                         const uint64_t* Zr_list_mont, const uint8_t* comm, size_t L,
                                                         spg_transcript* t, const uint8_t* proof, size_t proof_len) {
  if (!ctx || !t || !g || !r_list_mont || !Zr_list_mont || !comm || !proof || K == 0) return SPG_E_ARG;
  if (!nv_ok(num_vars)) return set_err(ctx, SPG_E_ARG, "poly eval verify (points): num_vars must be 1 .. 30");
  if (rs_of(num_vars) > g->g.n_pc)
    return set_err(ctx, SPG_E_ARG, "poly eval verify (points): polynomial wider than the generators");
  SPG_HIP(ctx, hipSetDevice(ctx->device));
  HostPin pin;
  std::vector<FqV> rl(K);
  for (size_t i = 0; i < K; i++) rl[i] = lds(r_list_mont + 4 * i * num_vars, num_vars);
  return tr_status(ctx, t->t, pe_verify_points(ctx, const_cast<ProverGens&>(g->g), t->t, rl, lds(Zr_list_mont, K),
                                               ldpts(comm, L), proof, proof_len));
}
extern "C" int spg_poly_eval_verify_plain_batched_instances(spg_ctx* ctx, const spg_poly_gens* g,
                                                            const uint64_t* r_list_mont, const size_t* r_lens,
                                                            const uint64_t* Zr_list_mont, const uint8_t* comms,
                                                            const size_t* comm_lens, const size_t* num_vars_list,
                                                            size_t n, spg_transcript* t, const uint8_t* proof,
                                                            size_t proof_len) {
  if (!ctx || !t || !g || !r_list_mont || !r_lens || !Zr_list_mont || !comms || !comm_lens || !num_vars_list ||
      !proof || n == 0)
    return SPG_E_ARG;
  size_t tot_r = 0;
  const int rc = instances_args(ctx, g, num_vars_list, r_lens, n, &tot_r, "poly eval verify (instances)");
  if (rc) return rc;
  SPG_HIP(ctx, hipSetDevice(ctx->device));
  HostPin pin;
  std::vector<FqV> rl(n);
  std::vector<std::vector<Pt>> cl(n);
  size_t ro = 0, co = 0;
  for (size_t i = 0; i < n; ro += r_lens[i], co += comm_lens[i], i++) {
    rl[i] = lds(r_list_mont + 4 * ro, r_lens[i]);
    cl[i] = ldpts(comms + 32 * co, comm_lens[i]);
  }
  return tr_status(ctx, t->t,
                   pe_verify_instances(ctx, const_cast<ProverGens&>(g->g), t->t, rl, lds(Zr_list_mont, n), cl,
                                       std::vector<size_t>(num_vars_list, num_vars_list + n), proof, proof_len));
}

// ---- the disjoint-rounds and univariate forms (spg_pe_*)
extern "C" int spg_pe_prove_disjoint(spg_ctx* ctx, const spg_poly_gens* g, const spg_buf* const* polys,
                                     const size_t* offsets, const size_t* num_proofs_list,
                                     const size_t* num_inputs_list, size_t n, const uint64_t* rq_mont, size_t rq_len,
                                     const uint64_t* ry_mont, size_t ry_len, const uint64_t* Zr_list_mont,
                                     spg_transcript* t, spg_random_tape* tape, uint8_t* proof, size_t cap,
                                     size_t* len) {
  if (!ctx || !t) return SPG_E_ARG;
  HostPin pin;
  return tr_status(ctx, t->t, prove_disjoint_impl(ctx, g, polys, offsets, num_proofs_list, num_inputs_list, n, rq_mont,
                                                  rq_len, ry_mont, ry_len, Zr_list_mont, t, tape, proof, cap, len));
}
// rows and evaluation commitments of n polynomials, as the verifiers take them
static void ld_comms(const uint8_t* C_Zr_list, const uint8_t* comms, const size_t* comm_lens, size_t n,
                     std::vector<Pt>* cz, std::vector<std::vector<Pt>>* cl) {
  *cz = ldpts(C_Zr_list, n);
  cl->resize(n);
  for (size_t i = 0, co = 0; i < n; co += comm_lens[i], i++) (*cl)[i] = ldpts(comms + 32 * co, comm_lens[i]);
}
extern "C" int spg_pe_verify_disjoint(spg_ctx* ctx, const spg_poly_gens* g, const size_t* num_proofs_list,
                                      const size_t* num_inputs_list, size_t n, const uint64_t* rq_mont, size_t rq_len,
                                      const uint64_t* ry_mont, size_t ry_len, const uint8_t* C_Zr_list,
                                      const uint8_t* comms, const size_t* comm_lens, spg_transcript* t,
                                      const uint8_t* proof, size_t proof_len) {
  if (!ctx || !t || !g || !num_proofs_list || !num_inputs_list || !rq_mont || !ry_mont || !C_Zr_list || !comms ||
      !comm_lens || !proof || n == 0)
    return SPG_E_ARG;
  const int rc = disjoint_args(ctx, g, num_proofs_list, num_inputs_list, n, rq_len, "poly eval verify (disjoint)");
  if (rc) return rc;
  SPG_HIP(ctx, hipSetDevice(ctx->device));
  HostPin pin;
  std::vector<Pt> cz;
  std::vector<std::vector<Pt>> cl;
  ld_comms(C_Zr_list, comms, comm_lens, n, &cz, &cl);
  return tr_status(ctx, t->t,
                   pe_verify_disjoint(ctx, const_cast<ProverGens&>(g->g), t->t,
                                      std::vector<size_t>(num_proofs_list, num_proofs_list + n),
                                      std::vector<size_t>(num_inputs_list, num_inputs_list + n), lds(rq_mont, rq_len),
                                      lds(ry_mont, ry_len), cz, cl, proof, proof_len));
}
extern "C" int spg_pe_uni_evals(spg_ctx* ctx, const spg_buf* const* polys, const size_t* offsets,
                                const size_t* num_vars_list, size_t n, const uint64_t* r_mont, uint64_t* Zr_out_mont) {
  if (!ctx) return SPG_E_ARG;
  HostPin pin;
  return uni_evals_impl(ctx, polys, offsets, num_vars_list, n, r_mont, Zr_out_mont);
}
extern "C" int spg_pe_prove_uni(spg_ctx* ctx, const spg_poly_gens* g, const spg_buf* const* polys,
                                const size_t* offsets, const size_t* num_vars_list, size_t n, const uint64_t* r_mont,
                                const uint64_t* Zr_list_mont, spg_transcript* t, spg_random_tape* tape, uint8_t* proof,
                                size_t cap, size_t* len, uint8_t C_Zr[32]) {
  if (!ctx || !t) return SPG_E_ARG;
  HostPin pin;
  return tr_status(ctx, t->t, prove_uni_impl(ctx, g, polys, offsets, num_vars_list, n, r_mont, Zr_list_mont, t, tape,
                                             proof, cap, len, C_Zr));
}
extern "C" int spg_pe_verify_uni(spg_ctx* ctx, const spg_poly_gens* g, const uint64_t* r_mont,
                                 const uint8_t* C_Zr_list, const uint8_t* comms, const size_t* comm_lens,
                                 const size_t* poly_sizes, size_t n, spg_transcript* t, const uint8_t* proof,
                                 size_t proof_len) {
  if (!ctx || !t || !g || !r_mont || !C_Zr_list || !comms || !comm_lens || !poly_sizes || !proof || n == 0)
    return SPG_E_ARG;
  size_t max_nv = 0;
  for (size_t i = 0; i < n; i++) {  // nv_i = lg next_pow2(size_i), as the reference reads them
    const size_t nv = poly_sizes[i] > ((size_t)1 << kPeMaxVars) ? kPeMaxVars + 1 : lg2(npow2(poly_sizes[i]));
    if (!nv_ok(nv)) return set_err(ctx, SPG_E_ARG, "poly eval verify (uni): num_vars must be 1 .. 30");
    max_nv = std::max(max_nv, nv);
  }
  if (rs_of(max_nv) > g->g.n_pc)
    return set_err(ctx, SPG_E_ARG, "poly eval verify (uni): polynomial wider than the generators");
  SPG_HIP(ctx, hipSetDevice(ctx->device));
  HostPin pin;
  std::vector<Pt> cz;
  std::vector<std::vector<Pt>> cl;
  ld_comms(C_Zr_list, comms, comm_lens, n, &cz, &cl);
  return tr_status(ctx, t->t,
                   pe_verify_uni(ctx, const_cast<ProverGens&>(g->g), t->t, ld_fq(r_mont), cz, cl,
                                 std::vector<size_t>(poly_sizes, poly_sizes + n), proof, proof_len));
}
