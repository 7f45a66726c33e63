// TEST HELPER — never linked into the product. The pieces of the CPU oracle's R1CSProof::prove (oracle/r1cs.hpp,
// oracle/sumcheck.hpp, oracle/poly.hpp as they stand) that pyoracle does not expose one by one, behind a C interface,
// for tests/test_r1cs_seams_oracle.py and tests/test_gpu_r1cs_seams.py. These are the very functions R1CSProof::prove
// calls, so the whole-proof goldens pin them. Scalars cross as four Montgomery u64 limbs, vectors as n x 4 limbs; a
// DensePolynomialPqx crosses flat in its allocation layout: instance p's num_proofs[p] x nws x num_inputs[p] scalars
// row-major, instances one after another.
#include <string.h>

#include <string>
#include <vector>

#include "../../include/spg.h"
#include "../../oracle/r1cs.hpp"

using namespace orc;

namespace {
Fq ld(const uint64_t* p) {
  Fq a;
  memcpy(a.v, p, 32);
  return a;
}
void st(uint64_t* p, const Fq& a) { memcpy(p, a.v, 32); }
FqVec ldv(const uint64_t* p, size_t n) {
  FqVec v(n);
  for (size_t i = 0; i < n; i++) v[i] = ld(p + 4 * i);
  return v;
}
void stv(uint64_t* p, const FqVec& v) {
  for (size_t i = 0; i < v.size(); i++) st(p + 4 * i, v[i]);
}

struct Shape {
  size_t P, max_np, nws, max_ni;
  std::vector<size_t> np, ni;
  Shape(size_t P_, const size_t* np_, size_t max_np_, size_t nws_, const size_t* ni_, size_t max_ni_)
      : P(P_), max_np(max_np_), nws(nws_), max_ni(max_ni_), np(np_, np_ + P_), ni(ni_, ni_ + P_) {}
};
// the nested vectors of a table (or of a z_mat in (p, q, w, x) order: the same nesting) from its flat form
Mat4 mat4(const uint64_t* z, const Shape& s) {
  Mat4 m(s.P);
  for (size_t p = 0; p < s.P; p++) {
    m[p].assign(s.np[p], std::vector<FqVec>(s.nws, FqVec(s.ni[p])));
    for (size_t q = 0; q < s.np[p]; q++)
      for (size_t w = 0; w < s.nws; w++)
        for (size_t x = 0; x < s.ni[p]; x++, z += 4) m[p][q][w][x] = ld(z);
  }
  return m;
}
// DensePolynomialPqx::new (custom_dense_mlpoly.rs:45-64)
Pqx pqx_new(const uint64_t* z, const Shape& s) {
  Pqx T;
  T.Z = mat4(z, s);
  T.num_instances = next_pow2(s.P);
  T.num_proofs = s.np;
  T.max_num_proofs = s.max_np;
  T.num_witness_secs = next_pow2(s.nws);
  T.num_inputs = s.ni;
  T.max_num_inputs = s.max_ni;
  return T;
}
// every allocated entry (the nested vectors never shrink), then the size fields: num_instances, max_num_proofs,
// num_witness_secs, max_num_inputs, num_proofs[0..P), num_inputs[0..P)
void pqx_out(const Pqx& T, uint64_t* out, size_t* sizes) {
  for (auto& ip : T.Z)
    for (auto& q : ip)
      for (auto& w : q)
        for (auto& x : w) {
          st(out, x);
          out += 4;
        }
  if (!sizes) return;
  sizes[0] = T.num_instances;
  sizes[1] = T.max_num_proofs;
  sizes[2] = T.num_witness_secs;
  sizes[3] = T.max_num_inputs;
  const size_t P = T.Z.size();
  for (size_t p = 0; p < P; p++) {
    sizes[4 + p] = T.num_proofs[p];
    sizes[4 + P + p] = T.num_inputs[p];
  }
}

R1CSInstance inst_from_c(const spg_r1cs_instance* ci) {
  std::vector<std::vector<SparseEntry>> A, B, C;
  for (size_t p = 0; p < ci->num_instances; p++)
    for (int m = 0; m < 3; m++) {
      std::vector<SparseEntry> v;
      const spg_sparse_entry* e = ci->entries[3 * p + m];
      for (size_t k = 0; k < ci->nnz[3 * p + m]; k++) {
        SparseEntry s;
        s.row = e[k].row;
        s.col = e[k].col;
        memcpy(s.val.v, e[k].val, 32);
        v.push_back(s);
      }
      (m == 0 ? A : m == 1 ? B : C).push_back(v);
    }
  std::vector<size_t> nc(ci->num_cons, ci->num_cons + ci->num_instances);
  return R1CSInstance::create(ci->num_instances, ci->max_num_cons, nc, ci->num_vars, A, B, C);
}

// evals_ABC of R1CSProof::prove (oracle/r1cs.hpp, r1csproof.rs:430-465) and its new_rev
Pqx abc_poly(const R1CSInstance& inst, size_t num_instances, size_t nws, size_t max_ni, const std::vector<size_t>& ni,
             const FqVec& evals_rx, const Fq& r_A, const Fq& r_B, const Fq& r_C) {
  Mat4 evals_ABC(inst.num_instances);
  for (size_t p = 0; p < inst.num_instances; p++) {
    auto eA = inst.A[p].eval_table_disjoint_rounds(evals_rx, nws, max_ni, ni[p]);
    auto eB = inst.B[p].eval_table_disjoint_rounds(evals_rx, nws, max_ni, ni[p]);
    auto eC = inst.C[p].eval_table_disjoint_rounds(evals_rx, nws, max_ni, ni[p]);
    evals_ABC[p].push_back(std::vector<FqVec>());
    for (size_t w = 0; w < nws; w++) {
      FqVec row;
      for (size_t i = 0; i < ni[p]; i++)
        row.push_back(fq_add(fq_add(fq_mul(r_A, eA[w][i]), fq_mul(r_B, eB[w][i])), fq_mul(r_C, eC[w][i])));
      evals_ABC[p][0].push_back(row);
    }
  }
  return Pqx::new_rev(evals_ABC, std::vector<size_t>(num_instances, 1), 1, ni, max_ni);
}

void ser_out(const ZKSumcheckProof& pf, uint8_t* proof, size_t cap, size_t* len) {
  Ser s;
  pf.ser(s);
  *len = s.b.size();
  if (s.b.size() > cap) throw std::string("proof buffer too small");
  memcpy(proof, s.b.data(), s.b.size());
}

// bincode(ZKSumcheckInstanceProof): false on truncated, trailing or oversized input and on a scalar that is not
// reduced (serde's Scalar reads four limbs; the product rejects limbs >= q as malformed, so does this reader)
struct Rd {
  const uint8_t* p;
  size_t n, o = 0;
  bool bad = false;
  bool take(size_t k) {
    if (bad || k > n - o) bad = true;
    return !bad;
  }
  uint64_t u64() {
    if (!take(8)) return 0;
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v |= (uint64_t)p[o + i] << (8 * i);
    o += 8;
    return v;
  }
  size_t len(size_t elem) {
    const uint64_t v = u64();
    if (bad || v > (n - o) / elem) {
      bad = true;
      return 0;
    }
    return (size_t)v;
  }
  CPt pt() {
    CPt c;
    memset(c.v, 0, 32);
    if (!take(32)) return c;
    memcpy(c.v, p + o, 32);
    o += 32;
    return c;
  }
  Fq sc() {
    Fq a = fq_zero();
    if (!take(32)) return a;
    for (int i = 0; i < 4; i++) {
      uint64_t v = 0;
      for (int k = 0; k < 8; k++) v |= (uint64_t)p[o + 8 * i + k] << (8 * k);
      a.v[i] = v;
    }
    o += 32;
    // reduced: a + 0 == a limb for limb only when a < q (fq_add reduces its result)
    const Fq b = fq_add(a, fq_zero());
    if (memcmp(a.v, b.v, 32) != 0) bad = true;
    return a;
  }
};
bool read_zk(const uint8_t* proof, size_t len, ZKSumcheckProof* out) {
  Rd r{proof, len};
  const size_t a = r.len(32);
  for (size_t i = 0; i < a; i++) out->comm_polys.push_back(r.pt());
  const size_t b = r.len(32);
  for (size_t i = 0; i < b; i++) out->comm_evals.push_back(r.pt());
  const size_t c = r.len(96);
  for (size_t i = 0; i < c && !r.bad; i++) {
    DotProductProof d;
    d.delta = r.pt();
    d.beta = r.pt();
    const size_t k = r.len(32);
    for (size_t j = 0; j < k; j++) d.z.push_back(r.sc());
    d.z_delta = r.sc();
    d.z_beta = r.sc();
    out->proofs.push_back(d);
  }
  return !r.bad && r.o == r.n;
}

void tail_out(Transcript& t, RandomTape& tape, uint8_t* check, uint64_t* tape_next) {
  t.challenge_bytes("seam_check", check, 64);
  st(tape_next, tape.random_scalar("seam_next"));
}
}  // namespace

extern "C" {

// Pqx::new_rev of z in (p, q, w, x) order
int rs_new_rev(const uint64_t* z, size_t P, const size_t* num_proofs, size_t max_np, size_t nws,
               const size_t* num_inputs, size_t max_ni, uint64_t* out, size_t* sizes) {
  const Shape s(P, num_proofs, max_np, nws, num_inputs, max_ni);
  pqx_out(Pqx::new_rev(mat4(z, s), s.np, max_np, s.ni, max_ni), out, sizes);
  return 0;
}

// SparseMat::eval_table_disjoint_rounds of A_p, B_p, C_p for every matrix instance of ci (r1csinstance.rs:484-534):
// out[m] receives [p][w][i], p < ci->num_instances, w < nws, i < num_inputs[p]. -2 where the reference would panic.
int rs_eval_tables(const spg_r1cs_instance* ci, size_t nws, size_t max_ni, const size_t* num_inputs,
                   const uint64_t* evals_rx, size_t n_rx, uint64_t* outA, uint64_t* outB, uint64_t* outC) {
  try {
    const R1CSInstance inst = inst_from_c(ci);
    const FqVec rx = ldv(evals_rx, n_rx);
    uint64_t* outs[3] = {outA, outB, outC};
    size_t o = 0;
    for (size_t p = 0; p < inst.num_instances; p++) {
      const SparseMat* M[3] = {&inst.A[p], &inst.B[p], &inst.C[p]};
      for (int m = 0; m < 3; m++) {
        const auto e = M[m]->eval_table_disjoint_rounds(rx, nws, max_ni, num_inputs[p]);
        for (size_t w = 0; w < nws; w++) stv(outs[m] + 4 * (o + w * num_inputs[p]), e[w]);
      }
      o += nws * num_inputs[p];
    }
    return 0;
  } catch (const std::string&) {
    return -2;
  }
}

// evals_ABC (r_A A + r_B B + r_C C) through new_rev, flat
int rs_abc_poly(const spg_r1cs_instance* ci, size_t num_instances, size_t nws, size_t max_ni, const size_t* num_inputs,
                const uint64_t* evals_rx, size_t n_rx, const uint64_t* rA, const uint64_t* rB, const uint64_t* rC,
                uint64_t* out, size_t* sizes) {
  try {
    const R1CSInstance inst = inst_from_c(ci);
    const std::vector<size_t> ni(num_inputs, num_inputs + num_instances);
    pqx_out(abc_poly(inst, num_instances, nws, max_ni, ni, ldv(evals_rx, n_rx), ld(rA), ld(rB), ld(rC)), out, sizes);
    return 0;
  } catch (const std::string&) {
    return -2;
  }
}

// x.commit(blind, gens_1) of R1CSGens(gens_label, gens_nv): the comm_claim a ZK sumcheck verifier starts from
int rs_commit1(const char* gens_label, size_t gens_nv, const uint64_t* x, const uint64_t* blind, uint8_t* out) {
  const R1CSGens g = R1CSGens::create(gens_label, gens_nv);
  const CPt c = cpt(commit1(ld(x), ld(blind), g.gens_1));
  memcpy(out, c.v, 32);
  return 0;
}

// phase1_round_evals (oracle/sumcheck.hpp:118) on the tables' current state: B, C, D flat with their allocation shape
// (alloc_np, alloc_ni; one section) and current sizes (cur: num_instances, then num_proofs[P], num_inputs[P]);
// num_proofs / num_cons: the round's local sizes (already halved)
int rs_phase1_round(int mode, size_t instance_len, size_t proof_len, size_t cons_len, size_t P, const size_t* alloc_np,
                    const size_t* alloc_ni, const size_t* cur, const size_t* num_proofs, const size_t* num_cons,
                    const uint64_t* Ap, size_t nAp, const uint64_t* Aq, size_t nAq, const uint64_t* Ax, size_t nAx,
                    const uint64_t* B, const uint64_t* C, const uint64_t* D, uint64_t* out3) {
  const Shape s(P, alloc_np, 1, 1, alloc_ni, 1);
  Pqx T[3] = {pqx_new(B, s), pqx_new(C, s), pqx_new(D, s)};
  for (Pqx& t : T) {
    t.num_instances = cur[0];
    t.num_proofs.assign(cur + 1, cur + 1 + P);
    t.num_inputs.assign(cur + 1 + P, cur + 1 + 2 * P);
  }
  Fq e0, e2, e3;
  phase1_round_evals(mode, instance_len, proof_len, cons_len, std::vector<size_t>(num_proofs, num_proofs + P),
                     std::vector<size_t>(num_cons, num_cons + P), DensePoly(ldv(Ap, nAp)), DensePoly(ldv(Aq, nAq)),
                     DensePoly(ldv(Ax, nAx)), T[0], T[1], T[2], &e0, &e2, &e3);
  st(out3, e0);
  st(out3 + 4, e2);
  st(out3 + 8, e3);
  return 0;
}

// prove_phase1 (oracle/sumcheck.hpp:150) on a fresh Transcript(tr_label) and RandomTape("proof", tape_seed): Ap, Aq,
// Ax of 2^np, 2^nq, 2^nx scalars; B, C, D flat tables of shape (P, num_proofs, 2^nq, one section, num_cons, 2^nx).
// Outputs: the proof, r (rounds), claims (4), the last blind, the bound tables (flat) with B's sizes, the bound eq
// vectors' first entries eq3, 64 bytes of challenge_bytes("seam_check") and the tape's next scalar ("seam_next").
int rs_phase1(const char* gens_label, size_t gens_nv, const char* tr_label, const uint64_t* tape_seed, size_t nx,
              size_t nq, size_t np, const uint64_t* Ap, const uint64_t* Aq, const uint64_t* Ax, size_t P,
              const size_t* num_proofs, const size_t* num_cons, const uint64_t* B, const uint64_t* C,
              const uint64_t* D, uint8_t* proof, size_t cap, size_t* len, uint64_t* r, uint64_t* claims,
              uint64_t* blind, uint64_t* Bo, uint64_t* Co, uint64_t* Do, size_t* sizes, uint64_t* eq3, uint8_t* check,
              uint64_t* tape_next) {
  try {
    const R1CSGens g = R1CSGens::create(gens_label, gens_nv);
    Transcript t(tr_label);
    RandomTape tape("proof", ld(tape_seed));
    const Shape s(P, num_proofs, pow2(nq), 1, num_cons, pow2(nx));
    Pqx Bt = pqx_new(B, s), Ct = pqx_new(C, s), Dt = pqx_new(D, s);
    DensePoly ap(ldv(Ap, pow2(np))), aq(ldv(Aq, pow2(nq))), ax(ldv(Ax, pow2(nx)));
    FqVec rr, cl;
    Fq bl;
    const ZKSumcheckProof pf = prove_phase1(nx + nq + np, nx, nq, np, s.np, s.ni, ap, aq, ax, Bt, Ct, Dt, g.gens_1,
                                            g.gens_4, t, tape, &rr, &cl, &bl);
    ser_out(pf, proof, cap, len);
    stv(r, rr);
    stv(claims, cl);
    st(blind, bl);
    pqx_out(Bt, Bo, sizes);
    pqx_out(Ct, Co, nullptr);
    pqx_out(Dt, Do, nullptr);
    st(eq3, ap[0]);
    st(eq3 + 4, aq[0]);
    st(eq3 + 8, ax[0]);
    tail_out(t, tape, check, tape_next);
    return 0;
  } catch (const std::string&) {
    return -2;
  }
}

// prove_phase2 (oracle/sumcheck.hpp:219) on a fresh transcript and tape: eq of 2^np scalars; ABC flat, one proof row,
// Pa instances of num_inputs_abc widths in new_rev order; Z = new_rev(z) of shape (P, num_proofs, max_np, nws,
// num_inputs, 2^ny) bound at rq (n_rq challenges, bound_vars_rq). Outputs as rs_phase1, with the bound ABC and Z.
int rs_phase2(const char* gens_label, size_t gens_nv, const char* tr_label, const uint64_t* tape_seed,
              const uint64_t* claim, const uint64_t* blind_claim, size_t ny, size_t nw, size_t np, int single,
              size_t nws, const uint64_t* eq, size_t Pa, const size_t* num_inputs_abc, const uint64_t* ABC, size_t P,
              const size_t* num_proofs, size_t max_np, const size_t* num_inputs, const uint64_t* z, const uint64_t* rq,
              size_t n_rq, uint8_t* proof, size_t cap, size_t* len, uint64_t* r, uint64_t* claims, uint64_t* blind,
              uint64_t* ABCo, size_t* sizes_abc, uint64_t* Zo, size_t* sizes_z, uint64_t* eq0, uint8_t* check,
              uint64_t* tape_next) {
  try {
    const R1CSGens g = R1CSGens::create(gens_label, gens_nv);
    Transcript t(tr_label);
    RandomTape tape("proof", ld(tape_seed));
    const std::vector<size_t> ones(Pa, 1);
    const Shape sa(Pa, ones.data(), 1, nws, num_inputs_abc, pow2(ny));
    Pqx At = pqx_new(ABC, sa);
    const Shape sz(P, num_proofs, max_np, nws, num_inputs, pow2(ny));
    Pqx Zt = Pqx::new_rev(mat4(z, sz), sz.np, max_np, sz.ni, sz.max_ni);
    Zt.bound_vars_rq(ldv(rq, n_rq));
    DensePoly e(ldv(eq, pow2(np)));
    FqVec rr, cl;
    Fq bl;
    const ZKSumcheckProof pf = prove_phase2(ld(claim), ld(blind_claim), ny + nw + np, ny, nw, np, single != 0, nws,
                                            sz.ni, e, At, Zt, g.gens_1, g.gens_4, t, tape, &rr, &cl, &bl);
    ser_out(pf, proof, cap, len);
    stv(r, rr);
    stv(claims, cl);
    st(blind, bl);
    pqx_out(At, ABCo, sizes_abc);
    pqx_out(Zt, Zo, sizes_z);
    st(eq0, e[0]);
    tail_out(t, tape, check, tape_next);
    return 0;
  } catch (const std::string&) {
    return -2;
  }
}

// ZKSumcheckProof::verify (oracle/sumcheck.hpp:50) of proof bytes on a fresh Transcript(tr_label): 1 accepted (post,
// r and the 64-byte transcript check are written), 0 rejected -- malformed bytes, a wrong round count and a point
// that does not decompress included
int rs_verify(const char* gens_label, size_t gens_nv, const char* tr_label, const uint8_t* comm_claim, size_t rounds,
              const uint8_t* proof, size_t len, uint8_t* post, uint64_t* r, uint8_t* check) {
  ZKSumcheckProof pf;
  if (!read_zk(proof, len, &pf)) return 0;
  if (pf.proofs.size() != rounds) return 0;  // (the reference zips the three vectors; bincode of a prover has them equal)
  for (const DotProductProof& d : pf.proofs)
    if (d.z.size() != 4) return 0;  // (a cubic's four coefficients: gens_4 has no fifth generator to commit z with)
  try {
    const R1CSGens g = R1CSGens::create(gens_label, gens_nv);
    Transcript t(tr_label);
    CPt cc, fin;
    memcpy(cc.v, comm_claim, 32);
    FqVec rr;
    if (!pf.verify(cc, rounds, 3, g.gens_1, g.gens_4, t, &fin, &rr)) return 0;
    memcpy(post, fin.v, 32);
    stv(r, rr);
    t.challenge_bytes("seam_check", check, 64);
    return 1;
  } catch (const std::string&) {
    return 0;
  }
}

// R1CSProof::prove's body from multiply_vec_block to the end of phase 2 without the sigma proofs between the phases
// (oracle/r1cs.hpp:266-342), on a fresh Transcript(tr_label) and RandomTape("proof", tape_seed): tau_p, tau_q, tau_x
// drawn as there; multiply_vec_block; phase 1; r_A, r_B, r_C; the phase-2 claim r_A Az + r_B Bz + r_C Cz with a zero
// blind; eq(rx); evals_ABC and its new_rev; new_rev(z_mat) bound at rq_rev; eq(rp); phase 2.
int rs_chain(const spg_r1cs_instance* ci, size_t P, const size_t* num_proofs, size_t max_np, const size_t* num_inputs,
             size_t max_ni, size_t nws, const uint64_t* z, const char* gens_label, size_t gens_nv, const char* tr_label,
             const uint64_t* tape_seed, uint8_t* proof1, size_t cap1, size_t* len1, uint8_t* proof2, size_t cap2,
             size_t* len2, uint64_t* claims2, uint8_t* check, uint64_t* tape_next) {
  try {
    const R1CSInstance inst = inst_from_c(ci);
    const R1CSGens g = R1CSGens::create(gens_label, gens_nv);
    Transcript t(tr_label);
    RandomTape tape("proof", ld(tape_seed));
    const Shape sz(P, num_proofs, max_np, nws, num_inputs, max_ni);
    const Mat4 z_mat = mat4(z, sz);
    const size_t num_cons = inst.max_num_cons;
    const std::vector<size_t> block_num_cons =
        inst.num_instances == 1 ? std::vector<size_t>(P, inst.num_cons[0]) : inst.num_cons;
    const size_t np = log_2(next_pow2(P)), nq = log_2(max_np), nx = log_2(num_cons), nw = log_2(nws),
                 ny = log_2(max_ni);
    const FqVec tau_p = t.challenge_vector("challenge_tau_p", np);
    const FqVec tau_q = t.challenge_vector("challenge_tau_q", nq);
    const FqVec tau_x = t.challenge_vector("challenge_tau_x", nx);
    DensePoly ptp(eq_evals(tau_p)), ptq(eq_evals(tau_q)), ptx(eq_evals(tau_x));
    Pqx Az, Bz, Cz;
    inst.multiply_vec_block(P, sz.np, max_np, sz.ni, max_ni, num_cons, block_num_cons, z_mat, &Az, &Bz, &Cz);
    FqVec rx_all, claims1;
    Fq blind1;
    const ZKSumcheckProof sc1 = prove_phase1(nx + nq + np, nx, nq, np, sz.np, block_num_cons, ptp, ptq, ptx, Az, Bz,
                                             Cz, g.gens_1, g.gens_4, t, tape, &rx_all, &claims1, &blind1);
    ser_out(sc1, proof1, cap1, len1);
    const FqVec rx_rev(rx_all.begin(), rx_all.begin() + nx), rq_rev(rx_all.begin() + nx, rx_all.begin() + nx + nq),
        rp(rx_all.begin() + nx + nq, rx_all.end());
    const FqVec rx(rx_rev.rbegin(), rx_rev.rend());
    const Fq r_A = t.challenge_scalar("challenge_Az"), r_B = t.challenge_scalar("challenge_Bz"),
             r_C = t.challenge_scalar("challenge_Cz");
    const Fq claim2 = fq_add(fq_add(fq_mul(r_A, claims1[1]), fq_mul(r_B, claims1[2])), fq_mul(r_C, claims1[3]));
    Pqx ABC = abc_poly(inst, P, nws, max_ni, sz.ni, eq_evals(rx), r_A, r_B, r_C);
    Pqx Zp = Pqx::new_rev(z_mat, sz.np, max_np, sz.ni, max_ni);
    Zp.bound_vars_rq(rq_rev);
    DensePoly eq_p(eq_evals(rp));
    FqVec ry_all, cl2;
    Fq blind2;
    const ZKSumcheckProof sc2 = prove_phase2(claim2, fq_zero(), ny + nw + np, ny, nw, np, inst.num_instances == 1, nws,
                                             sz.ni, eq_p, ABC, Zp, g.gens_1, g.gens_4, t, tape, &ry_all, &cl2, &blind2);
    ser_out(sc2, proof2, cap2, len2);
    stv(claims2, cl2);
    tail_out(t, tape, check, tape_next);
    return 0;
  } catch (const std::string&) {
    return -2;
  }
}
}
