// TEST HELPER — never linked into the product. The dense polynomial commitment entries of the CPU oracle
// (oracle/polyeval.hpp, oracle/nizk.hpp as they stand) behind a C interface, for tests/test_polyeval_oracle.py and
// tests/test_gpu_polyeval.py. Scalars cross as four Montgomery u64 limbs, vectors as n x 4 limbs.
//
// Every prove wrapper runs on a fresh Transcript(tlabel) and RandomTape(tape_name, seed) and returns, besides the
// bincode bytes, 64 bytes of challenge_bytes("seam_check") drawn from the transcript afterwards and one more
// random_scalar("seam_check") drawn from the tape afterwards: the positions both were left in.
#include <string.h>

#include <string>
#include <vector>

#include "../../oracle/polyeval.hpp"

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
PolyCommitment ldc(const uint8_t* p, size_t n) {
  PolyCommitment c(n);
  for (size_t i = 0; i < n; i++) memcpy(c[i].v, p + 32 * i, 32);
  return c;
}
// bytes out, the positions of transcript and tape after the prover
int finish(const Ser& s, Transcript& t, RandomTape& tape, uint8_t* proof, size_t cap, size_t* len, uint8_t* check,
           uint64_t* tape_next) {
  *len = s.b.size();
  if (s.b.size() <= cap) memcpy(proof, s.b.data(), s.b.size());
  t.challenge_bytes("seam_check", check, 64);
  st(tape_next, tape.random_scalar("seam_check"));
  return s.b.size() <= cap ? 0 : -2;
}
// the fitted point of prove_batched_instances (dense_mlpoly.rs:712-722)
FqVec fit(const FqVec& r, size_t nv) {
  if (nv >= r.size()) {
    FqVec v(nv - r.size(), fq_zero());
    v.insert(v.end(), r.begin(), r.end());
    return v;
  }
  return FqVec(r.end() - nv, r.end());
}
// the blinded L.Z of PolyEvalProof::prove (dense_mlpoly.rs:466-475)
void blinded_bound(const DensePoly& poly, const FqVec& r, const FqVec* blinds, FqVec* L, FqVec* R, FqVec* LZ,
                   Fq* LZ_blind) {
  eq_factored_evals(r, L, R);
  *LZ = poly.bound(*L);
  *LZ_blind = fq_zero();
  for (size_t i = 0; blinds && i < L->size(); i++) *LZ_blind = fq_add(*LZ_blind, fq_mul((*blinds)[i], (*L)[i]));
}
}  // namespace

extern "C" {

// DensePolynomial::commit_inner (dense_mlpoly.rs:184-212) with PolyCommitmentGens::new(gens_nv, label): the L =
// 2^(nv/2) rows of Z (2^nv scalars) committed as commitv(row, blinds[i], gens_n); blinds NULL = zeros. rows: L x 32
int pe_commit(const char* label, size_t gens_nv, const uint64_t* Z, size_t nv, const uint64_t* blinds, uint8_t* rows) {
  try {
    const DotGens g = poly_commit_gens_new(gens_nv, label);
    const DensePoly poly(ldv(Z, pow2(nv)));
    size_t ln, rn;
    eq_factored_lens(nv, &ln, &rn);
    const size_t L = pow2(ln), R = pow2(rn);
    for (size_t i = 0; i < L; i++) {
      const FqVec row(poly.Z.begin() + R * i, poly.Z.begin() + R * (i + 1));
      const CPt c = cpt(commitv(row, blinds ? ld(blinds + 4 * i) : fq_zero(), g.gens_n));
      memcpy(rows + 32 * i, c.v, 32);
    }
    return 0;
  } catch (const std::string&) {
    return -1;
  }
}

// the blinded bound alone: LZ (2^(nv - nv/2) scalars) and LZ_blind = sum_i blinds[i] L[i]
int pe_bound(const uint64_t* Z, size_t nv, const uint64_t* r, const uint64_t* blinds, uint64_t* LZ_out,
             uint64_t* LZ_blind_out) {
  const DensePoly poly(ldv(Z, pow2(nv)));
  const FqVec bl = blinds ? ldv(blinds, pow2(nv / 2)) : FqVec();
  FqVec L, R, LZ;
  Fq b;
  blinded_bound(poly, ldv(r, nv), blinds ? &bl : nullptr, &L, &R, &LZ, &b);
  stv(LZ_out, LZ);
  st(LZ_blind_out, b);
  return 0;
}

// PolyEvalProof::prove (dense_mlpoly.rs:437-490) with blinds: the oracle's prove has none, so the blinded form is
// composed here from eq_factored_evals, DensePoly::bound, sum blinds[i] L[i] and DotProductProofLog::prove. *verified:
// the oracle's own PolyEvalProof::verify on a fresh Transcript(tlabel) against the blinded commitment of Z and C_Zr;
// with tamper != 0 the proof's z1 has its lowest byte flipped first (in the verified copy only)
int pe_prove(const char* label, size_t gens_nv, const char* tlabel, const char* tape_name, const uint64_t* seed,
             const uint64_t* Z, size_t nv, const uint64_t* r, const uint64_t* Zr, const uint64_t* blinds,
             const uint64_t* blind_Zr, int tamper, uint8_t* proof, size_t cap, size_t* len, uint8_t* C_Zr,
             uint8_t* check, uint64_t* tape_next, int* verified) {
  try {
    const DotGens g = poly_commit_gens_new(gens_nv, label);
    const DensePoly poly(ldv(Z, pow2(nv)));
    const FqVec rv = ldv(r, nv), bl = blinds ? ldv(blinds, pow2(nv / 2)) : FqVec();
    Transcript t(tlabel);
    RandomTape tape(tape_name, ld(seed));
    t.append_protocol_name("polynomial evaluation proof");
    FqVec L, R, LZ;
    Fq LZ_blind;
    blinded_bound(poly, rv, blinds ? &bl : nullptr, &L, &R, &LZ, &LZ_blind);
    CPt cx, cy;
    PolyEvalProof p;
    p.proof = DotProductProofLog::prove(g, t, tape, LZ, LZ_blind, R, ld(Zr), blind_Zr ? ld(blind_Zr) : fq_zero(), &cx,
                                        &cy);
    memcpy(C_Zr, cy.v, 32);
    Ser s;
    p.ser(s);
    const int rc = finish(s, t, tape, proof, cap, len, check, tape_next);
    PolyCommitment comm;
    const size_t Rn = R.size();
    for (size_t i = 0; i < L.size(); i++) {
      const FqVec row(poly.Z.begin() + Rn * i, poly.Z.begin() + Rn * (i + 1));
      comm.push_back(cpt(commitv(row, blinds ? bl[i] : fq_zero(), g.gens_n)));
    }
    if (tamper) p.proof.z1.v[0] ^= 1;
    Transcript tv(tlabel);
    *verified = p.verify(g, tv, rv, cy, comm) ? 1 : 0;
    return rc;
  } catch (const std::string&) {
    return -1;
  }
}

// PolyEvalProof::prove_batched_points (dense_mlpoly.rs:531-622): K points of nv scalars on Z, then ser_proofs.
// *nproofs = the list's length; *verified: orc::verify_plain_batched_points against poly_commit(Z) on a fresh
// transcript (tamper: the last proof's z1 lowest byte flipped first)
int pe_prove_points(const char* label, size_t gens_nv, const char* tlabel, const char* tape_name, const uint64_t* seed,
                    const uint64_t* Z, size_t nv, const uint64_t* r_list, size_t K, const uint64_t* Zr_list, int tamper,
                    uint8_t* proof, size_t cap, size_t* len, size_t* nproofs, uint8_t* check, uint64_t* tape_next,
                    int* verified) {
  try {
    const DotGens g = poly_commit_gens_new(gens_nv, label);
    const DensePoly poly(ldv(Z, pow2(nv)));
    std::vector<FqVec> rl;
    for (size_t i = 0; i < K; i++) rl.push_back(ldv(r_list + 4 * i * nv, nv));
    const FqVec zr = ldv(Zr_list, K);
    Transcript t(tlabel);
    RandomTape tape(tape_name, ld(seed));
    std::vector<PolyEvalProof> ps = PolyEvalProof::prove_batched_points(poly, rl, zr, g, t, tape);
    *nproofs = ps.size();
    Ser s;
    ser_proofs(s, ps);
    const int rc = finish(s, t, tape, proof, cap, len, check, tape_next);
    if (tamper) ps.back().proof.z1.v[0] ^= 1;
    Transcript tv(tlabel);
    *verified = verify_plain_batched_points(ps, g, tv, rl, zr, poly_commit(poly, g)) ? 1 : 0;
    return rc;
  } catch (const std::string&) {
    return -1;
  }
}

// PolyEvalProof::prove_batched_instances (dense_mlpoly.rs:689-780): n polynomials (Z concatenated, 2^nv_list[i]
// scalars each), points concatenated with r_lens[i] scalars each. *verified: orc::verify_plain_batched_instances
int pe_prove_instances(const char* label, size_t gens_nv, const char* tlabel, const char* tape_name,
                       const uint64_t* seed, const uint64_t* Z, const size_t* nv_list, size_t n, const uint64_t* r_list,
                       const size_t* r_lens, const uint64_t* Zr_list, int tamper, uint8_t* proof, size_t cap,
                       size_t* len, size_t* nproofs, uint8_t* check, uint64_t* tape_next, int* verified) {
  try {
    const DotGens g = poly_commit_gens_new(gens_nv, label);
    std::vector<DensePoly> polys;
    std::vector<FqVec> rl;
    std::vector<size_t> nvs(nv_list, nv_list + n);
    size_t zo = 0, ro = 0;
    for (size_t i = 0; i < n; zo += pow2(nv_list[i]), ro += r_lens[i], i++) {
      polys.push_back(DensePoly(ldv(Z + 4 * zo, pow2(nv_list[i]))));
      rl.push_back(ldv(r_list + 4 * ro, r_lens[i]));
    }
    std::vector<const DensePoly*> pp;
    for (auto& p : polys) pp.push_back(&p);
    const FqVec zr = ldv(Zr_list, n);
    Transcript t(tlabel);
    RandomTape tape(tape_name, ld(seed));
    std::vector<PolyEvalProof> ps = PolyEvalProof::prove_batched_instances(pp, rl, zr, g, t, tape);
    *nproofs = ps.size();
    Ser s;
    ser_proofs(s, ps);
    const int rc = finish(s, t, tape, proof, cap, len, check, tape_next);
    std::vector<PolyCommitment> comms;
    for (auto& p : polys) comms.push_back(poly_commit(p, g));
    if (tamper) ps.back().proof.z1.v[0] ^= 1;
    Transcript tv(tlabel);
    *verified = verify_plain_batched_instances(ps, g, tv, rl, zr, comms, nvs) ? 1 : 0;
    return rc;
  } catch (const std::string&) {
    return -1;
  }
}

// The grouping of the two batched forms as the oracle's provers derive it (their key lists and the running
// coefficient), without proving: group[i] = the proof slot of term i in first-seen order, exp[i] = the power of
// challenge_c it joins with (0 for the term that opened the slot), fitted = every term's fitted point concatenated.
// instances = 0: n points of nv_list[0] scalars (r_lens unused). Returns the number of slots.
long pe_groups(int instances, size_t n, const size_t* nv_list, const uint64_t* r_list, const size_t* r_lens,
               size_t* group, size_t* exp, uint64_t* fitted) {
  std::vector<std::pair<size_t, FqVec>> keys;
  size_t e = 0, ro = 0, fo = 0;
  for (size_t i = 0; i < n; i++) {
    const size_t nv = instances ? nv_list[i] : nv_list[0], len = instances ? r_lens[i] : nv;
    const FqVec r = fit(ldv(r_list + 4 * ro, len), nv);
    ro += len;
    stv(fitted + 4 * fo, r);
    fo += nv;
    FqVec L, R;
    eq_factored_evals(r, &L, &R);
    size_t ln, rn;
    eq_factored_lens(nv, &ln, &rn);
    const std::pair<size_t, FqVec> key =
        instances ? std::make_pair(nv, R) : std::make_pair((size_t)0, FqVec(r.begin(), r.begin() + ln));
    size_t idx = keys.size();
    for (size_t k = 0; k < keys.size(); k++)
      if (keys[k] == key) {
        idx = k;
        break;
      }
    group[i] = idx;
    if (idx < keys.size()) {
      exp[i] = ++e;
    } else {
      exp[i] = 0;
      keys.push_back(key);
    }
  }
  return (long)keys.size();
}

}  // extern "C"
