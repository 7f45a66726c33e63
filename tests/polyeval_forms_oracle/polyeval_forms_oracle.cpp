// TEST HELPER — never linked into the product. The disjoint-rounds and univariate forms of PolyEvalProof in the CPU
// oracle (oracle/polyeval.hpp as it stands) behind a C interface, for tests/test_polyeval_forms_oracle.py and
// tests/test_gpu_polyeval_forms.py. Scalars cross as four Montgomery u64 limbs, vectors as n x 4 limbs.
//
// Both prove wrappers run on a fresh Transcript(tlabel) and RandomTape(tape_name, seed) and return, besides the bincode
// bytes, 64 bytes of challenge_bytes("seam_check") drawn from the transcript afterwards and one more
// random_scalar("seam_check") drawn from the tape afterwards (the positions both were left in), the commitments
// C_Zr_i = Zr_i G_n (gens_1, blind 0) to the evaluations, and the verdict of the oracle's own verifier on the proof
// against poly_commit of every polynomial and those commitments, on a fresh Transcript(tlabel).
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
int finish(const Ser& s, Transcript& t, RandomTape& tape, uint8_t* proof, size_t cap, size_t* len, uint8_t* check,
           uint64_t* tape_next) {
  *len = s.b.size();
  if (s.b.size() <= cap) memcpy(proof, s.b.data(), s.b.size());
  t.challenge_bytes("seam_check", check, 64);
  st(tape_next, tape.random_scalar("seam_check"));
  return s.b.size() <= cap ? 0 : -2;
}
// the polynomials of a call (Z concatenated, sizes[i] scalars each), their commitments and the C_Zr_i
struct Instances {
  std::vector<DensePoly> polys;
  std::vector<const DensePoly*> pp;
  std::vector<PolyCommitment> comms;
  std::vector<const PolyCommitment*> cp;
  std::vector<Ge> czr;
  Instances(const DotGens& g, const uint64_t* Z, const std::vector<size_t>& sizes, const FqVec& zr, uint8_t* C_Zr_out) {
    size_t zo = 0;
    for (size_t i = 0; i < sizes.size(); zo += sizes[i], i++) polys.push_back(DensePoly(ldv(Z + 4 * zo, sizes[i])));
    for (auto& p : polys) {
      pp.push_back(&p);
      comms.push_back(poly_commit(p, g));
    }
    for (auto& c : comms) cp.push_back(&c);
    for (size_t i = 0; i < sizes.size(); i++) {
      czr.push_back(commit1(zr[i], fq_zero(), g.gens_1));
      const CPt c = cpt(czr.back());
      memcpy(C_Zr_out + 32 * i, c.v, 32);
    }
  }
};
}  // namespace

extern "C" {

// PolyEvalProof::prove_batched_instances_disjoint_rounds (dense_mlpoly.rs:861-960), then ser_proofs: polynomial i has
// np_list[i] * ni_list[i] scalars. *verified: verify_batched_instances_disjoint_rounds (:962-1044)
int pf_prove_disjoint(const char* label, size_t gens_nv, const char* tlabel, const char* tape_name,
                      const uint64_t* seed, const uint64_t* Z, const size_t* np_list, const size_t* ni_list, size_t n,
                      const uint64_t* rq, size_t rq_len, const uint64_t* ry, size_t ry_len, const uint64_t* Zr_list,
                      uint8_t* proof, size_t cap, size_t* len, size_t* nproofs, uint8_t* check, uint64_t* tape_next,
                      int* verified, uint8_t* C_Zr_out) {
  try {
    const DotGens g = poly_commit_gens_new(gens_nv, label);
    const std::vector<size_t> np(np_list, np_list + n), ni(ni_list, ni_list + n);
    std::vector<size_t> sizes;
    for (size_t i = 0; i < n; i++) sizes.push_back(np[i] * ni[i]);
    const FqVec zr = ldv(Zr_list, n), q = ldv(rq, rq_len), y = ldv(ry, ry_len);
    Instances in(g, Z, sizes, zr, C_Zr_out);
    Transcript t(tlabel);
    RandomTape tape(tape_name, ld(seed));
    const std::vector<PolyEvalProof> ps =
        PolyEvalProof::prove_batched_instances_disjoint_rounds(in.pp, np, ni, q, y, zr, g, t, tape);
    *nproofs = ps.size();
    Ser s;
    ser_proofs(s, ps);
    const int rc = finish(s, t, tape, proof, cap, len, check, tape_next);
    Transcript tv(tlabel);
    *verified =
        PolyEvalProof::verify_batched_instances_disjoint_rounds(ps, np, ni, g, tv, q, y, in.czr, in.cp) ? 1 : 0;
    return rc;
  } catch (const std::string&) {
    return -1;
  }
}

// PolyEvalProof::prove_uni_batched_instances (dense_mlpoly.rs:1046-1130): n polynomials of 2^nv_list[i] scalars at
// the scalar r. C_Zr_prime: the prover's own commitment to the combined evaluation. *verified:
// verify_uni_batched_instances (:1132-1203) with poly_size[i] = 2^nv_list[i]
int pf_prove_uni(const char* label, size_t gens_nv, const char* tlabel, const char* tape_name, const uint64_t* seed,
                 const uint64_t* Z, const size_t* nv_list, size_t n, const uint64_t* r, const uint64_t* Zr_list,
                 uint8_t* proof, size_t cap, size_t* len, uint8_t* C_Zr_prime, uint8_t* check, uint64_t* tape_next,
                 int* verified, uint8_t* C_Zr_out) {
  try {
    const DotGens g = poly_commit_gens_new(gens_nv, label);
    std::vector<size_t> sizes;
    for (size_t i = 0; i < n; i++) sizes.push_back(pow2(nv_list[i]));
    const FqVec zr = ldv(Zr_list, n);
    Instances in(g, Z, sizes, zr, C_Zr_out);
    Transcript t(tlabel);
    RandomTape tape(tape_name, ld(seed));
    CPt cy;
    const PolyEvalProof p = PolyEvalProof::prove_uni_batched_instances(in.pp, ld(r), zr, g, t, tape, &cy);
    memcpy(C_Zr_prime, cy.v, 32);
    Ser s;
    p.ser(s);
    const int rc = finish(s, t, tape, proof, cap, len, check, tape_next);
    Transcript tv(tlabel);
    *verified = verify_uni_batched_instances(p, g, tv, ld(r), in.czr, in.cp, sizes) ? 1 : 0;
    return rc;
  } catch (const std::string&) {
    return -1;
  }
}

// the evaluations the univariate form opens: out[i] = sum_k Z_i[k] r^k (Horner from the top coefficient)
int pf_uni_evals(const uint64_t* Z, const size_t* nv_list, size_t n, const uint64_t* r, uint64_t* out) {
  const Fq rr = ld(r);
  size_t zo = 0;
  for (size_t i = 0; i < n; zo += pow2(nv_list[i]), i++) {
    Fq e = fq_zero();
    for (size_t k = pow2(nv_list[i]); k-- > 0;) e = fq_add(fq_mul(e, rr), ld(Z + 4 * (zo + k)));
    st(out + 4 * i, e);
  }
  return 0;
}

}  // extern "C"
