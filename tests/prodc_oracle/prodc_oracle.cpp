// TEST HELPER — never linked into the product. The product-circuit entries of the CPU oracle (oracle/spark.hpp,
// oracle/sumcheck.hpp as they stand) behind a C interface, for tests/test_prodc_oracle.py and tests/test_gpu_prodc.py.
// Scalars cross as four Montgomery u64 limbs, vectors as n x 4 limbs.
#include <string.h>

#include <string>
#include <vector>

#include "../../oracle/spark.hpp"

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
}  // namespace

extern "C" {

// The hash part of orc::build_layers (spark.hpp:403-430; Layers::build_hash_layer, src/sparse_mlpoly.rs:612-687):
// eval_table, audit_ts: cells scalars; addrs, derefs, read_ts: n x ops scalars (instance k at k * ops).
// init, audit: cells scalars; reads, writes: n x ops.
int po_hash_layer(const uint64_t* eval_table, const uint64_t* audit_ts, size_t cells, const uint64_t* addrs,
                  const uint64_t* derefs, const uint64_t* read_ts, size_t n, size_t ops, const uint64_t* r_hash,
                  const uint64_t* r_multiset, uint64_t* init, uint64_t* reads, uint64_t* writes, uint64_t* audit) {
  const Fq rh = ld(r_hash), rms = ld(r_multiset), r2 = fq_mul(rh, rh);
  auto hash = [&](const Fq& addr, const Fq& val, const Fq& ts) {
    return fq_sub(fq_add(fq_add(fq_mul(ts, r2), fq_mul(val, rh)), addr), rms);
  };
  for (size_t i = 0; i < cells; i++) {
    const Fq a = fq_from_u64(i), v = ld(eval_table + 4 * i);
    st(init + 4 * i, hash(a, v, fq_zero()));
    st(audit + 4 * i, hash(a, v, ld(audit_ts + 4 * i)));
  }
  for (size_t i = 0; i < n * ops; i++) {
    const Fq a = ld(addrs + 4 * i), v = ld(derefs + 4 * i), ts = ld(read_ts + 4 * i);
    st(reads + 4 * i, hash(a, v, ts));
    st(writes + 4 * i, hash(a, v, fq_add(ts, fq_one())));
  }
  return 0;
}

// ProductCircuit::create (src/product_tree.rs:18-58) of M leaves: left (then right) receives left_vec[0], left_vec[1],
// ... back to back (M/2 + M/4 + ... + 1 = M - 1 scalars each), eval the circuit's evaluate()
int po_circuit_layers(const uint64_t* leaves, size_t M, uint64_t* left, uint64_t* right, uint64_t* eval) {
  try {
    const ProductCircuit c = ProductCircuit::create(DensePoly(ldv(leaves, M)));
    size_t o = 0;
    for (size_t k = 0; k < c.left_vec.size(); k++) {
      stv(left + 4 * o, c.left_vec[k].Z);
      stv(right + 4 * o, c.right_vec[k].Z);
      o += c.left_vec[k].len;
    }
    st(eval, c.evaluate());
    return 0;
  } catch (const std::string&) {
    return -1;
  }
}

// orc::prove_cubic_batched (src/sumcheck.rs:264-434) on a fresh Transcript(label). Apar, Bpar: n_par x len scalars; Cpar:
// len; Aseq, Bseq, Cseq: n_seq x len. polys: num_rounds x 3; r: num_rounds; every vector's bound state (len >>
// num_rounds scalars each) into bound in the order Apar.., Bpar.., Cpar, Aseq.., Bseq.., Cseq..; check: 64 bytes of
// challenge_bytes("seam_check") drawn afterwards
int po_cubic_batched(const char* label, const uint64_t* claim, size_t num_rounds, const uint64_t* Apar,
                     const uint64_t* Bpar, size_t n_par, const uint64_t* Cpar, const uint64_t* Aseq,
                     const uint64_t* Bseq, const uint64_t* Cseq, size_t n_seq, size_t len, const uint64_t* coeffs,
                     uint64_t* polys, uint64_t* r, uint64_t* bound, uint8_t* check) {
  try {
    std::vector<DensePoly> ap, bp, as, bs, cs;
    for (size_t i = 0; i < n_par; i++) {
      ap.push_back(DensePoly(ldv(Apar + 4 * i * len, len)));
      bp.push_back(DensePoly(ldv(Bpar + 4 * i * len, len)));
    }
    for (size_t i = 0; i < n_seq; i++) {
      as.push_back(DensePoly(ldv(Aseq + 4 * i * len, len)));
      bs.push_back(DensePoly(ldv(Bseq + 4 * i * len, len)));
      cs.push_back(DensePoly(ldv(Cseq + 4 * i * len, len)));
    }
    DensePoly cpar(ldv(Cpar, len));
    std::vector<DensePoly*> Ap, Bp, As, Bs, Cs;
    for (size_t i = 0; i < n_par; i++) Ap.push_back(&ap[i]), Bp.push_back(&bp[i]);
    for (size_t i = 0; i < n_seq; i++) As.push_back(&as[i]), Bs.push_back(&bs[i]), Cs.push_back(&cs[i]);
    Transcript t(label);
    FqVec rr;
    const SumcheckProof sp =
        prove_cubic_batched(ld(claim), num_rounds, Ap, Bp, cpar, As, Bs, Cs, ldv(coeffs, n_par + n_seq), t, &rr);
    for (size_t j = 0; j < num_rounds; j++) {
      stv(polys + 12 * j, sp.polys[j]);
      st(r + 4 * j, rr[j]);
    }
    const size_t m = len >> num_rounds;
    size_t o = 0;
    auto put = [&](const DensePoly& p) {
      stv(bound + 4 * o, p.Z);
      o += m;
    };
    for (auto& p : ap) put(p);
    for (auto& p : bp) put(p);
    put(cpar);
    for (auto& p : as) put(p);
    for (auto& p : bs) put(p);
    for (auto& p : cs) put(p);
    t.challenge_bytes("seam_check", check, 64);
    return 0;
  } catch (const std::string&) {
    return -1;
  }
}

// ProductCircuitEvalProofBatched::prove (src/product_tree.rs:260-396) over nc circuits of M leaves (leaves: nc x M) and
// nd dot-product circuits (dotp: nd x 3 x M/2: left, right, weight) on a fresh Transcript(label), then ser. proof
// receives the bytes (*len = their number even when cap is too small), rand lg(M) scalars, check 64 bytes of
// challenge_bytes("seam_check") drawn from the prover's transcript afterwards. *verified: whether the oracle's own
// verify accepts these bytes' proof on a fresh Transcript(label) with claims = the circuits' evaluate() and the dot
// products' evaluate(); with tamper != 0 the first claims_prod_left scalar of the last layer proof has its lowest
// byte changed first (in the verified copy only: proof still receives the prover's bytes)
int po_prove_batched(const char* label, const uint64_t* leaves, size_t nc, size_t M, const uint64_t* dotp, size_t nd,
                     int tamper, uint8_t* proof, size_t cap, size_t* len, uint64_t* rand, uint8_t* check,
                     int* verified) {
  try {
    std::vector<ProductCircuit> pc;
    std::vector<DotProductCircuit> dc(nd);
    for (size_t c = 0; c < nc; c++) pc.push_back(ProductCircuit::create(DensePoly(ldv(leaves + 4 * c * M, M))));
    const size_t h = M / 2;
    FqVec claims_prod, claims_dotp;
    for (auto& c : pc) claims_prod.push_back(c.evaluate());
    for (size_t k = 0; k < nd; k++) {
      dc[k].left = DensePoly(ldv(dotp + 4 * (3 * k) * h, h));
      dc[k].right = DensePoly(ldv(dotp + 4 * (3 * k + 1) * h, h));
      dc[k].weight = DensePoly(ldv(dotp + 4 * (3 * k + 2) * h, h));
      claims_dotp.push_back(dc[k].evaluate());
    }
    std::vector<ProductCircuit*> P;
    std::vector<DotProductCircuit*> D;
    for (auto& c : pc) P.push_back(&c);
    for (auto& d : dc) D.push_back(&d);
    Transcript t(label);
    FqVec rnd;
    ProductCircuitEvalProofBatched pf = ProductCircuitEvalProofBatched::prove(P, D, t, &rnd);
    Ser s;
    pf.ser(s);
    *len = s.b.size();
    if (s.b.size() <= cap) memcpy(proof, s.b.data(), s.b.size());
    stv(rand, rnd);
    t.challenge_bytes("seam_check", check, 64);
    if (tamper) pf.proof.back().claims_prod_left[0].v[0] ^= 1;
    Transcript tv(label);
    FqVec co, cdo, ro;
    *verified = pf.verify(claims_prod, claims_dotp, M, tv, &co, &cdo, &ro) ? 1 : 0;
    return s.b.size() <= cap ? 0 : -2;
  } catch (const std::string&) {
    return -1;
  }
}

}  // extern "C"
