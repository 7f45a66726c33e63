// spg — the grouping rule of PolyEvalProof's batched openings (src/dense_mlpoly.rs:531-960), derived from the points
// and sizes alone and written once. Host-only (no HIP types). Every prover and verifier of a batched form asks it
// for the walk: polyeval.hip (the whole-proof provers prove_batched_points / prove_batched_instances and the
// spg_poly_eval_* and spg_pe_* entries), r1cs.hip (Prover::polyeval_batched), verify.hip (V::pe_batched_disjoint,
// V::pe_plain_batched_points, V::pe_plain_batched_instances), and libspg_hostcheck.so (spgh_pe_plan,
// spgh_pe_plan_disjoint, spgh_pe_plan_uni and spgh_pe_walk_disjoint: the tests' view of it).
//
// Every batched form walks its terms in order and keeps a map from a key to a proof slot. A term whose key is new
// opens a slot (coefficient 1); a term whose key repeats first advances the one running coefficient c <- c * c_base
// and then joins its slot with that c. c advances on every repeat of any key, so the exponents of the repeats count
// 1, 2, 3, .. in encounter order across all slots, not per slot (pe_walk; the coefficients: pe_coeff_powers).
//   points form    (prove_batched_points, :531-622):    key = the left half of r (the first num_vars / 2 entries)
//   instances form (prove_batched_instances, :689-780): key = (num_vars, R vector) of the fitted point
//   disjoint rounds (prove_batched_instances_disjoint_rounds, :861-960): key = (num_proofs, num_inputs)
// The reference compares R vectors; eq tables of equal length are equal exactly when their points are (r_j is the sum
// of the entries whose index has bit j set), so the walk compares the right halves of the fitted points instead.
// Points are compared by their bytes: an Fq is the unique canonical value in [0, q) (field.hpp; fq_eq is the same
// limb comparison), which holds for transcript challenges, field results and the reduced scalars the C-ABI takes.
// The univariate form (prove_uni_batched_instances, :1046-1130) has no grouping: c advances after every term. It
// shares the power vectors below and has a plan of its own (pe_plan_uni): its terms have different widths.
//
// The plan also lays out the device bound (polyeval.hip): every term that is bound owns S row ranges of `chunk` rows
// ("slabs" of Rs partial sums each), and the slabs of one group's terms are contiguous, so the column-sum stage adds
// a group's S_g slabs without an indirection.
#pragma once
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "field.hpp"
#include "hostmath.hpp"

namespace spg {

constexpr int kPeKTMax = 4;          // L vectors one pass over Z can feed in the points form (an Fq is 8 VGPRs)
// .. and how many the shipped plan gives it. Measured at num_vars 24 with 4 distinct left halves, the tiled pass (4)
// did not beat 4 single passes by more than the run-to-run spread: the pass is bound by its Fq products, which
// tiling does not reduce, not by the bytes it saves (scripts/micro/pe_bound.hip)
constexpr int kPeKT = 1;
constexpr size_t kPeBlocks = 2048;   // workgroups the partial stage aims at: 8 per CU
constexpr size_t kPeMaxVars = 30;

struct PeTerm {
  size_t group = 0;       // proof slot, in first-seen order
  size_t exp = 0;         // its coefficient is c_base^exp; 0 for the term that opened the slot
  size_t nv = 0;          // variables of its polynomial
  std::vector<Fq> r;      // the fitted point: nv scalars
  bool bound = false;     // it owns slabs (instances form: every term; points form: the term that opened the slot)
  size_t S = 0, chunk = 0;  // its slabs and the rows per slab
  size_t slab = 0;        // its first slab among its group's
};
struct PeGroup {
  size_t nv = 0, Ls = 0, Rs = 0;
  size_t first = 0;       // the term that opened it
  size_t S = 0;           // slabs of all its terms
  size_t part_off = 0;    // first scalar of its slabs in the partial buffer
  size_t out_off = 0;     // first scalar of its L.Z vector in the output
};
struct PePlan {
  std::vector<PeTerm> terms;
  std::vector<PeGroup> groups;
  size_t part_len = 0, out_len = 0;  // scalars
  size_t xblocks = 0;                // column blocks of the partial stage over all its jobs
};

// ---- the walk
struct PeWalk {
  std::vector<size_t> group, exp;  // per term: its slot, and the e of its coefficient c_base^e (0 if it opened the slot)
  std::vector<size_t> first;       // per slot, in first-seen order: the term that opened it
  bool opens(size_t i) const { return first[group[i]] == i; }
  size_t repeats() const { return group.size() - first.size(); }  // the largest exponent
};
// same(i, j): is term i's key equal to the key of term j (j < i, a term that opened a slot)
template <class Same>
inline PeWalk pe_walk(size_t n, const Same& same) {
  PeWalk w;
  size_t e = 0;
  for (size_t i = 0; i < n; i++) {
    size_t k = 0;
    while (k < w.first.size() && !same(i, w.first[k])) k++;
    const bool opens = k == w.first.size();
    if (opens) w.first.push_back(i);
    w.group.push_back(k);
    w.exp.push_back(opens ? 0 : ++e);
  }
  return w;
}
inline bool pe_same(const Fq* a, const Fq* b, size_t n) { return n == 0 || memcmp(a, b, n * sizeof(Fq)) == 0; }
// points form: points of one length
inline PeWalk pe_walk_points(const std::vector<FqV>& r) {
  const size_t ln = r.empty() ? 0 : r[0].size() / 2;
  return pe_walk(r.size(), [&](size_t i, size_t j) { return pe_same(r[i].data(), r[j].data(), ln); });
}
// instances form: the fitted point of every polynomial (num_vars scalars each)
inline PeWalk pe_walk_instances(const std::vector<FqV>& r) {
  return pe_walk(r.size(), [&](size_t i, size_t j) {
    const size_t nv = r[i].size(), ln = nv / 2;
    return r[j].size() == nv && pe_same(r[i].data() + ln, r[j].data() + ln, nv - ln);
  });
}
// disjoint rounds: (num_proofs, num_inputs) of every polynomial
inline PeWalk pe_walk_disjoint(const std::vector<std::pair<size_t, size_t>>& shape) {
  return pe_walk(shape.size(), [&](size_t i, size_t j) { return shape[i] == shape[j]; });
}

// (b^i)_i, i < n
inline FqV pe_powers(const Fq& b, size_t n) {
  FqV p(n, fq_one());
  for (size_t i = 1; i < n; i++) p[i] = fq_mul(p[i - 1], b);
  return p;
}
// c_base^e for e = 0 .. a walk's largest exponent
inline FqV pe_coeff_powers(const Fq& c_base, size_t repeats) { return pe_powers(c_base, repeats + 1); }

// a point shorter than nv is padded with zeros at the front, a longer one keeps its last nv entries (:712-722)
inline FqV pe_fit(const Fq* r, size_t len, size_t nv) {
  FqV v;
  if (nv >= len) {
    v.assign(nv - len, fq_zero());
    v.insert(v.end(), r, r + len);
  } else {
    v.assign(r + (len - nv), r + len);
  }
  return v;
}
inline FqV pe_fit(const FqV& r, size_t nv) { return pe_fit(r.data(), r.size(), nv); }
// the eq tables of both halves of a point: L over its first |r| / 2 scalars, R over the rest
inline void pe_eq_halves(const FqV& r, FqV* L, FqV* R) {
  const size_t ln = r.size() / 2;
  *L = eq_evals_host(FqV(r.begin(), r.begin() + ln));
  *R = eq_evals_host(FqV(r.begin() + ln, r.end()));
}
// the univariate form's vectors at r: L = (r^(Rs j))_j, j < Ls, of a polynomial of nv variables (one table per
// distinct nv, `of` = each term's), and R = (r^i)_i, i < Rs, of the largest
struct PeUniL {
  std::vector<FqV> L;
  std::vector<size_t> nv, of;
};
inline PeUniL pe_uni_Ls(const Fq& r, const std::vector<size_t>& nv_list) {
  PeUniL u;
  for (size_t nv : nv_list) {
    size_t k = 0;
    while (k < u.nv.size() && u.nv[k] != nv) k++;
    if (k == u.nv.size()) {
      Fq r_base = fq_one();
      for (size_t e = 0; e < ((size_t)1 << (nv - nv / 2)); e++) r_base = fq_mul(r_base, r);
      u.nv.push_back(nv);
      u.L.push_back(pe_powers(r_base, (size_t)1 << (nv / 2)));
    }
    u.of.push_back(k);
  }
  return u;
}
inline FqV pe_uni_R(const Fq& r, size_t max_nv) { return pe_powers(r, (size_t)1 << (max_nv - max_nv / 2)); }

// slabs: jobs of up to kt L vectors each (1 in the instances form) share the grid; a job of nbx column blocks gets
// about kPeBlocks / xblocks row ranges, at most one per row
inline void pe_layout(PePlan* p, bool points, int kt = kPeKT) {
  size_t D = p->groups.size();
  p->xblocks = 0;
  if (points) {
    if (D) p->xblocks = ((D + kt - 1) / kt) * ((p->groups[0].Rs + 255) / 256);
  } else {
    for (const PeTerm& t : p->terms) p->xblocks += (p->groups[t.group].Rs + 255) / 256;
  }
  const size_t want = std::max<size_t>(1, kPeBlocks / std::max<size_t>(1, p->xblocks));
  for (PeGroup& g : p->groups) g.S = 0;
  for (PeTerm& t : p->terms) {
    if (!t.bound) continue;
    PeGroup& g = p->groups[t.group];
    size_t S = std::min(g.Ls, want);
    t.chunk = (g.Ls + S - 1) / S;
    t.S = (g.Ls + t.chunk - 1) / t.chunk;
    t.slab = g.S;
    g.S += t.S;
  }
  p->part_len = p->out_len = 0;
  for (PeGroup& g : p->groups) {
    g.part_off = p->part_len;
    g.out_off = p->out_len;
    p->part_len += g.S * g.Rs;
    p->out_len += g.Rs;
  }
}

// the plan of a walk over the terms' (fitted) points: a term is bound if it opened its slot, or always (instances)
inline PePlan pe_plan_of(const PeWalk& w, std::vector<FqV> r, bool points, int kt) {
  PePlan p;
  for (size_t i = 0; i < r.size(); i++) {
    PeTerm t;
    t.group = w.group[i], t.exp = w.exp[i], t.nv = r[i].size();
    t.bound = !points || w.opens(i);
    t.r = std::move(r[i]);
    p.terms.push_back(std::move(t));
  }
  for (size_t i : w.first) {
    PeGroup g;
    g.nv = p.terms[i].nv, g.Ls = (size_t)1 << (g.nv / 2), g.Rs = (size_t)1 << (g.nv - g.nv / 2), g.first = i;
    p.groups.push_back(g);
  }
  pe_layout(&p, points, kt);
  return p;
}
// points form: K points of nv scalars each (row-major) on one polynomial
inline PePlan pe_plan_points(const Fq* r_list, size_t K, size_t nv, int kt = kPeKT) {
  std::vector<FqV> r(K);
  for (size_t i = 0; i < K; i++) r[i].assign(r_list + i * nv, r_list + (i + 1) * nv);
  return pe_plan_of(pe_walk_points(r), r, true, kt);
}
// instances form: n polynomials of nv_list[i] variables, point i of r_lens[i] scalars (concatenated in r_list)
inline PePlan pe_plan_instances(const size_t* nv_list, const Fq* r_list, const size_t* r_lens, size_t n) {
  std::vector<FqV> r(n);
  for (size_t i = 0, o = 0; i < n; o += r_lens[i++]) r[i] = pe_fit(r_list + o, r_lens[i], nv_list[i]);
  return pe_plan_of(pe_walk_instances(r), r, false, kPeKT);
}
// disjoint rounds: polynomial i has np[i] * ni[i] scalars (powers of two, lg np[i] <= rq_len: the caller's check); its
// point is the last lg np[i] entries of rq, then ry fitted to lg ni[i] entries (:905-921). The instances form with
// another key and another fit: every term is bound, a repeat's scaled L table makes the group sum LZ_list[idx] += c LZ
inline PePlan pe_plan_disjoint(const size_t* np, const size_t* ni, size_t n, const Fq* rq, size_t rq_len, const Fq* ry,
                               size_t ry_len) {
  std::vector<std::pair<size_t, size_t>> shape(n);
  std::vector<FqV> r(n);
  for (size_t i = 0; i < n; i++) {
    shape[i] = {np[i], ni[i]};
    r[i].assign(rq + (rq_len - lg2(np[i])), rq + rq_len);
    const FqV rys = pe_fit(ry, ry_len, lg2(ni[i]));
    r[i].insert(r[i].end(), rys.begin(), rys.end());
  }
  return pe_plan_of(pe_walk_disjoint(shape), r, false, kPeKT);
}

// The univariate form (prove_uni_batched_instances, :1046-1130) has no walk: term i joins with c_base^i (c advances
// after every term, the first included) and all terms add into ONE vector of the widest polynomial's R_size, term i
// into its first Rs_i entries only (:1109-1112). The slabs of a term therefore have a width of their own, and a group
// of the column-sum stage is a list of terms of different widths (k_pe_sum_ragged, pe_bound.hpp): term t owns S slabs
// of Rs scalars at part_off. per_term: one output of Rs_i scalars per term instead (the evaluations sum_k Z_i[k] r^k
// are read from them), each group a list of one.
struct PeUniTerm {
  size_t exp = 0;           // its coefficient is c_base^exp: its index
  size_t nv = 0, Ls = 0, Rs = 0;
  size_t S = 0, chunk = 0;  // its slabs and the rows per slab
  size_t part_off = 0;      // first scalar of its slabs in the partial buffer
  size_t out_off = 0;       // first scalar of the output it adds into
};
struct PeUniPlan {
  std::vector<PeUniTerm> terms;  // term i: coefficient c_base^i
  size_t R_size = 0;             // of the widest polynomial
  bool per_term = false;
  size_t part_len = 0, out_len = 0, xblocks = 0;
};
inline PeUniPlan pe_plan_uni(const size_t* nv_list, size_t n, bool per_term) {
  PeUniPlan p;
  p.per_term = per_term;
  for (size_t i = 0; i < n; i++) {
    PeUniTerm t;
    t.exp = i;
    t.nv = nv_list[i], t.Ls = (size_t)1 << (t.nv / 2), t.Rs = (size_t)1 << (t.nv - t.nv / 2);
    p.R_size = std::max(p.R_size, t.Rs);
    p.xblocks += (t.Rs + 255) / 256;
    p.terms.push_back(t);
  }
  const size_t want = std::max<size_t>(1, kPeBlocks / std::max<size_t>(1, p.xblocks));  // as pe_layout
  for (PeUniTerm& t : p.terms) {
    const size_t S = std::min(t.Ls, want);
    t.chunk = (t.Ls + S - 1) / S;
    t.S = (t.Ls + t.chunk - 1) / t.chunk;
    t.part_off = p.part_len;
    p.part_len += t.S * t.Rs;
    if (per_term) {
      t.out_off = p.out_len;
      p.out_len += t.Rs;
    }
  }
  if (!per_term) p.out_len = p.R_size;
  return p;
}
// L'_t = c_base^t (r^(Rs_t j))_j of every term: the scaled eq tables' counterpart
inline std::vector<FqV> pe_uni_scaled_Ls(const Fq& r, const std::vector<size_t>& nv_list, const Fq& c_base) {
  const PeUniL u = pe_uni_Ls(r, nv_list);
  std::vector<FqV> Lp(nv_list.size());
  Fq c = fq_one();
  for (size_t i = 0; i < nv_list.size(); i++, c = fq_mul(c, c_base)) {
    Lp[i] = u.L[u.of[i]];
    if (i)
      for (Fq& x : Lp[i]) x = fq_mul(x, c);
  }
  return Lp;
}

// bincode(DotProductProofLog) of n = Rs scalars: two point vectors of lg Rs, delta, beta, z1, z2
inline size_t pe_proof_bytes(size_t Rs) { return 2 * (8 + 32 * lg2(Rs)) + 4 * 32; }
inline size_t pe_list_bytes(const PePlan& p) {
  size_t b = 8;
  for (const PeGroup& g : p.groups) b += pe_proof_bytes(g.Rs);
  return b;
}

}  // namespace spg
