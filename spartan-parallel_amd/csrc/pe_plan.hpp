// spg — the grouping plan of PolyEvalProof's batched openings (src/dense_mlpoly.rs:531-857), derived from the points
// and sizes alone and written once. Host-only (no HIP types): polyeval.hip's provers and verifiers and
// libspg_hostcheck.so (spgh_pe_plan, the tests' view of it) include it.
//
// Both batched forms walk their terms in order and keep a map from a key to a proof slot. A term whose key is new
// opens a slot (coefficient 1); a term whose key repeats first advances the one running coefficient c <- c * c_base
// and then joins its slot with that c. c advances on every repeat of any key, so the exponents of the repeats count
// 1, 2, 3, .. in encounter order across all slots, not per slot.
//   points form    (prove_batched_points, :531-622):    key = the left half of r (the first num_vars / 2 entries)
//   instances form (prove_batched_instances, :689-780): key = (num_vars, R vector) of the fitted point
// The reference compares R vectors; eq tables of equal length are equal exactly when their points are (r_j is the sum
// of the entries whose index has bit j set), so the plan compares the right halves of the fitted points instead.
//
// The plan also lays out the device bound (polyeval.hip): every term that is bound owns S row ranges of `chunk` rows
// ("slabs" of Rs partial sums each), and the slabs of one group's terms are contiguous, so the column-sum stage adds
// a group's S_g slabs without an indirection.
#pragma once
#include <string.h>

#include <algorithm>
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

// a point shorter than nv is padded with zeros at the front, a longer one keeps its last nv entries (:712-722)
inline std::vector<Fq> pe_fit(const Fq* r, size_t len, size_t nv) {
  std::vector<Fq> v;
  if (nv >= len) {
    v.assign(nv - len, fq_zero());
    v.insert(v.end(), r, r + len);
  } else {
    v.assign(r + (len - nv), r + len);
  }
  return v;
}
inline bool pe_same(const Fq* a, const Fq* b, size_t n) { return n == 0 || memcmp(a, b, n * sizeof(Fq)) == 0; }

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

// points form: K points of nv scalars each (row-major) on one polynomial
inline PePlan pe_plan_points(const Fq* r_list, size_t K, size_t nv, int kt = kPeKT) {
  PePlan p;
  const size_t ln = nv / 2;
  size_t e = 0;
  for (size_t i = 0; i < K; i++) {
    PeTerm t;
    t.nv = nv;
    t.r.assign(r_list + i * nv, r_list + (i + 1) * nv);
    size_t idx = p.groups.size();
    for (size_t k = 0; k < p.groups.size(); k++)
      if (pe_same(p.terms[p.groups[k].first].r.data(), t.r.data(), ln)) {
        idx = k;
        break;
      }
    t.group = idx;
    if (idx < p.groups.size()) {
      t.exp = ++e;
    } else {
      PeGroup g;
      g.nv = nv, g.Ls = (size_t)1 << ln, g.Rs = (size_t)1 << (nv - ln), g.first = i;
      p.groups.push_back(g);
      t.bound = true;
    }
    p.terms.push_back(std::move(t));
  }
  pe_layout(&p, true, kt);
  return p;
}

// instances form: n polynomials of nv_list[i] variables, point i of r_lens[i] scalars (concatenated in r_list)
inline PePlan pe_plan_instances(const size_t* nv_list, const Fq* r_list, const size_t* r_lens, size_t n) {
  PePlan p;
  size_t e = 0, o = 0;
  for (size_t i = 0; i < n; o += r_lens[i++]) {
    PeTerm t;
    t.nv = nv_list[i];
    t.r = pe_fit(r_list + o, r_lens[i], t.nv);
    t.bound = true;
    const size_t ln = t.nv / 2, rn = t.nv - ln;
    size_t idx = p.groups.size();
    for (size_t k = 0; k < p.groups.size(); k++)
      if (p.groups[k].nv == t.nv && pe_same(p.terms[p.groups[k].first].r.data() + ln, t.r.data() + ln, rn)) {
        idx = k;
        break;
      }
    t.group = idx;
    if (idx < p.groups.size()) {
      t.exp = ++e;
    } else {
      PeGroup g;
      g.nv = t.nv, g.Ls = (size_t)1 << ln, g.Rs = (size_t)1 << rn, g.first = i;
      p.groups.push_back(g);
    }
    p.terms.push_back(std::move(t));
  }
  pe_layout(&p, false);
  return p;
}

// bincode(DotProductProofLog) of n = Rs scalars: two point vectors of lg Rs, delta, beta, z1, z2
inline size_t pe_proof_bytes(size_t Rs) { return 2 * (8 + 32 * lg2(Rs)) + 4 * 32; }
inline size_t pe_list_bytes(const PePlan& p) {
  size_t b = 8;
  for (const PeGroup& g : p.groups) b += pe_proof_bytes(g.Rs);
  return b;
}

}  // namespace spg
