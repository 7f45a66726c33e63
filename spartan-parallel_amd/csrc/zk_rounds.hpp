// spg — the round bookkeeping of the two ZK sumchecks of R1CSProof::prove (the Prover of r1cs.hip) and of their seams (seams.hip).
#pragma once
#include "hostpoly.hpp"
#include "knobs.hpp"
#include "proto.hpp"

namespace spg {

// ZK sumcheck round bookkeeping shared by phase 1 and phase 2 (sumcheck.rs:1247-1370).
// The RandomTape is a transcript that only ever absorbs labels, so the values a round draws do not depend on
// the proof: init() draws blinds_poly / blinds_evals as the reference does, then reads every round's
// DotProductProof randomness (d_vec, r_delta, r_beta) from a copy of the tape at that position and computes,
// in one host burst, the points that depend on randomness alone (blind * h terms, delta). The rounds then
// commit only their data-dependent terms, and the tape continues from the copy's final state after the last
// round (no other draw happens between the rounds), so proofs are byte-identical.
struct ZKRounds {
  FqV blinds_poly, blinds_evals;
  Fq claim, blind_claim;
  Pt comm_claim;
  ZKSumcheckP out;
  FqV poly;
  Pt comm_poly;
  std::vector<DotPre> pre;
  std::vector<h::HExt> hp, he;  // blinds_poly[j] * h (gens_4), blinds_evals[j] * h (gens_1)
  Tape tape_end{"", fq_zero()};
  bool ahead = false;
  void init(ProverGens& g, Tape& tape, size_t rounds, const Fq& c, const Fq& b) {
    blinds_poly = tape.vec("blinds_poly", rounds);
    blinds_evals = tape.vec("blinds_evals", rounds);
    claim = c;
    blind_claim = b;
    ahead = knob::tape_ahead() && rounds > 0 && g.gens_4.G.size() == 4;
    if (!ahead) {
      comm_claim = commit_batch(g, {CJob(g.gens_1, {c}, b)})[0];
      return;
    }
    tape_end = tape;
    pre.resize(rounds);
    for (size_t j = 0; j < rounds; j++) {
      pre[j].d = tape_end.vec("d_vec", 4);
      pre[j].r_delta = tape_end.scalar("r_delta");
      pre[j].r_beta = tape_end.scalar("r_beta");
    }
    hp.resize(rounds);
    he.resize(rounds);
    // jobs: comm_claim, then per round blinds_poly h4, blinds_evals h1, r_beta h1, delta (d G4 + r_delta h4)
    std::vector<std::pair<std::vector<size_t>, FqV>> jobs;
    jobs.push_back({{g.gens_1.G[0], g.gens_1.h}, {c, b}});
    for (size_t j = 0; j < rounds; j++) {
      jobs.push_back({{g.gens_4.h}, {blinds_poly[j]}});
      jobs.push_back({{g.gens_1.h}, {blinds_evals[j]}});
      jobs.push_back({{g.gens_1.h}, {pre[j].r_beta}});
      std::vector<size_t> idx(g.gens_4.G.begin(), g.gens_4.G.end());
      idx.push_back(g.gens_4.h);
      FqV sc = pre[j].d;
      sc.push_back(pre[j].r_delta);
      jobs.push_back({idx, sc});
    }
    g.host.run(jobs, nullptr, [&](size_t k, const h::HExt& sum) {
      if (k == 0) {
        comm_claim = compress(sum);
        return;
      }
      const size_t j = (k - 1) / 4;
      switch ((k - 1) % 4) {
        case 0: hp[j] = sum; break;
        case 1: he[j] = sum; break;
        case 2: pre[j].rbh = sum; break;
        default: pre[j].delta = compress(sum);
      }
    });
  }
  // commit the round polynomial and draw r_j
  Fq begin(ProverGens& g, Tr& t, size_t j, const Fq e[3]) {
    Fq ev[4] = {e[0], fq_sub(claim, e[0]), e[1], e[2]};
    poly = uni_from_evals3(ev);
    if (ahead)
      comm_poly = g.host.commit_many_plus({{g.gens_4.G, poly}}, &hp[j])[0];
    else
      comm_poly = commit_batch(g, {CJob(g.gens_4, poly, blinds_poly[j])})[0];
    t.point("comm_poly", comm_poly);
    out.comm_polys.push_back(comm_poly);
    return t.challenge("challenge_nextround");
  }
  void finish(ProverGens& g, Tr& t, Tape& tape, size_t j, const Fq& r_j) {
    Fq eval = uni_eval(poly, r_j);
    Pt comm_eval = ahead ? g.host.commit_many_plus({{{g.gens_1.G[0]}, {eval}}}, &he[j])[0]
                         : commit_batch(g, {CJob(g.gens_1, {eval}, blinds_evals[j])})[0];
    t.point("comm_claim_per_round", comm_claim);
    t.point("comm_eval", comm_eval);
    FqV w = t.challenges("combine_two_claims_to_one", 2);
    Fq target = fq_add(fq_mul(w[0], claim), fq_mul(w[1], eval));
    Fq blind_sc = j == 0 ? blind_claim : blinds_evals[j - 1];
    Fq blind = fq_add(fq_mul(w[0], blind_sc), fq_mul(w[1], blinds_evals[j]));
    size_t n = poly.size();
    FqV a(n);
    Fq pw = fq_one();
    for (size_t k = 0; k < n; k++) {
      Fq a_sc = k == 0 ? fq_dbl(fq_one()) : fq_one();
      a[k] = fq_add(fq_mul(w[0], a_sc), fq_mul(w[1], pw));
      pw = fq_mul(pw, r_j);
    }
    out.proofs.push_back(dotproduct_prove(g, g.gens_1, g.gens_4, t, tape, poly, blinds_poly[j], a, target, blind,
                                          &comm_poly, ahead ? &pre[j] : nullptr));
    if (ahead && j + 1 == pre.size()) tape = tape_end;  // past every round's draws
    claim = eval;
    comm_claim = comm_eval;
    out.comm_evals.push_back(comm_eval);
  }
};

}  // namespace spg
