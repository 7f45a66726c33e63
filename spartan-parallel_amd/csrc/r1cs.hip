// spg — R1CSProof::prove (src/r1csproof.rs:210-685) with every O(N) table resident in HBM.
//
// This file is the Prover: the stages in protocol order, the sigma protocols, the openings and the cross-rank
// exchanges, with spg_r1cs_prove and spg_r1cs_sat_check. It holds no kernel.
// Device work (HIP):
//   the tables: Z, Az / Bz / Cz, ABC, the witness sections' L.Z bounds    r1cs_tables.hip (R1csTables, launch_*)
//   phase-1 / phase-2 round evaluation and folds                  sumcheck.rs:1067-1380, :788-1065 (sumcheck.hip)
//   bound_poly_vars_rq on Z                                       custom_dense_mlpoly.rs:300-304 (sumcheck.hip)
//   Bulletproof L/R/delta MSMs                                    proto.hip, msm.hip
// Host work: the Fiat-Shamir transcript, the round polynomials (4 scalars), the sigma protocols over
// <= 5 fixed generators, and the bincode writer. Per sumcheck round exactly three scalars come back.
#include <chrono>
#include <stdio.h>
#include <stdlib.h>

#include "comm.hpp"
#include "hostpoly.hpp"
#include "knobs.hpp"
#include "pe_plan.hpp"
#include "proto.hpp"
#include "r1cs_tables.hpp"
#include "satcheck.hpp"
#include "sumcheck.hpp"
#include "zk_rounds.hpp"

namespace spg {

// ------------------------------------------------------------------------------------ host helpers
// (eq tables, UniPoly::from_evals, short MLE evaluations: hostmath.hpp)

// (the prover's switches: knobs.hpp) a pair's size limits, within the buffers sized by kP1PairMax
static size_t p1_pair_max() { return std::min<size_t>(kP1PairMax, (size_t)knob::p1_pair_max()); }
static size_t p2_pair_max() { return std::min<size_t>(kP1PairMax, (size_t)knob::p2_pair_max()); }

// (ZKRounds, the ZK sumcheck round bookkeeping shared by phase 1 and phase 2: zk_rounds.hpp)

// (a pair's posted grid -> round j's and round j + 1's (e0, e2, e3): pair_round_j, pair_round_j1 of hostmath.hpp)

// ------------------------------------------------------------------------------------ the R1CS prover
// R1CSProof::prove (r1csproof.rs). Prover::run_stages calls the stages in protocol order: setup_tables (Z, Az, Bz, Cz
// shapes, descriptors, tau eq tables, k_spmv), run_phase1, sigma1, phase2_prep (ABC, the Z join and q folds, eq(rp)),
// run_phase2, witness_evals (lz_bound on the device), polyeval_batched, final_claims. A phase's loop asks
// p*_next_launch for the next launch form after every challenge; p*_round_single and p*_round_pair are its two arms
// (round_pair_arm is the host sequence both phases' pair arms share).

// what the stages hand on to later ones
struct Carry {
  // device tables (Z, Az, Bz, Cz: R1csTables): ABC; the tau eq tables of phase 1; eq(rx), eq(rp) of phase 2
  PqxDev ABC;
  Fq *Ap = nullptr, *Aq = nullptr, *Ax = nullptr;
  Fq *eq_rx = nullptr, *eq_p = nullptr;
  Fq* partials = nullptr;  // round evaluations: 3 per workgroup; pair launches: one per element
  // challenges: phase 1's (x and q also in the reference's reversed order), phase 2's
  FqV rx, rq, rq_rev, rp, ry, rw, rp2;
  Fq claims1[4], claims2[3];  // (tau, Az, Bz, Cz) at phase 1's point; (eq, ABC, Z) at phase 2's
  Fq Az_blind, Bz_blind, Cz_blind, blind_post1, blind_post2;
  Fq claim2, blind2;          // phase 2's claim and its blind
  Pt comm_Az, comm_Bz, comm_Cz, comm_prod;
};

// how the folds of the `pending` rounds whose challenges are drawn reach the tables, and what evaluates the next round
struct NextLaunch {
  bool ride;   // the next launch applies them; else a launch of their own does (then the compaction, when due)
  int rounds;  // of the next launch: 0 (none left), 1 or 2
};

// phase 1 as it goes (Prover::run_phase1)
struct Phase1 {
  size_t rounds = 0;
  ZKRounds zk;
  size_t cons_len, proof_len, instance_len;  // the half lengths of the reference's loop
  size_t lenP, lenQ, lenX;                   // live lengths of the eq tables
  std::vector<size_t> sc_np, sc_nc;          // local; P rounds use all-ones of length P
  PqxDev Ac;                                 // compact Az for the instance rounds; TB, TC share its shape there
  PqxDev* T = nullptr;                       // Az, then Ac
  Fq *TB = nullptr, *TC = nullptr;
  Fq *Aq = nullptr, *Ax = nullptr;           // the live eq(tau_q), eq(tau_x)
  Fq *Aq2 = nullptr, *Ax2 = nullptr;         // the other halves of their ping-pong pairs (a fused fold writes there)
  const Fq* Ap_l = nullptr;                  // eq(tau_p) indexed by the global instance in the x / q rounds
  bool cur_pair = false;                     // the launch in flight evaluates rounds j, j + 1
  FqV r;                                     // the challenges so far
};
// phase 2 as it goes (Prover::run_phase2)
struct Phase2 {
  size_t rounds = 0;
  ZKRounds zk;
  size_t inputs_len, ws_len, instance_len;
  size_t lenP;
  std::vector<size_t> sc_ni;
  PqxDev Zc, ABCc;              // compact Z and ABC for the instance rounds
  PqxDev *TZ = nullptr, *TA = nullptr;
  const Fq* eq_l = nullptr;     // eq(rp) at the local instances
  bool fuse2 = false;           // a single round's fold may ride in the next evaluation
  Fq* ABC2 = nullptr;           // a shared ABC's ping-pong buffer
  size_t W2 = 0;                // witness-section rows per instance of a pair
  bool cur_pair = false;
  FqV r;
};

// a witness-section polynomial (section w, instance p) in the batched opening
struct PolyRef {
  size_t w, p, np, ni, Rs;
  bool mine;
  FqV LZ, R;
  Fq ev;
};

struct Prover {
  spg_ctx* ctx;
  ProverGens& g;
  const spg_r1cs_inst& inst;
  const spg_r1cs_witness& wit;
  // the device tables of the rank's instances and what makes them; sh: the sizes of the prove
  R1csTables tb;
  const Shape& sh;
  const size_t P, max_np, Y, nws;
  const std::vector<size_t>& num_proofs;
  const std::vector<size_t>& num_inputs;
  Tr& t;
  Tape& tape;
  R1CSProofP pf;
  std::vector<FqV> challenges;

  // instance shard of this rank (R1CSProof sharded by instance p over nranks processes): balanced split,
  // the first P % nranks ranks hold one instance more, so every rank holds one when nranks <= P
  const size_t rank, nranks, p0, p1;

  // s: the checked arguments (prover_args)
  Prover(spg_ctx* c, ProverGens& gg, const spg_r1cs_inst& in, const spg_r1cs_witness& w, Tr& tt, Tape& tp,
         const R1csSizes& s)
      : ctx(c), g(gg), inst(in), wit(w), tb(c, in, w, s), sh(tb.sh), P(s.P), max_np(s.max_np), Y(s.Y), nws(s.nws),
        num_proofs(tb.sz.num_proofs), num_inputs(tb.sz.num_inputs), t(tt), tape(tp), rank((size_t)c->rank),
        nranks((size_t)c->nranks), p0(s.p0), p1(s.p1) {}

  static size_t shard_begin(size_t P, size_t nranks, size_t r) {
    return r * (P / nranks) + std::min(r, P % nranks);
  }
  size_t owner_of(size_t p) const {
    size_t r = 0;
    while (r + 1 < nranks && shard_begin(P, nranks, r + 1) <= p) r++;
    return r;
  }
  int sum_ranks(Fq e[3]);
  // the exchanges of a sharded prove, in order (payload bytes per rank): their sequence depends only on public
  // sizes, so a rank that fails locally between two of them takes part in the next one with its failure as status
  // (run()) and every rank returns from that same exchange -- none is left blocked in a later one
  std::vector<size_t> xplan;
  size_t xdone = 0;
  bool xshared = false;  // an exchange already returned a failure to every rank
  void plan_exchanges(size_t np, size_t nq, size_t nx, size_t nw, size_t ny);
  int exchange(const void* send, size_t bytes, std::vector<uint8_t>& recv);
  int gather_first(const std::vector<const PqxDev*>& tabs, std::vector<std::vector<Fq>>& full);

  Carry cy;
  Laps lp;

  int run();
  int run_stages();
  int setup_tables(ZFill& zf);
  int setup_tau();
  // phase 1
  int p1_mode(size_t j) const { return j < sh.nx ? MODE_X : (j < sh.nx + sh.nq ? MODE_Q : MODE_P); }
  int p1_advance(Phase1& s, size_t j);
  int p1_launch_single(Phase1& s, size_t j, const FoldPlan* fold);
  bool p1_pair_ok(const Phase1& s, size_t j) const;
  int p1_launch_pair(Phase1& s, size_t j, int nf, const FoldPlan* fp, const Fq& r1, const Fq& r2);
  int p1_fold2x(Phase1& s, int m, const Fq& r1, const Fq& r2);
  int p1_to_compact(Phase1& s);
  NextLaunch p1_next_launch(const Phase1& s, size_t j_next, int pending) const;
  int p1_launch_next(Phase1& s, size_t j_next, int pending, const Fq& r1, const Fq& r2);
  int p1_round_single(Phase1& s, size_t j, ZFill& zf);
  int p1_round_pair(Phase1& s, size_t j, ZFill& zf);
  int run_phase1(ZFill& zf, FqV& r_all);
  void sigma1();
  int phase2_prep(ZFill& zf);
  // phase 2
  int p2_mode(size_t j) const { return j < sh.ny ? MODE_X : (j < sh.ny + sh.nw ? MODE_W : MODE_P); }
  int p2_launch_single(Phase2& s, size_t j, const Fold2* fold);
  bool p2_pair_ok(const Phase2& s, size_t j, bool fold_pending) const;
  int p2_launch_pair(Phase2& s, int nf, const Fq& r1, const Fq& r2);
  int p2_fold2x(Phase2& s, const Fq& r1, const Fq& r2);
  int p2_to_compact(Phase2& s);
  NextLaunch p2_next_launch(const Phase2& s, size_t j_next, int pending) const;
  int p2_launch_next(Phase2& s, size_t j_next, int pending, const Fq& r1, const Fq& r2);
  int p2_round_single(Phase2& s, size_t j);
  int p2_round_pair(Phase2& s, size_t j);
  int run_phase2();
  // the pair arm of both phases once the grid `ev` is in: rounds j and j + 1, with the phase's `launch_next` between
  // round j + 1's challenge and the rest of its proof; `laps`: the phase's eval / host / fold lap names
  template <class Ph>
  int round_pair_arm(Ph& s, size_t j, const Fq ev[15], const char* const laps[3],
                     int (Prover::*launch_next)(Ph&, size_t, int, const Fq&, const Fq&));
  // openings and final claims
  int lz_bound(std::vector<PolyRef>& polys, size_t lz_total, std::vector<Fq>& lz_mine);
  int witness_evals(std::vector<PolyRef>& polys, std::vector<FqV>& eval_list);
  int polyeval_batched(std::vector<PolyRef>& polys);
  void final_claims(const std::vector<FqV>& eval_list);
};

int Prover::run() {
  lp = Laps();  // the breakdown's clock starts here
  int rc0 = run_stages();
  lp.print();
  if (rc0 && nranks > 1 && !xshared && xdone < xplan.size()) {
    // this rank failed alone: the next exchange of the plan carries the failure to every rank
    std::vector<uint8_t> none(xplan[xdone], 0), r;
    xdone++;
    comm_allgather(ctx, Shard{(int)rank, (int)nranks}, rc0, none.data(), none.size(), r);
  }
  return rc0;
}

// ---- cross-rank exchange (identity when nranks == 1): comm.hpp through api.hip's comm_allgather, so every exchange
// carries this rank's status and a failure on one rank fails all of them
int Prover::exchange(const void* send, size_t bytes, std::vector<uint8_t>& recv) {
  const Shard sh{(int)rank, (int)nranks};
  if (nranks > 1 && (xdone >= xplan.size() || xplan[xdone] != bytes)) {
    // the plan is a restatement of the stages' control flow (sum_ranks in p*_round_single, gather_first in
    // p*_to_compact, the L.Z gather in witness_evals); a mismatch is a library bug
    const int rc = set_err(ctx, SPG_E_ARG, "sharded R1CSProof: exchange " + std::to_string(xdone) + " of " +
                                               std::to_string(bytes) + " bytes is not in the exchange plan");
    xshared = true;
    std::vector<uint8_t> r;
    comm_allgather(ctx, sh, rc, send, bytes, r);
    return rc;
  }
  xdone++;
  const int rc = comm_allgather(ctx, sh, 0, send, bytes, recv);
  if (rc) xshared = true;
  return rc;
}
// (e0, e2, e3) summed over the ranks' instance shards
int Prover::sum_ranks(Fq e[3]) {
  if (nranks == 1) return 0;
  std::vector<uint8_t> r;
  const int rc = exchange(e, 3 * sizeof(Fq), r);
  if (rc) return rc;
  sum_over_ranks(r.data(), (int)nranks, 3, e);
  return 0;
}
// Witness-section polynomials' L.Z widths: Rs = 2^(nv - nv/2) of each (section, instance) polynomial (the bound
// rows that the LZ allgather carries)
static size_t lz_width(size_t np, size_t ni) {
  const size_t nv = lg2(np) + lg2(ni);
  return (size_t)1 << (nv - nv / 2);
}
void Prover::plan_exchanges(size_t np, size_t nq, size_t nx, size_t nw, size_t ny) {
  xplan.clear();
  xdone = 0;
  xshared = false;
  if (nranks == 1) return;
  const size_t PL = (P + nranks - 1) / nranks, sum = 3 * sizeof(Fq);
  // phase 1: one sum per x / q round (p1_round_single), the gather of Az, Bz, Cz before the instance rounds
  // (p1_to_compact)
  const size_t r1 = nx + nq + np;
  if (r1 && nx + nq == 0) xplan.push_back(PL * 3 * sizeof(Fq));
  for (size_t j = 0; j < r1; j++) {
    if (j < nx + nq) xplan.push_back(sum);
    if (j + 1 == nx + nq && np > 0) xplan.push_back(PL * 3 * sizeof(Fq));
  }
  // phase 2: one sum per y / w round (p2_round_single), the gather of Z (and ABC unless shared) before the instance
  // rounds (p2_to_compact)
  const size_t k2 = inst.num_instances == 1 ? 1 : 2, r2 = ny + nw + np;
  if (r2 && ny + nw == 0) xplan.push_back(PL * k2 * sizeof(Fq));
  for (size_t j = 0; j < r2; j++) {
    if (j < ny + nw) xplan.push_back(sum);
    if (j + 1 == ny + nw && np > 0) xplan.push_back(PL * k2 * sizeof(Fq));
  }
  // the L.Z bounds of every witness polynomial (witness_evals)
  size_t lz_total = 0;
  for (size_t i = 0; i < nws; i++)
    for (size_t p = 0; p < wit.num_proofs[i].size(); p++) lz_total += lz_width(wit.num_proofs[i][p], wit.num_inputs[i][p]);
  xplan.push_back(lz_total * sizeof(Fq));
}
// per local instance p, the element (p, 0, 0, 0) of each table -> the same for all P instances, on the host
int Prover::gather_first(const std::vector<const PqxDev*>& tabs, std::vector<std::vector<Fq>>& full) {
  const size_t k = tabs.size(), PL = (P + nranks - 1) / nranks;  // the largest shard; slots per rank
  std::vector<Fq> mine(PL * k, fq_zero());
  {  // one gather per kSegMax elements
    std::vector<FqSeg> segs;
    std::vector<Fq*> dst;
    std::vector<Fq> got;
    auto flush = [&]() -> int {
      got.resize(segs.size());
      int rc = d2h_multi(ctx, segs.data(), (int)segs.size(), got.data());
      for (size_t j = 0; j < segs.size(); j++) *dst[j] = got[j];
      segs.clear();
      dst.clear();
      return rc;
    };
    for (size_t i = 0; i < k; i++) {
      const PqxDev& T = *tabs[i];
      for (size_t p = 0; p < T.zlen; p++) {
        segs.push_back({T.d + T.off[p], 1});
        dst.push_back(&mine[i * PL + p]);
        if (segs.size() == (size_t)kSegMax)
          if (int rc = flush()) return rc;
      }
    }
    if (!segs.empty())
      if (int rc = flush()) return rc;
  }
  std::vector<uint8_t> r;
  int rc = exchange(mine.data(), mine.size() * sizeof(Fq), r);
  if (rc) return rc;
  const Fq* v = (const Fq*)r.data();
  full.assign(k, std::vector<Fq>(P, fq_zero()));
  for (size_t q = 0; q < nranks; q++)
    for (size_t i = 0; i < k; i++)
      for (size_t b = shard_begin(P, nranks, q), p = 0; b + p < shard_begin(P, nranks, q + 1); p++)
        full[i][b + p] = v[q * PL * k + i * PL + p];
  return 0;
}

int Prover::run_stages() {
  t.protocol("R1CS proof");
  plan_exchanges(sh.np, sh.nq, sh.nx, sh.nw, sh.ny);

  ZFill zf;
  int rc = setup_tables(zf);
  if (!rc && !knob::z_side()) rc = zf.queue();
  if (rc) return rc;
  lp.lap("setup");
  cy.partials = (Fq*)ws_get(ctx, Ws::R1csPart, std::max(3 * (size_t)kScGridMax, kP1PairMax) * sizeof(Fq) + 64);
  if (!cy.partials) return set_err(ctx, SPG_E_NOMEM, "partials");
  FqV r1;  // phase 1's challenges in round order: x, q, p
  if ((rc = run_phase1(zf, r1))) return rc;
  lp.lap("p1_claims");
  const FqV rx_rev(r1.begin(), r1.begin() + sh.nx);
  cy.rq_rev.assign(r1.begin() + sh.nx, r1.begin() + sh.nx + sh.nq);
  cy.rp.assign(r1.begin() + sh.nx + sh.nq, r1.end());
  cy.rx.assign(rx_rev.rbegin(), rx_rev.rend());
  cy.rq.assign(cy.rq_rev.rbegin(), cy.rq_rev.rend());
  // eq(rx) of phase 2 depends on phase 1's challenges alone: on the device while the host runs the sigma protocols
  cy.eq_rx = (Fq*)ws_get(ctx, Ws::R1csEqRx, (sizeof(Fq) << sh.nx) + 64);
  if (!cy.eq_rx) return set_err(ctx, SPG_E_NOMEM, "eq(rx)");
  if ((rc = eq_table(ctx, cy.rx, cy.eq_rx))) return rc;
  sigma1();
  lp.lap("sigma1");
  if ((rc = phase2_prep(zf))) return rc;
  lp.lap("p2_prep");
  if ((rc = run_phase2())) return rc;
  std::vector<PolyRef> polys;
  std::vector<FqV> eval_list;
  if ((rc = witness_evals(polys, eval_list))) return rc;
  lp.lap("polyeval_bound");
  if ((rc = polyeval_batched(polys))) return rc;
  lp.lap("polyeval_dotlog");
  final_claims(eval_list);
  lp.lap("final");
  return 0;
}

// Z (p, q_rev, w, x_rev) and Az, Bz, Cz = multiply_vec_block (p, q_rev, 0, x_rev) for the local instances: shapes,
// workspace, every setup descriptor in one host-to-device copy (R1csTables), the tau eq tables, k_spmv; zf: the Z fill,
// made ready
int Prover::setup_tables(ZFill& zf) {
  int rc = tb.setup_desc(zf, true);
  if (!rc) rc = setup_tau();
  if (!rc) rc = tb.launch_spmv();
  if (!ctx->check_sat) return rc;
  // check mode (spg_set_check_sat): refuse a witness that does not satisfy the instance, naming the row. Every rank
  // holds the merged report, so all of them return here together and none waits in a later exchange; a rank whose
  // setup failed still takes part, with its failure as status.
  spg_sat_report rep;
  if ((rc = tb.sat_check(rc, &rep))) {
    if (nranks > 1) xshared = true;  // the report's allgather gave every rank this failure
    return rc;
  }
  if (!rep.violations) return 0;
  xshared = true;
  std::string msg = sat_message(rep);
  if (ctx->sat_stage) {
    if (ctx->sat_order) msg += "; block " + std::to_string(ctx->sat_order[rep.p]);
    msg = std::string(ctx->sat_stage) + ": " + msg;
  }
  return set_err(ctx, SPG_E_UNSAT, msg);
}

// ---- tau tables (identical on every rank)
int Prover::setup_tau() {
  const size_t np = sh.np, nq = sh.nq, nx = sh.nx;
  FqV tau_p = t.challenges("challenge_tau_p", np);
  FqV tau_q = t.challenges("challenge_tau_q", nq);
  FqV tau_x = t.challenges("challenge_tau_x", nx);
  if (knob::debug_tr()) fprintf(stderr, "[prove] r1cs P=%zu np=%zu nq=%zu nx=%zu tau_x0 %08x\n", (size_t)P, (size_t)np, (size_t)nq, (size_t)nx, tau_x[0].l[0]);
  cy.Ap = (Fq*)ws_get(ctx, Ws::R1csTp, (sizeof(Fq) << np) + 64);
  cy.Aq = (Fq*)ws_get(ctx, Ws::R1csTq, (sizeof(Fq) << nq) + 64);
  cy.Ax = (Fq*)ws_get(ctx, Ws::R1csTx, (sizeof(Fq) << nx) + 64);
  if (!cy.Ap || !cy.Aq || !cy.Ax) return set_err(ctx, SPG_E_NOMEM, "eq tables");
  return eq_tables(ctx, {{tau_p, cy.Ap}, {tau_q, cy.Aq}, {tau_x, cy.Ax}});
}

// ---- phase 1 (sumcheck.rs:1067-1380)
// round j's sizes: the half lengths of the reference's loop and the per-instance domain sizes of the round
int Prover::p1_advance(Phase1& s, size_t j) {
  const int mode = p1_mode(j);
  if (s.cons_len > 1) s.cons_len /= 2;
  else if (s.proof_len > 1) s.proof_len /= 2;
  else s.instance_len /= 2;
  if (mode != MODE_P)
    for (size_t p = 0; p < s.sc_np.size(); p++) {  // instance_len >= P here: every instance takes part
      if (mode == MODE_X && s.sc_nc[p] > 1) s.sc_nc[p] /= 2;
      if (mode == MODE_Q && s.sc_np[p] > 1) s.sc_np[p] /= 2;
    }
  return mode;
}
// round j's evaluation is enqueued right after round j-1's folds, so it runs on the device while the host finishes
// round j-1's proof (comm_eval, DotProductProof); eval_wait then collects (e0, e2, e3)
int Prover::p1_launch_single(Phase1& s, size_t j, const FoldPlan* fold) {
  const int mode = p1_advance(s, j);
  if (mode == MODE_P) {
    std::vector<size_t> ones(P, 1);
    return phase1_eval(ctx, *s.T, mode, s.proof_len, s.cons_len, s.instance_len, ones, ones, cy.Ap, s.Aq, s.Ax, s.T->d,
                       s.TB, s.TC, cy.partials, nullptr);
  }
  return phase1_eval(ctx, *s.T, mode, s.proof_len, s.cons_len, s.instance_len, s.sc_np, s.sc_nc, s.Ap_l, s.Aq, s.Ax,
                     s.T->d, s.TB, s.TC, cy.partials, nullptr, fold);
}
// before the first instance round: collect every instance's remaining (Az, Bz, Cz) value
int Prover::p1_to_compact(Phase1& s) {
  std::vector<std::vector<Fq>> full;
  PqxDev Bt = tb.Az, Ct = tb.Az;
  Bt.d = tb.Bz;
  Ct.d = tb.Cz;
  int rc = gather_first({&tb.Az, &Bt, &Ct}, full);
  if (rc) return rc;
  Fq* buf = (Fq*)ws_get(ctx, Ws::R1csC1, 3 * P * sizeof(Fq) + 64);
  if (!buf) return set_err(ctx, SPG_E_NOMEM, "compact tables");
  for (int i = 0; i < 3; i++)
    SPG_HIP(ctx, hipMemcpyAsync(buf + i * P, full[i].data(), P * sizeof(Fq), hipMemcpyHostToDevice, ctx->stream));
  SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  s.Ac = compact_table(buf, P, P);
  s.T = &s.Ac;
  s.TB = buf + P;
  s.TC = buf + 2 * P;
  return 0;
}
// Two rounds per launch (sumcheck.hip k_phase1_pair; SPG_P1_PAIR=0: one per launch). A pair takes rounds j, j + 1 of
// one mode (x or q) when every instance's size in that mode is >= 4 and round j + 1's domain holds at most
// SPG_P1_PAIR_MAX (default 8192) points: the latency-bound rounds. Unsharded proofs only (a sharded round sums 3
// scalars over the ranks, a pair would sum 15).
bool Prover::p1_pair_ok(const Phase1& s, size_t j) const {
  if (!knob::p1_pair() || !s.Aq2 || nranks != 1 || j + 1 >= s.rounds || s.T != &tb.Az) return false;
  const int m = p1_mode(j);
  if (m == MODE_P || p1_mode(j + 1) != m) return false;
  size_t dom = 0;
  for (size_t p = 0; p < s.sc_np.size(); p++) {
    const size_t N = m == MODE_X ? s.T->num_inputs[p] : s.T->num_proofs[p];
    const size_t Nl = m == MODE_X ? s.sc_nc[p] : s.sc_np[p];  // the round's local size before its halving
    if (N < 4 || N != Nl) return false;
    dom += m == MODE_X ? s.sc_np[p] * (N / 4) : (N / 4) * s.sc_nc[p];
  }
  return dom > 0 && dom <= p1_pair_max();
}
// rounds j, j + 1 in one launch; nf = 1: round j - 1's pending fold (fp), 2: the previous pair's (r1, r2)
int Prover::p1_launch_pair(Phase1& s, size_t j, int nf, const FoldPlan* fp, const Fq& r1, const Fq& r2) {
  const int m = p1_advance(s, j);
  P1Pair pp;
  pp.mode = m;
  pp.c = m == MODE_X ? s.cons_len : s.proof_len;  // round j's half length of the mode's eq table
  for (size_t p = 0; p < s.sc_np.size(); p++) {
    const size_t N = m == MODE_X ? s.T->num_inputs[p] : s.T->num_proofs[p];
    if (m == MODE_X) {
      pp.rows.push_back(s.sc_np[p]);
      pp.cols.push_back(N / 4);
      pp.step_x.push_back(pp.c / (N / 2));
      pp.step_q.push_back(s.proof_len / s.sc_np[p]);
    } else {
      pp.rows.push_back(N / 4);
      pp.cols.push_back(s.sc_nc[p]);
      pp.step_q.push_back(pp.c / (N / 2));
      pp.step_x.push_back(s.cons_len / s.sc_nc[p]);
    }
  }
  p1_advance(s, j + 1);
  pp.nf = nf;
  pp.r1 = r1;
  pp.r2 = r2;
  Fq*& E = m == MODE_X ? s.Ax : s.Aq;
  Fq*& Ealt = m == MODE_X ? s.Ax2 : s.Aq2;
  size_t& lenE = m == MODE_X ? s.lenX : s.lenQ;
  if (nf == 1) {
    pp.fstride = fp->stride;
    pp.fmode = fp->arg.fmode;
    pp.side_in = fp->arg.side_in;
    pp.side_out = fp->arg.side_out;
    pp.side_live = fp->arg.side_half;
  } else if (nf == 2) {  // the previous pair's folds of this mode's eq table: E (live lenE) -> Ealt (lenE / 4)
    pp.fmode = m;
    pp.side_in = E;
    pp.side_out = Ealt;
    pp.side_live = lenE / 4;
    std::swap(E, Ealt);
    lenE /= 4;
  }
  pp.Ap = s.Ap_l;
  pp.Aq = s.Aq;
  pp.Ax = s.Ax;
  pp.B = s.T->d;
  pp.C = s.TB;
  pp.D = s.TC;
  int rc = phase1_pair(ctx, *s.T, pp, cy.partials, nullptr);
  if (rc) return rc;
  // the size bookkeeping of both rounds' folds (the folds themselves ride in the next launch)
  FoldPlan tmp;
  if ((rc = pqx_fold_plan(ctx, *s.T, m, &tmp)) || (rc = pqx_fold_plan(ctx, *s.T, m, &tmp))) return rc;
  return 0;
}
// a pair's pending folds (r1, r2) on their own launch, before a single round or the instance rounds
int Prover::p1_fold2x(Phase1& s, int m, const Fq& r1, const Fq& r2) {
  P1Pair pp;
  pp.mode = m;
  for (size_t p = 0; p < s.sc_np.size(); p++) {
    pp.rows.push_back(s.T->num_proofs[p]);
    pp.cols.push_back(s.T->num_inputs[p]);
  }
  Fq*& E = m == MODE_X ? s.Ax : s.Aq;
  Fq*& Ealt = m == MODE_X ? s.Ax2 : s.Aq2;
  size_t& lenE = m == MODE_X ? s.lenX : s.lenQ;
  pp.r1 = r1;
  pp.r2 = r2;
  pp.side_in = E;
  pp.side_out = Ealt;
  pp.side_live = lenE / 4;
  pp.B = s.T->d;
  pp.C = s.TB;
  pp.D = s.TC;
  std::swap(E, Ealt);
  lenE /= 4;
  return phase1_fold2x(ctx, *s.T, pp);
}
// The launch form after round j_next - 1's challenge, `pending` folds not yet in the tables (0: the first launch; 1: a
// single round's; 2: a pair's). A single round's fold rides in the next evaluation (fused) when one follows in mode x
// or q on the same tables; a pair's two ride in another pair of its mode. Else the folds take a launch of their own
// and the compaction, when the instance rounds come next, follows it. Whether the next launch is a pair (p1_pair_ok)
// shows in the tables' sizes once a single round's fold is booked or launched: rounds = 0 until then, and the caller
// asks again with nothing pending.
NextLaunch Prover::p1_next_launch(const Phase1& s, size_t j_next, int pending) const {
  if (pending == 0) return {false, j_next >= s.rounds ? 0 : (p1_pair_ok(s, j_next) ? 2 : 1)};
  const int mode = p1_mode(j_next - 1), next_mode = p1_mode(j_next);
  if (pending == 2) {
    const bool again = j_next < s.rounds && next_mode == mode && p1_pair_ok(s, j_next);
    return {again, again ? 2 : 0};
  }
  const bool compact_next = j_next == sh.nx + sh.nq && sh.np > 0;
  return {s.Aq2 && mode != MODE_P && j_next < s.rounds && !compact_next && next_mode != MODE_P, 0};
}
// applies or books the pending folds of challenges r1 (, r2) as p1_next_launch says, then launches round j_next
int Prover::p1_launch_next(Phase1& s, size_t j_next, int pending, const Fq& r1, const Fq& r2) {
  const NextLaunch n = p1_next_launch(s, j_next, pending);
  const bool ride = n.ride;
  const int mode = pending ? p1_mode(j_next - 1) : 0;
  FoldPlan fp;
  int rc = 0;
  if (pending == 1 && ride) {  // the round's eq factor is bound in the same launch as Az, Bz, Cz
    rc = pqx_fold_plan(ctx, *s.T, mode, &fp);
    Fq*& cur = mode == MODE_Q ? s.Aq : s.Ax;
    Fq*& alt = mode == MODE_Q ? s.Aq2 : s.Ax2;
    size_t& side_len = mode == MODE_Q ? s.lenQ : s.lenX;
    fp.arg.r = r1;
    fp.arg.fmode = mode;
    fp.arg.side_in = cur;
    fp.arg.side_out = alt;
    fp.arg.side_half = (uint32_t)(side_len / 2);
    std::swap(cur, alt);
    side_len /= 2;
  } else if (pending == 1) {
    Fq* side = mode == MODE_P ? cy.Ap : (mode == MODE_Q ? s.Aq : s.Ax);
    size_t& side_len = mode == MODE_P ? s.lenP : (mode == MODE_Q ? s.lenQ : s.lenX);
    rc = pqx_bound(ctx, *s.T, s.TB, s.TC, r1, mode, side, side_len);
    side_len /= 2;
  } else if (pending == 2 && !ride) {
    rc = p1_fold2x(s, mode, r1, r2);
  }
  if (!rc && pending && !ride && j_next == sh.nx + sh.nq && sh.np > 0) rc = p1_to_compact(s);
  if (rc) return rc;
  const int nf = ride ? pending : 0;
  const int rounds = pending && !n.rounds ? p1_next_launch(s, j_next, 0).rounds : n.rounds;
  s.cur_pair = rounds == 2;
  if (rounds == 2) return p1_launch_pair(s, j_next, nf, &fp, nf ? r1 : fq_zero(), nf == 2 ? r2 : fq_zero());
  return rounds ? p1_launch_single(s, j_next, nf ? &fp : nullptr) : 0;
}
// a single round in flight: its values, its challenge, the next launch, the rest of its proof
int Prover::p1_round_single(Phase1& s, size_t j, ZFill& zf) {
  const int mode = p1_mode(j);
  Fq e[3];
  int rc = eval_wait(ctx, e);
  if (!rc && j == (size_t)knob::z_after()) rc = zf.queue();  // round j is done and round j + 1 not yet queued
  if (!rc && j == 1 && failpoint(ctx, "r1cs_round")) rc = set_err(ctx, SPG_E_HIP, "failpoint r1cs_round");
  if (!rc && mode != MODE_P) rc = sum_ranks(e);
  if (rc) return rc;
  lp.lap("p1_eval");
  const Fq r_j = s.zk.begin(g, t, j, e);
  lp.lap("p1_host");
  if ((rc = p1_launch_next(s, j + 1, 1, r_j, fq_zero()))) return rc;
  lp.lap("p1_fold");
  s.zk.finish(g, t, tape, j, r_j);
  lp.lap("p1_host");
  s.r.push_back(r_j);
  return 1;
}
// the pair arm: round j is F(X, 0) + F(X, 1) at X = 0, 2, 3; round j + 1 the cubics t -> F(t, Y) (Y = 0, 2, 3) at
// t = r_j
template <class Ph>
int Prover::round_pair_arm(Ph& s, size_t j, const Fq ev[15], const char* const laps[3],
                           int (Prover::*launch_next)(Ph&, size_t, int, const Fq&, const Fq&)) {
  lp.lap(laps[0]);
  Fq ej[3], ej1[3];
  pair_round_j(ev, ej);
  const Fq r_j = s.zk.begin(g, t, j, ej);
  s.zk.finish(g, t, tape, j, r_j);
  s.r.push_back(r_j);
  pair_round_j1(ev, r_j, ej1);
  const Fq r_j1 = s.zk.begin(g, t, j + 1, ej1);
  lp.lap(laps[1]);
  if (int rc = (this->*launch_next)(s, j + 2, 2, r_j, r_j1)) return rc;
  lp.lap(laps[2]);
  s.zk.finish(g, t, tape, j + 1, r_j1);
  lp.lap(laps[1]);
  s.r.push_back(r_j1);
  return 2;
}
int Prover::p1_round_pair(Phase1& s, size_t j, ZFill& zf) {
  static const char* const laps[3] = {"p1_eval", "p1_host", "p1_fold"};
  Fq ev[15];
  int rc = pair_wait(ctx, ev);
  if (!rc && (j == (size_t)knob::z_after() || j + 1 == (size_t)knob::z_after())) rc = zf.queue();
  if (!rc && (j == 1 || j + 1 == 1) && failpoint(ctx, "r1cs_round")) rc = set_err(ctx, SPG_E_HIP, "failpoint r1cs_round");
  if (rc) return rc;
  return round_pair_arm(s, j, ev, laps, &Prover::p1_launch_next);
}
int Prover::run_phase1(ZFill& zf, FqV& r_all) {
  const size_t nx = sh.nx, nq = sh.nq, np = sh.np;
  Phase1 s;
  s.rounds = nx + nq + np;
  s.cons_len = s.lenX = (size_t)1 << nx, s.proof_len = s.lenQ = (size_t)1 << nq;
  s.instance_len = s.lenP = (size_t)1 << np;
  s.sc_np = sh.l_proofs, s.sc_nc = sh.l_cons;
  s.T = &tb.Az, s.TB = tb.Bz, s.TC = tb.Cz;
  s.Aq = cy.Aq, s.Ax = cy.Ax, s.Ap_l = cy.Ap + p0;
  if (knob::sc_fuse()) {
    s.Aq2 = (Fq*)ws_get(ctx, Ws::R1csTq2, (sizeof(Fq) << nq) + 64);
    s.Ax2 = (Fq*)ws_get(ctx, Ws::R1csTx2, (sizeof(Fq) << nx) + 64);
    if (!s.Aq2 || !s.Ax2) return set_err(ctx, SPG_E_NOMEM, "eq tables");
  }
  int rc = s.rounds && nx + nq == 0 ? p1_to_compact(s) : 0;
  if (!rc) rc = p1_launch_next(s, 0, 0, fq_zero(), fq_zero());
  if (rc) return rc;
  s.zk.init(g, tape, s.rounds, fq_zero(), fq_zero());  // host precomputation while round 0 evaluates
  for (size_t j = 0; j < s.rounds;) {
    const int n = s.cur_pair ? p1_round_pair(s, j, zf) : p1_round_single(s, j, zf);
    if (n < 0) return n;
    j += (size_t)n;
  }
  Fq a[6];  // eq factors, then Az, Bz, Cz (a single instance: it sits on this (only) rank's local tables)
  rc = np == 0 ? d2h_multi(ctx, {{cy.Ap, 1}, {s.Aq, 1}, {s.Ax, 1}, {tb.Az.d, 1}, {tb.Bz, 1}, {tb.Cz, 1}}, a)
               : d2h_multi(ctx, {{cy.Ap, 1}, {s.Aq, 1}, {s.Ax, 1}, {s.T->d, 1}, {s.TB, 1}, {s.TC, 1}}, a);
  if (rc) return rc;
  cy.claims1[1] = a[3];
  cy.claims1[2] = a[4];
  cy.claims1[3] = a[5];
  cy.claims1[0] = fq_mul(fq_mul(a[0], a[1]), a[2]);
  cy.blind_post1 = s.zk.blinds_evals[s.rounds - 1];
  pf.sc1 = std::move(s.zk.out);
  r_all = std::move(s.r);
  return 0;
}

// the claims' blinds and commitments, and the three sigma protocols on them
void Prover::sigma1() {
  const Fq tau_claim = cy.claims1[0], Az_claim = cy.claims1[1], Bz_claim = cy.claims1[2], Cz_claim = cy.claims1[3];
  cy.Az_blind = tape.scalar("Az_blind"), cy.Bz_blind = tape.scalar("Bz_blind"), cy.Cz_blind = tape.scalar("Cz_blind");
  const Fq prod_blind = tape.scalar("prod_Az_Bz_blind");
  const Fq prod = fq_mul(Az_claim, Bz_claim);
  const Fq blind_expected1 = fq_mul(tau_claim, fq_sub(prod_blind, cy.Cz_blind));
  const Fq claim_post1 = fq_mul(fq_sub(prod, Cz_claim), tau_claim);
  Sigma1Pre sp;
  if (knob::sigma_ahead())
    sigma1_points(g, g.gens_1, tape, Cz_claim, cy.Cz_blind, Az_claim, cy.Az_blind, Bz_claim, cy.Bz_blind, prod,
                  prod_blind, claim_post1, blind_expected1, claim_post1, cy.blind_post1, &sp);
  pf.pok = knowledge_prove(g, g.gens_1, t, tape, Cz_claim, cy.Cz_blind, &cy.comm_Cz,
                           knob::sigma_ahead() ? sp.k : nullptr);
  pf.prod = product_prove(g, g.gens_1, t, tape, Az_claim, cy.Az_blind, Bz_claim, cy.Bz_blind, prod, prod_blind,
                          &cy.comm_Az, &cy.comm_Bz, &cy.comm_prod, knob::sigma_ahead() ? sp.p : nullptr);
  t.point("comm_Az_claim", cy.comm_Az);
  t.point("comm_Bz_claim", cy.comm_Bz);
  t.point("comm_Cz_claim", cy.comm_Cz);
  t.point("comm_prod_Az_Bz_claims", cy.comm_prod);
  pf.eq1 = equality_prove(g, g.gens_1, t, tape, claim_post1, blind_expected1, claim_post1, cy.blind_post1,
                          knob::sigma_ahead() ? sp.e : nullptr);
}

// phase 2's inputs: the claim, ABC = r_A A + r_B B + r_C C at rx (k_abc), Z joined and bound at rq_rev, eq(rp)
int Prover::phase2_prep(ZFill& zf) {
  const Fq r_A = t.challenge("challenge_Az"), r_B = t.challenge("challenge_Bz"), r_C = t.challenge("challenge_Cz");
  cy.claim2 = fq_add(fq_add(fq_mul(r_A, cy.claims1[1]), fq_mul(r_B, cy.claims1[2])), fq_mul(r_C, cy.claims1[3]));
  cy.blind2 = fq_add(fq_add(fq_mul(r_A, cy.Az_blind), fq_mul(r_B, cy.Bz_blind)), fq_mul(r_C, cy.Cz_blind));
  // ABC: the shared matrix once (every rank), or this rank's instances
  const size_t Ab0 = sh.single ? 0 : p0, Abn = sh.single ? 1 : sh.PLn;
  PqxDev& ABC = cy.ABC;
  ABC = pqx_shape(std::vector<size_t>(Abn, 1), nws, {num_inputs.begin() + Ab0, num_inputs.begin() + Ab0 + Abn},
                  npow2(inst.num_instances), 1, npow2(nws), Y);
  ABC.num_proofs.assign(P, 1);
  ABC.num_inputs.assign(num_inputs.begin() + Ab0, num_inputs.end());
  const size_t btot = ABC.total;
  ABC.d = (Fq*)ws_get(ctx, Ws::R1csAbc, btot * sizeof(Fq) + 64);
  if (!ABC.d) return set_err(ctx, SPG_E_NOMEM, "ABC");
  int rc = tb.launch_abc(ABC, Ab0, cy.eq_rx, r_A, r_B, r_C);
  if (!rc) rc = zf.queue();  // (phase 1 had no rounds)
  if (!rc) rc = zf.join();  // the Z table's first use
  if (rc) return rc;
  // Z.bound_poly_vars_rq(rq_rev): every q fold in one pass over Z against eq(rq_rev), or one fold launch per
  // challenge, each a read-write pass over the live rows
  const FqV& rq_rev = cy.rq_rev;
  if (knob::q_bound_all() && rq_rev.size() >= 2) {
    Fq* eq_q = (Fq*)ws_get(ctx, Ws::R1csEqQ, (sizeof(Fq) << rq_rev.size()) + 64);
    if (!eq_q) return set_err(ctx, SPG_E_NOMEM, "eq(rq)");
    rc = eq_table(ctx, rq_rev, eq_q);
    if (!rc) rc = pqx_bound_q_all(ctx, tb.Zp, eq_q, rq_rev.size());
    if (rc) return rc;
  } else {
    for (size_t k = 0; k < rq_rev.size(); k++)
      if ((rc = pqx_bound(ctx, tb.Zp, nullptr, nullptr, rq_rev[k], MODE_Q))) return rc;
  }
  cy.eq_p = (Fq*)ws_get(ctx, Ws::R1csEqP, (sizeof(Fq) << sh.np) + 64);
  if (!cy.eq_p) return set_err(ctx, SPG_E_NOMEM, "eq(rp)");
  return eq_table(ctx, cy.rp, cy.eq_p);
}

// ---- phase 2 (sumcheck.rs:788-1065)
int Prover::p2_launch_single(Phase2& s, size_t j, const Fold2* fold) {
  const int mode = p2_mode(j);
  if (s.inputs_len > 1) s.inputs_len /= 2;
  else if (s.ws_len > 1) s.ws_len /= 2;
  else s.instance_len /= 2;
  if (mode == MODE_P) {
    std::vector<size_t> ones(P, 1);
    return phase2_eval(ctx, *s.TA, *s.TZ, mode, s.instance_len, s.ws_len, nws, sh.single, ones, cy.eq_p, cy.partials,
                       nullptr);
  }
  for (size_t p = 0; p < s.sc_ni.size(); p++)
    if (mode == MODE_X && s.sc_ni[p] > 1) s.sc_ni[p] /= 2;
  return phase2_eval(ctx, *s.TA, *s.TZ, mode, s.instance_len, s.ws_len, nws, sh.single, s.sc_ni, s.eq_l, cy.partials,
                     nullptr, fold);
}
// before the first instance round: every instance's remaining Z (and ABC) value
int Prover::p2_to_compact(Phase2& s) {
  const bool single = sh.single;
  hipStream_t st = ctx->stream;
  std::vector<std::vector<Fq>> full;
  int rc = single ? gather_first({&tb.Zp}, full) : gather_first({&tb.Zp, &cy.ABC}, full);
  if (rc) return rc;
  Fq* buf = (Fq*)ws_get(ctx, Ws::R1csC2, 2 * P * sizeof(Fq) + 64);
  if (!buf) return set_err(ctx, SPG_E_NOMEM, "compact tables");
  SPG_HIP(ctx, hipMemcpyAsync(buf, full[0].data(), P * sizeof(Fq), hipMemcpyHostToDevice, st));
  if (single) {  // the shared ABC keeps its single (0,0,0,0) element
    SPG_HIP(ctx, hipMemcpyAsync(buf + P, cy.ABC.d, sizeof(Fq), hipMemcpyDeviceToDevice, st));
  } else {
    SPG_HIP(ctx, hipMemcpyAsync(buf + P, full[1].data(), P * sizeof(Fq), hipMemcpyHostToDevice, st));
  }
  SPG_HIP(ctx, hipStreamSynchronize(st));
  s.Zc = compact_table(buf, P, P);
  s.ABCc = compact_table(buf + P, single ? 1 : P, P);
  s.TZ = &s.Zc;
  s.TA = &s.ABCc;
  return 0;
}
// Two y rounds per launch (sumcheck.hip k_phase2_pair; SPG_P2_PAIR=0: one per launch): rounds j, j + 1 both y rounds,
// ABC per instance, every instance's live y size >= 4 (the same in ABC and Z), at most SPG_P2_PAIR_MAX (default 8192)
// elements, unsharded. A run of pairs starts with no fold pending (a single round's fold before it is launched on its
// own) and ends with k_phase2_fold2x.
// (fold_pending: round j - 1's fold is not yet in the tables' sizes; the caller launches it first)
bool Prover::p2_pair_ok(const Phase2& s, size_t j, bool fold_pending) const {
  const bool single = sh.single;
  const PqxDev &ABC = cy.ABC, &Zp = tb.Zp;
  // (one ABC shared by every instance folds through its ping-pong buffer, as the fused single rounds do)
  if (!knob::p2_pair() || (single && !s.ABC2) || nranks != 1 || j + 1 >= sh.ny || s.TA != &ABC || s.TZ != &Zp ||
      ABC.zlen != (single ? 1 : Zp.zlen))
    return false;
  auto live = [&](size_t n) { return fold_pending && n > 1 ? n / 2 : n; };
  size_t dom = 0;
  for (size_t p = 0; p < s.sc_ni.size(); p++) {
    const size_t N = live(Zp.num_inputs[p]);
    if (N < 4 || live(ABC.num_inputs[single ? 0 : p]) != N || s.sc_ni[p] != N) return false;
    dom += s.W2 * (N / 4);
  }
  return dom > 0 && dom <= p2_pair_max();
}
// y rounds j, j + 1 in one launch; nf = 2: the previous pair's folds (r1, r2) ride in it
int Prover::p2_launch_pair(Phase2& s, int nf, const Fq& r1, const Fq& r2) {
  for (int k = 0; k < 2; k++) {  // p2_launch_single's size bookkeeping for both y rounds
    if (s.inputs_len > 1) s.inputs_len /= 2;
    for (size_t p = 0; p < s.sc_ni.size(); p++)
      if (s.sc_ni[p] > 1) s.sc_ni[p] /= 2;
  }
  P2Pair pp;
  pp.nf = nf;
  pp.r1 = r1;
  pp.r2 = r2;
  pp.W = s.W2;
  pp.eq = s.eq_l;
  pp.B_out = sh.single ? s.ABC2 : nullptr;
  int rc = phase2_pair(ctx, cy.ABC, tb.Zp, pp, cy.partials);
  if (rc) return rc;
  if (sh.single && nf == 2) std::swap(cy.ABC.d, s.ABC2);  // the folded shared ABC is in the other buffer now
  FoldPlan tmp;  // the table bookkeeping of both rounds' folds (the folds ride in the next launch)
  for (int k = 0; k < 2 && !rc; k++) {
    rc = pqx_fold_plan(ctx, cy.ABC, MODE_X, &tmp);
    if (!rc) rc = pqx_fold_plan(ctx, tb.Zp, MODE_X, &tmp);
  }
  return rc;
}
int Prover::p2_fold2x(Phase2& s, const Fq& r1, const Fq& r2) {
  P2Pair pp;
  pp.nf = 2;
  pp.r1 = r1;
  pp.r2 = r2;
  pp.W = s.W2;
  pp.B_out = sh.single ? s.ABC2 : nullptr;
  const int rc = phase2_fold2x(ctx, cy.ABC, tb.Zp, pp);
  if (!rc && sh.single) std::swap(cy.ABC.d, s.ABC2);
  return rc;
}
// The launch form after round j_next - 1's challenge, `pending` folds not yet in the tables (as p1_next_launch). A
// pair's two folds ride in another pair; a single y round before a run of pairs folds on its own launch (the pair
// starts with nothing pending); else a single round's fold rides in the next evaluation (k_phase2_eval<true>) when
// one follows in mode y or w on the same tables.
NextLaunch Prover::p2_next_launch(const Phase2& s, size_t j_next, int pending) const {
  const int left = j_next < s.rounds ? 1 : 0;
  if (pending == 0) return {false, left && p2_pair_ok(s, j_next, false) ? 2 : left};
  if (pending == 2) {
    const bool again = j_next < sh.ny && p2_pair_ok(s, j_next, false);
    return {again, again ? 2 : left};
  }
  const int mode = p2_mode(j_next - 1);
  if (mode == MODE_X && p2_pair_ok(s, j_next, true)) return {false, 2};
  const bool compact_next = j_next == sh.ny + sh.nw && sh.np > 0;
  return {s.fuse2 && mode != MODE_P && left && !compact_next && p2_mode(j_next) != MODE_P, left};
}
// applies or books the pending folds of challenges r1 (, r2) as p2_next_launch says, then launches round j_next
int Prover::p2_launch_next(Phase2& s, size_t j_next, int pending, const Fq& r1, const Fq& r2) {
  const NextLaunch n = p2_next_launch(s, j_next, pending);
  const int mode = pending ? p2_mode(j_next - 1) : 0;
  const bool single = sh.single;
  s.cur_pair = n.rounds == 2;
  if (pending == 2 && n.ride) return p2_launch_pair(s, 2, r1, r2);
  int rc = 0;
  if (pending == 1 && n.ride) {
    Fold2 f;
    rc = pqx_fold_plan(ctx, *s.TA, mode, &f.a);
    if (!rc) rc = pqx_fold_plan(ctx, *s.TZ, mode, &f.z);
    f.arg.r = r1;
    f.arg.fmode = mode;
    f.arg.fw = f.z.fw;
    f.arg.ping = single ? 1 : 0;
    f.arg.b_out = single ? s.ABC2 : s.TA->d;
    if (!rc) rc = p2_launch_single(s, j_next, &f);
    if (!rc && single) std::swap(s.TA->d, s.ABC2);
    return rc;
  }
  if (pending == 2) {
    rc = p2_fold2x(s, r1, r2);
  } else if (pending == 1) {
    if (mode == MODE_P) {
      rc = dev_fold_top(ctx, cy.eq_p, s.lenP, r1);
      s.lenP /= 2;
    }
    if (!rc && (mode != MODE_P || !single)) rc = pqx_bound2(ctx, *s.TA, *s.TZ, r1, mode);
    else if (!rc) rc = pqx_bound(ctx, *s.TZ, nullptr, nullptr, r1, mode);
  }
  if (!rc && pending && j_next == sh.ny + sh.nw && sh.np > 0) rc = p2_to_compact(s);
  if (rc) return rc;
  if (n.rounds == 2) return p2_launch_pair(s, 0, fq_zero(), fq_zero());
  return n.rounds ? p2_launch_single(s, j_next, nullptr) : 0;
}
int Prover::p2_round_single(Phase2& s, size_t j) {
  Fq e[3];
  int rc = eval_wait(ctx, e);
  if (!rc && p2_mode(j) != MODE_P) rc = sum_ranks(e);
  if (rc) return rc;
  lp.lap("p2_eval");
  const Fq r_j = s.zk.begin(g, t, j, e);
  lp.lap("p2_host");
  if ((rc = p2_launch_next(s, j + 1, 1, r_j, fq_zero()))) return rc;
  lp.lap("p2_fold");
  s.zk.finish(g, t, tape, j, r_j);
  lp.lap("p2_host");
  s.r.push_back(r_j);
  return 1;
}
int Prover::p2_round_pair(Phase2& s, size_t j) {
  static const char* const laps[3] = {"p2_eval", "p2_host", "p2_fold"};
  Fq ev[15];
  if (int rc = pair_wait(ctx, ev)) return rc;
  return round_pair_arm(s, j, ev, laps, &Prover::p2_launch_next);
}
int Prover::run_phase2() {
  const size_t ny = sh.ny, nw = sh.nw, np = sh.np;
  Phase2 s;
  s.rounds = ny + nw + np;
  s.inputs_len = (size_t)1 << ny, s.ws_len = (size_t)1 << nw, s.instance_len = s.lenP = (size_t)1 << np;
  s.sc_ni = sh.l_inputs;
  s.TZ = &tb.Zp, s.TA = &cy.ABC;
  s.eq_l = cy.eq_p + p0;
  s.W2 = std::min(s.ws_len, nws);
  // one ABC serving every instance is folded into ABC2 by a fused round (then the two swap). The fused fold writes it
  // from the points of local instance 0 (global p0): only when that instance spans ABC's whole width (num_inputs[0])
  // -- a sharded rank whose first instance is narrower takes the separate fold
  s.fuse2 = knob::sc_fuse() && (!sh.single || num_inputs[p0] == num_inputs[0]);
  if (s.fuse2 && sh.single) {
    s.ABC2 = (Fq*)ws_get(ctx, Ws::R1csAbc2, cy.ABC.total * sizeof(Fq) + 64);
    if (!s.ABC2) return set_err(ctx, SPG_E_NOMEM, "ABC");
  }
  int rc = s.rounds && ny + nw == 0 ? p2_to_compact(s) : 0;
  if (!rc) rc = p2_launch_next(s, 0, 0, fq_zero(), fq_zero());
  if (rc) return rc;
  s.zk.init(g, tape, s.rounds, cy.claim2, cy.blind2);  // host precomputation while round 0 evaluates
  for (size_t j = 0; j < s.rounds;) {
    const int n = s.cur_pair ? p2_round_pair(s, j) : p2_round_single(s, j);
    if (n < 0) return n;
    j += (size_t)n;
  }
  rc = d2h_multi(ctx, {{cy.eq_p, 1}, {s.TA->d, 1}, {s.TZ->d, 1}}, cy.claims2);
  if (rc) return rc;
  cy.blind_post2 = s.zk.blinds_evals[s.rounds - 1];
  pf.sc2 = std::move(s.zk.out);
  cy.ry.assign(s.r.rbegin() + (nw + np), s.r.rend());  // the y challenges, reversed
  cy.rw.assign(s.r.begin() + ny, s.r.begin() + ny + nw);
  cy.rp2.assign(s.r.begin() + ny + nw, s.r.end());
  return 0;
}

// ---- witness-section evaluations and their batched opening (r1csproof.rs:518-639)
// R = eq(rr) of every polynomial, once per distinct right point (instances of one shape share theirs), on the pool
static void right_tables(std::vector<PolyRef>& polys, const std::vector<FqV>& rr_of) {
  std::vector<size_t> uniq, at(polys.size());
  for (size_t k = 0; k < polys.size(); k++) {
    size_t u = 0;
    while (u < uniq.size() && !(rr_of[uniq[u]].size() == rr_of[k].size() &&
                                memcmp(rr_of[uniq[u]].data(), rr_of[k].data(), rr_of[k].size() * sizeof(Fq)) == 0))
      u++;
    if (u == uniq.size()) uniq.push_back(k);
    at[k] = u;
  }
  std::vector<FqV> tabs(uniq.size());
  pool().parallel_for((int)uniq.size(), [&](int u) { tabs[u] = eq_evals_host(rr_of[uniq[u]]); });
  for (size_t k = 0; k < polys.size(); k++) polys[k].R = tabs[at[k]];
}
// LZ = bound(L) of each owned polynomial on this rank's device (lz_mine, zero elsewhere). Every polynomial's eq(rl),
// partial column sums and LZ are queued back to back into disjoint workspace ranges and the LZ of all of them come
// back in one download (one host wait instead of one per polynomial). The host eq tables of the right points are
// computed while the device works (queued first; d2h_fq waits for it).
int Prover::lz_bound(std::vector<PolyRef>& polys, size_t lz_total, std::vector<Fq>& lz_mine) {
  const size_t nq = sh.nq, ny = sh.ny;
  hipStream_t st = ctx->stream;
  struct BoundJob {
    FqV rl;
    size_t Ls, Rs, S, chunk, offL, offP, o;
  };
  std::vector<BoundJob> jobs;
  size_t o = 0, totL = 0, totP = 0;
  bool all_mine = true;
  std::vector<FqV> rr_of(polys.size());  // each polynomial's right point
  size_t pk = 0;
  for (auto& pr : polys) {
    size_t lnp = lg2(pr.np), lni = lg2(pr.ni);
    FqV r(cy.rq.begin() + (nq - lnp), cy.rq.end());
    if (pr.ni >= Y) {
      r.insert(r.end(), lni - ny, fq_zero());
      r.insert(r.end(), cy.ry.begin(), cy.ry.end());
    } else {
      r.insert(r.end(), cy.ry.begin() + (ny - lni), cy.ry.end());
    }
    size_t nv = r.size(), ln = nv / 2;
    FqV rl(r.begin(), r.begin() + ln), rr(r.begin() + ln, r.end());
    size_t Ls = (size_t)1 << ln, Rs = (size_t)1 << (nv - ln);
    rr_of[pk++] = std::move(rr);
    if (pr.mine) {
      size_t S = std::min<size_t>(Ls, 32);  // 32 partial rows: short column sums
      const size_t chunk = (Ls + S - 1) / S;
      S = (Ls + chunk - 1) / chunk;
      jobs.push_back({std::move(rl), Ls, Rs, S, chunk, totL, totP, o});
      totL += Ls;
      totP += S * Rs;
    } else {
      all_mine = false;
    }
    o += Rs;
  }
  if (jobs.empty()) {
    right_tables(polys, rr_of);
    return 0;
  }
  Fq* dL = (Fq*)ws_get(ctx, Ws::R1csL, totL * sizeof(Fq) + 64);
  Fq* dpart = (Fq*)ws_get(ctx, Ws::R1csBoundPart, totP * sizeof(Fq) + 64);
  Fq* dout = (Fq*)ws_get(ctx, Ws::R1csBoundOut, lz_total * sizeof(Fq) + 64);
  if (!dL || !dpart || !dout) return set_err(ctx, SPG_E_NOMEM, "bound");
  if (!all_mine) SPG_HIP(ctx, hipMemsetAsync(dout, 0, lz_total * sizeof(Fq), st));  // other ranks' ranges
  // one eq table per distinct rl (polynomials of one shape share it)
  std::vector<size_t> eq_at(jobs.size());
  std::vector<EqJob> eqs;
  for (size_t k = 0; k < jobs.size(); k++) {
    size_t same = k;
    for (size_t m = 0; m < k; m++)
      if (jobs[m].rl.size() == jobs[k].rl.size() &&
          memcmp(jobs[m].rl.data(), jobs[k].rl.data(), jobs[k].rl.size() * sizeof(Fq)) == 0) {
        same = m;
        break;
      }
    eq_at[k] = same == k ? jobs[k].offL : eq_at[same];
    if (same == k) eqs.push_back({jobs[k].rl.data(), (int)jobs[k].rl.size(), dL + jobs[k].offL});
  }
  int rc = dev_eq_tables(ctx, eqs.data(), (int)eqs.size());
  if (rc) return rc;
  std::vector<const PolyRef*> mine;
  for (auto& pr : polys)
    if (pr.mine) mine.push_back(&pr);
  std::vector<BoundBatch> batches;
  for (size_t k0 = 0; k0 < jobs.size(); k0 += kBoundMax) {
    BoundBatch b;
    BoundJobs& bj = b.jobs;
    bj.n = (int)std::min<size_t>(kBoundMax, jobs.size() - k0);
    uint32_t nb = 0, nc = 0;
    for (int q = 0; q < bj.n; q++) {
      const BoundJob& j = jobs[k0 + q];
      const PolyRef& pr = *mine[k0 + q];
      const uint32_t nbx = (uint32_t)((j.Rs + 255) / 256);
      bj.d[q] = {wit.ptr[pr.w][pr.p], (uint32_t)eq_at[k0 + q], (uint32_t)j.Ls, (uint32_t)j.Rs,
                 (uint32_t)j.chunk, (uint32_t)j.S, (uint32_t)j.offP, (uint32_t)j.o, nb, nc};
      nb += nbx * (uint32_t)j.S;
      nc += (uint32_t)((j.Rs + kSumCols - 1) / kSumCols);
    }
    b.nb = nb, b.nc = nc;
    batches.push_back(b);
  }
  launch_bound(ctx, batches, dL, dpart, dout);
  SPG_HIP(ctx, hipGetLastError());
  right_tables(polys, rr_of);
  return d2h_fq(ctx, dout, lz_mine.data(), lz_total);
}
// every witness polynomial's evaluation at (rq, ry): LZ from its owner shared with every rank, <LZ, R>, commitments
int Prover::witness_evals(std::vector<PolyRef>& polys, std::vector<FqV>& eval_list) {
  const size_t ny = sh.ny;
  FqV ry_factors(ny + 1, fq_one());
  for (size_t i = 0; i < ny; i++) ry_factors[i + 1] = fq_mul(ry_factors[i], fq_sub(fq_one(), cy.ry[i]));
  size_t lz_total = 0;
  for (size_t i = 0; i < nws; i++) {
    for (size_t p = 0; p < wit.num_proofs[i].size(); p++) {
      PolyRef pr;
      pr.w = i;
      pr.p = p;
      pr.np = wit.num_proofs[i][p];
      pr.ni = wit.num_inputs[i][p];
      pr.Rs = lz_width(pr.np, pr.ni);
      pr.mine = wit.num_proofs[i].size() == 1 ? rank == 0 : (p >= p0 && p < p1);
      lz_total += pr.Rs;
      polys.push_back(std::move(pr));
    }
  }
  std::vector<Fq> lz_mine(lz_total, fq_zero());
  int rc = lz_bound(polys, lz_total, lz_mine);
  if (rc) return rc;
  {
    std::vector<uint8_t> r;
    rc = exchange(lz_mine.data(), lz_total * sizeof(Fq), r);
    if (rc) return rc;
    const Fq* v = (const Fq*)r.data();
    size_t o = 0;
    for (auto& pr : polys) {
      size_t owner = 0;
      if (wit.num_proofs[pr.w].size() != 1) owner = owner_of(pr.p);
      pr.LZ.assign(v + owner * lz_total + o, v + owner * lz_total + o + pr.Rs);
      o += pr.Rs;
    }
  }
  // (both lists end with nws trailing empty lists, as the reference's do: verify.hip relies on it)
  eval_list.assign(nws, {});
  pf.comm_vars_at_ry_list.assign(nws, {});
  size_t k = 0;
  std::vector<CJob> cj;  // every evaluation's commitment in one host burst
  // <LZ, R> of every polynomial, one pool task each
  pool().parallel_for((int)polys.size(), [&](int q) {
    PolyRef& pr = polys[q];
    Fq ev = fq_zero();
    for (size_t m = 0; m < pr.Rs; m++) ev = fq_add(ev, fq_mul(pr.LZ[m], pr.R[m]));
    pr.ev = ev;
  });
  for (size_t i = 0; i < nws; i++) {
    eval_list.push_back({});
    for (size_t p = 0; p < wit.num_proofs[i].size(); p++, k++) {
      PolyRef& pr = polys[k];
      const Fq ev = pr.ev;
      size_t lni = lg2(pr.ni);
      eval_list[i].push_back(pr.ni >= Y ? ev : fq_mul(ev, ry_factors[ny - lni]));
      cj.push_back(CJob(g.gens_1, {ev}, fq_zero()));
    }
  }
  const std::vector<Pt> cv = commit_batch(g, cj);
  k = 0;
  for (size_t i = 0; i < nws; i++) {
    pf.comm_vars_at_ry_list.push_back({});
    for (size_t p = 0; p < wit.num_proofs[i].size(); p++) pf.comm_vars_at_ry_list[i].push_back(cv[k++]);
  }
  return 0;
}
// PolyEvalProof::prove_batched_instances_disjoint_rounds (dense_mlpoly.rs:861-960)
int Prover::polyeval_batched(std::vector<PolyRef>& polys) {
  t.protocol("polynomial evaluation proof");
  std::vector<std::pair<size_t, size_t>> shape;
  for (const PolyRef& pr : polys) shape.push_back({pr.np, pr.ni});
  const PeWalk wk = pe_walk_disjoint(shape);
  const FqV c = pe_coeff_powers(t.challenge("challenge_c"), wk.repeats());
  // the coefficients in the reference's order (the walk of pe_plan.hpp), then every LZ_list[k] += c LZ over the pool
  // (axpy_pool; config 4 adds 7 x 1024 products here, ~170 us on one thread)
  const size_t D = wk.first.size();
  std::vector<FqV> LZ_list(D), R_list(D);
  FqV Zc(D);
  std::vector<Axpy> ax;
  for (size_t q = 0; q < polys.size(); q++) {
    const PolyRef& pr = polys[q];
    const size_t k = wk.group[q];
    if (wk.opens(q)) {
      LZ_list[k] = pr.LZ, R_list[k] = pr.R, Zc[k] = pr.ev;
    } else {
      ax.push_back({&LZ_list[k], c[wk.exp[q]], &pr.LZ});
      Zc[k] = fq_add(Zc[k], fq_mul(c[wk.exp[q]], pr.ev));
    }
  }
  axpy_pool(ax);
  for (size_t k = 0; k < LZ_list.size(); k++) {
    DotProductProofLogP dp;
    Pt comm;
    int rc = dotproduct_log_prove(ctx, g, t, tape, LZ_list[k], fq_zero(), R_list[k], Zc[k], fq_zero(), &dp, &comm);
    if (rc) return rc;
    pf.evals.push_back(std::move(dp));
  }
  return 0;
}
// prefix_list (r1csproof.rs:577-606), the combined evaluation, the last equality proof and the returned challenges
void Prover::final_claims(const std::vector<FqV>& eval_list) {
  const FqV& rw = cy.rw;
  FqV prefix;
  {
    Fq one = fq_one();
    size_t W2 = npow2(nws);
    if (W2 == 1) prefix = {one};
    else if (W2 == 2) prefix = {fq_sub(one, rw[0]), rw[0]};
    else if (W2 == 4)
      prefix = {fq_mul(fq_sub(one, rw[0]), fq_sub(one, rw[1])), fq_mul(fq_sub(one, rw[0]), rw[1]),
                fq_mul(rw[0], fq_sub(one, rw[1])), fq_mul(rw[0], rw[1])};
    else
      for (int i = 0; i < 8; i++) {
        Fq a = (i & 4) ? rw[0] : fq_sub(one, rw[0]);
        Fq b = (i & 2) ? rw[1] : fq_sub(one, rw[1]);
        Fq cc = (i & 1) ? rw[2] : fq_sub(one, rw[2]);
        prefix.push_back(fq_mul(fq_mul(a, b), cc));
      }
  }
  FqV comb_list;
  for (size_t p = 0; p < P; p++) {
    Fq comb = fq_zero();
    for (size_t i = 0; i < nws; i++) {
      size_t pw = wit.num_proofs[i].size() == 1 ? 0 : p;
      comb = fq_add(comb, fq_mul(prefix[i], eval_list[i][pw]));
    }
    for (size_t q = 0; q < sh.nq - lg2(num_proofs[p]); q++) comb = fq_mul(comb, fq_sub(fq_one(), cy.rq[q]));
    comb_list.push_back(comb);
  }
  Fq eval_vars_at_ry = dense_eval_host(comb_list, cy.rp2);
  pf.comm_vars_at_ry = commit_batch(g, {CJob(g.gens_1, {eval_vars_at_ry}, fq_zero())})[0];
  Fq claim_post2 = fq_mul(fq_mul(cy.claims2[0], cy.claims2[1]), cy.claims2[2]);
  pf.eq2 = equality_prove(g, g.gens_1, t, tape, claim_post2, fq_zero(), claim_post2, cy.blind_post2);
  pf.claims_phase2[0] = cy.comm_Az;
  pf.claims_phase2[1] = cy.comm_Bz;
  pf.claims_phase2[2] = cy.comm_Cz;
  pf.claims_phase2[3] = cy.comm_prod;
  FqV rwry(rw);
  rwry.insert(rwry.end(), cy.ry.begin(), cy.ry.end());
  challenges = {cy.rp2, cy.rq_rev, cy.rx, rwry};
}


}  // namespace spg

using namespace spg;

// argument check of spg_r1cs_prove; also derives this rank's instance shard [p0, p1)
static int check_prove_args(spg_ctx* ctx, const spg_r1cs_inst* inst, size_t num_instances, size_t max_num_proofs,
                            const size_t* num_proofs, size_t max_num_inputs, const size_t* num_inputs,
                            const spg_r1cs_witness* wit, size_t rank, size_t nranks, size_t* p0, size_t* p1) {
  if (!num_instances || !is_pow2(max_num_proofs) || !is_pow2(max_num_inputs))
    return set_err(ctx, SPG_E_ARG, "bad sizes");
  if (inst->num_instances != 1 && inst->num_instances != num_instances)
    return set_err(ctx, SPG_E_ARG, "instance count mismatch");
  if (wit->nws * max_num_inputs > inst->num_vars) return set_err(ctx, SPG_E_ARG, "witness wider than num_vars");
  for (size_t p = 0; p < num_instances; p++) {
    if (!is_pow2(num_proofs[p]) || num_proofs[p] > max_num_proofs || !is_pow2(num_inputs[p]) ||
        num_inputs[p] > max_num_inputs)
      return set_err(ctx, SPG_E_ARG, "num_proofs / num_inputs must be powers of two within the maxima");
  }
  for (size_t w = 0; w < wit->nws; w++) {
    if (wit->num_proofs[w].size() != 1 && wit->num_proofs[w].size() != num_instances)
      return set_err(ctx, SPG_E_ARG, "witness section instance count mismatch");
    for (size_t p = 0; p < num_instances; p++) {
      size_t pw = wit->num_proofs[w].size() == 1 ? 0 : p;
      if (wit->num_proofs[w][pw] != 1 && wit->num_proofs[w][pw] < num_proofs[p])
        return set_err(ctx, SPG_E_ARG, "witness section has fewer rows than num_proofs");
      if (wit->num_proofs[w][pw] > max_num_proofs) return set_err(ctx, SPG_E_ARG, "witness section too tall");
    }
  }
  if (nranks > num_instances) return set_err(ctx, SPG_E_ARG, "more ranks than instances");
  *p0 = Prover::shard_begin(num_instances, nranks, rank);
  *p1 = Prover::shard_begin(num_instances, nranks, rank + 1);
  for (size_t w = 0; w < wit->nws; w++) {
    if (wit->num_proofs[w].size() == 1) continue;
    for (size_t p = *p0; p < *p1; p++)
      if (wit->off[w][p] == kNotResident) return set_err(ctx, SPG_E_ARG, "witness shard does not hold instance");
  }
  return SPG_OK;
}

// the argument check on every rank, then the checked sizes with this rank's instances; shared by spg_r1cs_prove and
// spg_r1cs_sat_check
static int prover_args(spg_ctx* ctx, R1csSizes& sz, const spg_r1cs_inst* inst, size_t num_instances,
                       size_t max_num_proofs, const size_t* num_proofs, size_t max_num_inputs,
                       const size_t* num_inputs, const spg_r1cs_witness* wit) {
  const size_t rank = (size_t)ctx->rank, nranks = (size_t)ctx->nranks;
  int rc_args = check_prove_args(ctx, inst, num_instances, max_num_proofs, num_proofs, max_num_inputs, num_inputs,
                                 wit, rank, nranks, &sz.p0, &sz.p1);
  if (nranks > 1) {
    // a sharded prove starts with every rank agreeing on the argument check, so a rank-local failure
    // (e.g. a witness shard that does not hold this rank's instances) fails every rank alike instead of
    // leaving the others blocked in the first round's allgather
    int32_t mine = rc_args;
    std::vector<uint8_t> all;
    int rc = comm_allgather(ctx, Shard{(int)rank, (int)nranks}, 0, &mine, sizeof(mine), all);
    if (rc) return rc;
    for (size_t q = 0; q < nranks && !rc_args; q++)
      if (((const int32_t*)all.data())[q]) rc_args = set_err(ctx, SPG_E_ARG, "a peer rank rejected its arguments");
  }
  if (rc_args) return rc_args;
  sz.P = num_instances;
  sz.max_np = max_num_proofs;
  sz.Y = max_num_inputs;
  sz.nws = wit->nws;
  sz.num_proofs.assign(num_proofs, num_proofs + num_instances);
  sz.num_inputs.assign(num_inputs, num_inputs + num_instances);
  return SPG_OK;
}

static int r1cs_prove_impl(spg_ctx* ctx, const spg_r1cs_gens* gens, const spg_r1cs_inst* inst,
                           size_t num_instances, size_t max_num_proofs, const size_t* num_proofs,
                           size_t max_num_inputs, const size_t* num_inputs, const spg_r1cs_witness* wit,
                           spg_transcript* transcript, spg_random_tape* tape, uint8_t* proof, size_t proof_cap,
                           size_t* proof_len, uint64_t* challenges_out, size_t* ch_lens) {
  R1csSizes sz;
  int rc = prover_args(ctx, sz, inst, num_instances, max_num_proofs, num_proofs, max_num_inputs, num_inputs, wit);
  if (rc) return rc;
  Prover pr(ctx, const_cast<spg_r1cs_gens*>(gens)->g, *inst, *wit, transcript->t, tape->t, sz);
  timer_start(ctx);
  rc = pr.run();
  timer_stop(ctx);
  if (rc == SPG_E_UNSAT) *proof_len = 0;  // check mode: no proof was written
  if (rc) return rc;
  Writer wr;
  pr.pf.ser(wr);
  *proof_len = wr.out.size();
  if (challenges_out && ch_lens) {
    size_t k = 0;
    for (int i = 0; i < 4; i++) {
      ch_lens[i] = pr.challenges[i].size();
      for (auto& c : pr.challenges[i]) st_fq(challenges_out + 4 * k++, c);
    }
  }
  if (!proof || wr.out.size() > proof_cap) return set_err(ctx, SPG_E_ARG, "proof buffer too small");
  memcpy(proof, wr.out.data(), wr.out.size());
  return SPG_OK;
}

extern "C" int spg_r1cs_prove(spg_ctx* ctx, const spg_r1cs_gens* gens, const spg_r1cs_inst* inst,
                              size_t num_instances, size_t max_num_proofs, const size_t* num_proofs,
                              size_t max_num_inputs, const size_t* num_inputs, const spg_r1cs_witness* wit,
                              spg_transcript* transcript, spg_random_tape* tape, uint8_t* proof, size_t proof_cap,
                              size_t* proof_len, uint64_t* challenges_out, size_t* ch_lens) {
  if (!ctx || !gens || !inst || !num_proofs || !num_inputs || !wit || !transcript || !tape || !proof_len)
    return SPG_E_ARG;
  HostPin pin;
  TrFailScope tfs(ctx, transcript->t);
  return tr_status(ctx, transcript->t,
                   r1cs_prove_impl(ctx, gens, inst, num_instances, max_num_proofs, num_proofs, max_num_inputs, num_inputs,
                                   wit, transcript, tape, proof, proof_cap, proof_len, challenges_out, ch_lens));
}

// R1CSInstance::is_sat (src/r1csinstance.rs:322-357) over every execution of every instance: the prover's own table
// setup (R1csTables: descriptors and k_spmv, no Z fill), then k_sat_check (satcheck.hip). A collective under
// spg_set_comm, as spg_r1cs_prove.
extern "C" int spg_r1cs_sat_check(spg_ctx* ctx, const spg_r1cs_inst* inst, size_t num_instances, size_t max_num_proofs,
                                  const size_t* num_proofs, size_t max_num_inputs, const size_t* num_inputs,
                                  const spg_r1cs_witness* wit, spg_sat_report* out) {
  if (!ctx || !inst || !num_proofs || !num_inputs || !wit || !out) return SPG_E_ARG;
  R1csSizes sz;
  int rc = prover_args(ctx, sz, inst, num_instances, max_num_proofs, num_proofs, max_num_inputs, num_inputs, wit);
  if (rc) return rc;
  R1csTables tb(ctx, *inst, *wit, sz);
  ZFill zf;
  rc = tb.setup_desc(zf, false);
  if (!rc) rc = tb.launch_spmv();
  return tb.sat_check(rc, out);
}
