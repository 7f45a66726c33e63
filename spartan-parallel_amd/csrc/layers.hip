// spg — product circuits and their batched layer sumchecks on device vectors (spark.hip and prodc.hip drive these
// through prodc.hpp).
//
//   ProductCircuit::new / evaluate               src/product_tree.rs:36-58              tree_build: k_tree_level, k_tree_top
//   DotProductCircuit::evaluate                  :110-180                               dotp_evaluate: k_dot3
//   ProductCircuitEvalProofBatched::prove        :271-396                               batched_prove
//   SumcheckInstanceProof::prove_cubic_batched   src/sumcheck.rs:264-434                cubic_layer; k_layer_* (layer.hpp)
//
// Tree layout: circuit c at c * 2M; its levels v_0 (the M leaves), v_1, .. v_{L-1} (2 entries) back to back at offset
// 2M - 2(M >> k). Layer k of the circuit is (left, right) = the two halves of v_k, and v_{k+1}[i] = v_k[i] * v_k[i + |v_k|/2].
#include <algorithm>
#include <array>

#include "hostpoly.hpp"
#include "knobs.hpp"
#include "proto.hpp"
#include "layer.hpp"
#include "msm_plan.hpp"
#include "sumcheck.hpp"

namespace spg {

// ------------------------------------------------------------------------------------ kernels
__global__ void k_scale(Fq* __restrict__ v, size_t n, Fq s) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] = fq_mul(v[i], s);
}
// v_{k+1}[i] = v_k[i] * v_k[i + half] for every circuit (circuit stride 2M)
__global__ void k_tree_level(Fq* __restrict__ tree, size_t nc, size_t stride, size_t off_k, size_t off_k1, int log_half) {
  const size_t half = (size_t)1 << log_half;
  size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nc * half) return;
  size_t c = t >> log_half, i = t & (half - 1);
  Fq* v = tree + c * stride;
  v[off_k1 + i] = fq_mul(v[off_k + i], v[off_k + i + half]);
}
// The levels of every circuit's tree from level k0 up, and its top product, in one launch: workgroup c builds circuit c's
// levels (each level's products read the level below, which this workgroup wrote: a barrier between levels) -- the
// small top levels would otherwise be one launch each, ~3 us of work behind a ~4 us launch
__global__ void __launch_bounds__(256) k_tree_top(Fq* __restrict__ tree, size_t stride, int log_m, int k0,
                                                  Fq* __restrict__ tops) {
  Fq* v = tree + blockIdx.x * stride;
  const size_t M = (size_t)1 << log_m;
  for (int k = k0; k + 1 < log_m; k++) {
    const size_t ok = 2 * M - 2 * (M >> k), ok1 = 2 * M - 2 * (M >> (k + 1)), half = M >> (k + 1);
    for (size_t i = threadIdx.x; i < half; i += 256) v[ok1 + i] = fq_mul(v[ok + i], v[ok + i + half]);
    __syncthreads();
  }
  if (threadIdx.x == 0) tops[blockIdx.x] = fq_mul(v[2 * M - 4], v[2 * M - 3]);
}
// ProductCircuit::evaluate of every circuit: product of the top level's two entries
__global__ void k_tops(const Fq* __restrict__ tree, size_t nc, size_t stride, size_t off, Fq* __restrict__ out) {
  size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c < nc) out[c] = fq_mul(tree[c * stride + off], tree[c * stride + off + 1]);
}

// DotProductCircuit::evaluate per triple: sum_i A*B*C over n entries (blockIdx.y = triple)
__global__ void __launch_bounds__(256) k_dot3(const Triple* __restrict__ tr, size_t n, Fq* __restrict__ partials) {
  const Triple x = tr[blockIdx.y];
  Fq acc = fq_zero(), z = fq_zero(), z2 = fq_zero();
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    acc = fq_add(acc, fq_mul(fq_mul(x.A[i], x.B[i]), x.C[i]));
  block_sum3_sp(acc, z, z2);
  if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// UniPoly::append_to_transcript (unipoly.rs:112-120)
static void append_unipoly(Tr& t, const FqV& c) {
  t.msg("poly", "UniPoly_begin");
  for (auto& x : c) t.scalar("coeff", x);
  t.msg("poly", "UniPoly_end");
}

// ------------------------------------------------------------------------------------ trees and dot products
int tree_build(spg_ctx* ctx, Fq* tree, size_t nc, size_t M, Fq* tops) {
  hipStream_t s = ctx->stream;
  KScope ks(ctx, "spark_product_tree", 96.0 * nc * M / 2);
  // levels of more than kTopHalf products per circuit: one grid-wide launch each; the rest and the tops: k_tree_top
  const size_t kTopHalf = (size_t)knob::tree_top();
  size_t k = 0;
  for (; k + 1 < lg2(M) && (M >> (k + 1)) > kTopHalf; k++) {
    size_t ok = 2 * M - 2 * (M >> k), ok1 = 2 * M - 2 * (M >> (k + 1));
    hipLaunchKernelGGL(k_tree_level, dim3(nblk(nc * (M >> (k + 1)))), dim3(256), 0, s, tree, nc, 2 * M, ok, ok1,
                       (int)lg2(M >> (k + 1)));
  }
  if (kTopHalf) {
    hipLaunchKernelGGL(k_tree_top, dim3((unsigned)nc), dim3(256), 0, s, tree, 2 * M, (int)lg2(M), (int)k, tops);
  } else {
    for (; k + 1 < lg2(M); k++) {
      size_t ok = 2 * M - 2 * (M >> k), ok1 = 2 * M - 2 * (M >> (k + 1));
      hipLaunchKernelGGL(k_tree_level, dim3(nblk(nc * (M >> (k + 1)))), dim3(256), 0, s, tree, nc, 2 * M, ok, ok1,
                         (int)lg2(M >> (k + 1)));
    }
    const size_t top = 2 * M - 4;  // v_{L-1}
    hipLaunchKernelGGL(k_tops, dim3(nblk(nc)), dim3(256), 0, s, tree, nc, 2 * M, top, tops);
  }
  SPG_HIP(ctx, hipGetLastError());
  return 0;
}

int dotp_evaluate(spg_ctx* ctx, const std::vector<Triple>& dotp, size_t n, Fq* out) {
  const size_t nd = dotp.size();
  if (!nd) return 0;
  Triple* dtr = (Triple*)ws_get(ctx, Ws::LayerTriples, 3 * nd * sizeof(Triple) + 64);
  unsigned nb = (unsigned)std::min<size_t>(nblk(n), std::max<size_t>(1, 2048 / nd));
  Fq* part = (Fq*)ws_get(ctx, Ws::SegPart, nd * nb * sizeof(Fq) + 64);
  Fq* dres = (Fq*)ws_get(ctx, Ws::Seg, nd * sizeof(Fq) + 64);
  if (!dtr || !part || !dres) return set_err(ctx, SPG_E_NOMEM, "dotp eval");
  SPG_HIP(ctx, hipMemcpyAsync(dtr, dotp.data(), nd * sizeof(Triple), hipMemcpyHostToDevice, ctx->stream));
  KScope ks(ctx, "spark_dotp_eval", 96.0 * nd * n);
  hipLaunchKernelGGL(k_dot3, dim3(nb, (unsigned)nd), dim3(256), 0, ctx->stream, dtr, n, part);
  hipLaunchKernelGGL(k_sum_seg, dim3((unsigned)nd), dim3(256), 0, ctx->stream, part, (int)nb, dres);
  SPG_HIP(ctx, hipGetLastError());
  return d2h_fq(ctx, dres, out, nd);
}

// workgroups and block size of a fused layer round over W = nt * len elements: one workgroup up to kOneWgMax
// elements (no ticket), else about kEltPerThread elements per thread over 256-thread workgroups
static void layer_grid(size_t W, unsigned* K, int* BS) {
  layer_grid(W, (size_t)knob::layer_onewg(), (size_t)knob::layer_ept(), K, BS);  // msm_plan.hpp
}

// ------------------------------------------------------------------------------------ the layer prover
// ProductCircuitEvalProofBatched::prove (product_tree.rs:271-396): batched_prove below walks the layers; per layer
// layer_setup uploads the descriptors, run_rounds asks plan_step for the next launch form (round_single, round_pair,
// round_triple, then layer_close when no launch posted the final entries) and layer_finals appends the claims.

// (the launch forms' switches: knobs.hpp) what the launch plan asks in every cell of its table, read once: the two
// switches, the size from which a round takes the throughput form, and the limits the buffers put on the launches.
// A paired launch of E elements (16 lanes each) stores 16 partials per workgroup of BSp / 16 elements into `part` (3 x
// 2048 scalars): 16 E / BSp * 16 <= 6144, so E <= 6144 with 256-thread workgroups and E <= 1536 with 64-thread ones;
// a tripled launch takes a wave per element, four per workgroup, 64 partials per workgroup
struct LayerLimits {
  bool pair_on = knob::layer_pair(), triple_on = knob::layer_triple();
  size_t wide_min = (size_t)knob::wide_min();
  size_t pair_max = std::min<size_t>((size_t)knob::pair_max(), knob::pair_bs() == 64 ? 1536 : 6144);
  size_t triple_max = std::min<size_t>((size_t)knob::triple_max(), 384);
};

// The launch plan. Two rounds in one launch (k_layer_pair): small rounds of an unsharded layer (`multi`), every
// element's 16 lanes within pair_max elements, the last pair's corners within the mailbox; three (k_layer_triple): a
// wave per element within triple_max elements, the last triple's corners within the mailbox. nt triples in ngroups
// thread groups; k rounds left.
static bool pair_ok(const LayerLimits& lim, size_t nt, size_t ngroups, bool multi, size_t k) {
  return lim.pair_on && multi && k >= 2 && (nt << (k - 2)) <= lim.pair_max && 15 + 12 * nt <= kMboxScalars &&
         ngroups * ((size_t)1 << (k - 1)) < lim.wide_min;
}
static bool triple_ok(const LayerLimits& lim, size_t nt, size_t ngroups, bool multi, size_t k) {
  return lim.triple_on && multi && k >= 3 && (nt << (k - 3)) <= lim.triple_max && 64 + 24 * nt <= kMboxScalars &&
         ngroups * ((size_t)1 << (k - 1)) < lim.wide_min;
}
// Single rounds first, then pairs, then triples (a pair leaves two pending folds, which only a pair or a triple
// applies; a triple three, which only a triple applies), the cheapest by step_cost. Returns the rounds of the first
// launch from k rounds left with `npend` folds pending, 0 when no plan finishes the layer.
static int plan_step(size_t nt, size_t ngroups, bool multi, size_t k, int npend) {
  const int inf = 1 << 28, mode = npend >= 3 ? 2 : (npend == 2 ? 1 : 0);  // 0: free, 1: after a pair, 2: after a triple
  static const LayerLimits lim;
  static const knob::StepCosts cost = knob::step_costs();
  std::vector<std::array<int, 3>> best(k + 1), first(k + 1);
  for (size_t j = 0; j <= k; j++)
    for (int md = 0; md < 3; md++) {
      int b = j == 0 ? 0 : inf, f = 0;
      if (j >= 1 && md == 0 && best[j - 1][0] < inf && cost.c[0] + best[j - 1][0] < b)
        b = cost.c[0] + best[j - 1][0], f = 1;
      if (md <= 1 && pair_ok(lim, nt, ngroups, multi, j) && best[j - 2][1] < inf && cost.c[1] + best[j - 2][1] < b)
        b = cost.c[1] + best[j - 2][1], f = 2;
      if (triple_ok(lim, nt, ngroups, multi, j) && best[j - 3][2] < inf && cost.c[2] + best[j - 3][2] < b)
        b = cost.c[2] + best[j - 3][2], f = 3;
      best[j][md] = b;
      first[j][md] = f;
    }
  return first[k][mode];
}

// what stays fixed over a prove's layers
struct LayerEnv {
  spg_ctx* ctx;
  Tr& t;
  const Shard& sh;
  Laps& lp;
  size_t nc;         // product circuits: triples 0 .. nc-1 share the eq vector
  Fq* cbuf[2];       // the shared eq vector's ping-pong pair
  uint8_t* ddesc;    // the layer's triples, then (at tr_bytes) their coefficients
  size_t tr_bytes;
  Fq* part;          // the ticketed reductions' partials (3 x 2048 scalars)
  Fq* gbuf;          // sharded: the gathered entries
  size_t W;          // ranks the trees are sharded over
  int rank;
  const Triple* dtr() const { return (const Triple*)ddesc; }
  const Fq* dcoef() const { return (const Fq*)(ddesc + tr_bytes); }
};
// a layer's sumcheck as it goes
struct LayerState {
  size_t nt = 0, ngroups = 0;  // triples; thread groups (the product circuits share one thread per index)
  int cur = 0;                 // the buffer holding the shared eq vector C
  // bound_poly_var_top's not yet applied, with r[0], then r[1], then r[2]: one after a single round, two after a
  // paired launch (which only a pair or a triple applies), three after a tripled one (which only a triple applies)
  int npend = 0;
  Fq r[3] = {fq_zero(), fq_zero(), fq_zero()};
  Fq e = fq_zero();  // the running claim
  FqV r_prod;        // the layer's challenges
  LayerProofP proof;
  bool shared = false;  // a failure returned from an exchange: every rank has it
};

// the host half of a round: UniPoly from (e0, e2, e3), transcript, r_j
static Fq host_round(const LayerEnv& E, LayerState& S, const Fq ev[3]) {
  Fq evals[4] = {ev[0], fq_sub(S.e, ev[0]), ev[1], ev[2]};
  FqV poly = uni_from_evals3(evals);
  append_unipoly(E.t, poly);
  Fq r_j = E.t.challenge("challenge_nextround");
  S.r_prod.push_back(r_j);
  S.e = uni_eval(poly, r_j);
  S.proof.polys.push_back({poly[0], poly[2], poly[3]});
  return r_j;
}

// A[0], B[0], C[0] of every triple (after the pending fold, if any), by mailbox
static int layer_close(const LayerEnv& E, LayerState& S, FqV& fin) {
  spg_ctx* ctx = E.ctx;
  if (S.npend > 1) return set_err(ctx, SPG_E_ARG, "layer close after a paired round");  // (the last pair posts its ends)
  fin.resize(3 * S.nt);
  KScope ks(ctx, "spark_layer_close");
  const uint32_t seq = ++ctx->mbox_seq;
  hipLaunchKernelGGL(k_layer_close, dim3(1), dim3(256), 0, ctx->stream, E.dtr(), (int)S.nt, S.npend, S.r[0],
                     E.cbuf[S.cur], ctx->d_mbox, seq);
  SPG_HIP(ctx, hipGetLastError());
  S.npend = 0;
  return mbox_wait(ctx, seq, fin.data(), (int)fin.size());
}

// One round in one launch, 2^log_len entries per vector. `local`: the round's sums are added over the ranks. *done:
// the layer's last round in one workgroup also posted every vector's two entries and `fin` holds the final claims.
static int round_single(const LayerEnv& E, LayerState& S, size_t log_len, bool local, bool close_after, FqV* fin,
                        bool* done) {
  spg_ctx* ctx = E.ctx;
  hipStream_t s = ctx->stream;
  if (S.npend > 1) return set_err(ctx, SPG_E_ARG, "single layer round after a paired one");
  log_len--;
  const size_t len = (size_t)1 << log_len, nt = S.nt, ngroups = S.ngroups, nc = E.nc;
  const bool pending = S.npend == 1, wide = ngroups * len >= (size_t)knob::wide_min();
  const Triple* dtr = E.dtr();
  const Fq* dcoef = E.dcoef();
  Fq *cin = E.cbuf[S.cur], *cout = E.cbuf[S.cur ^ 1];
  unsigned K;
  int BS;
  // algorithmic HBM bytes of the round: per distinct vector (A, B of every triple; the shared C once; each
  // dot-product circuit's own C) and index, 2 entries read, or with the pending fold 4 read + 2 written
  const double layer_bytes = (pending ? 192.0 : 64.0) * (double)len * (double)(2 * nt + ngroups);
  if (wide) {  // throughput form for rounds that fill the chip
    K = (unsigned)std::min<size_t>((ngroups * len + 255) / 256, 2048);
    // Fq products per index: per product circuit k A B at 3 points from the folded A, B (3 + 2 + 4 folds), the
    // shared C folded once (2) and multiplied in (3); a dot-product circuit 14 (its own C folded too)
    const double fqm_w = (double)len * ((pending ? 2.0 : 0.0) + 3.0 + (double)nc * (pending ? 9.0 : 5.0) +
                                        (double)(nt - nc) * (pending ? 14.0 : 8.0));
    KScope ks(ctx, "spark_layer_round", layer_bytes, 0.0, fqm_w);
    hipLaunchKernelGGL(k_layer_round_wide<256>, dim3(K), dim3(256), 0, s, dtr, dcoef, (int)nc, (int)nt, (int)log_len,
                       pending ? 1 : 0, S.r[0], cin, cout, E.part, ctx->d_counter, ctx->d_mbox, ++ctx->mbox_seq);
  } else if (knob::layer_quad()) {  // a quad per element, about one element per quad
    const size_t Wd = nt * len;
    BS = Wd <= 16 ? 64 : 256;
    K = (unsigned)std::min<size_t>((Wd * 4 + BS - 1) / BS, 2048);
  } else {
    layer_grid(nt * len, &K, &BS);
  }
  // the layer's last round in one workgroup also posts every vector's two entries: the host then folds the
  // final claims with the round's challenge, and no close launch (another round trip) follows
  const bool ends =
      close_after && log_len == 0 && knob::layer_quad() && K == 1 && 3 + 6 * nt <= kMboxScalars && !wide &&
      knob::layer_ends();
  if (!wide) {
    // Fq products per element: lanes 0..2 fold their vector's two entries (6) and form k A B C at their point (9)
    KScope ks(ctx, "spark_layer_round", layer_bytes, 0.0, (double)nt * (double)len * (pending ? 15.0 : 9.0));
    const int lg = (int)log_len, df = pending ? 1 : 0;
    const uint32_t seq = ++ctx->mbox_seq;
    if (knob::layer_quad() && BS == 64)
      hipLaunchKernelGGL(k_layer_round_q<64>, dim3(K), dim3(64), 0, s, dtr, dcoef, (int)nt, lg, df, S.r[0], cin, cout,
                         E.part, ctx->d_counter, ctx->d_mbox, seq, nullptr, ends ? 1 : 0);
    else if (knob::layer_quad())
      hipLaunchKernelGGL(k_layer_round_q<256>, dim3(K), dim3(256), 0, s, dtr, dcoef, (int)nt, lg, df, S.r[0], cin, cout,
                         E.part, ctx->d_counter, ctx->d_mbox, seq, nullptr, ends ? 1 : 0);
    else if (BS == 64)
      hipLaunchKernelGGL(k_layer_round<64>, dim3(K), dim3(64), 0, s, dtr, dcoef, (int)nt, lg, df, S.r[0], cin, cout,
                         E.part, ctx->d_counter, ctx->d_mbox, seq, nullptr);
    else
      hipLaunchKernelGGL(k_layer_round<256>, dim3(K), dim3(256), 0, s, dtr, dcoef, (int)nt, lg, df, S.r[0], cin, cout,
                         E.part, ctx->d_counter, ctx->d_mbox, seq, nullptr);
  }
  if (pending) S.cur ^= 1;
  FqV ev(ends ? 3 + 6 * nt : 3);
  const hipError_t le = hipGetLastError();
  int rc = le != hipSuccess ? set_err(ctx, SPG_E_HIP, std::string("layer round: ") + hipGetErrorString(le))
                            : mbox_wait(ctx, ctx->mbox_seq, ev.data(), (int)ev.size());
  if (local) {
    rc = comm_sum_fq(ctx, E.sh, rc, ev.data(), 3);
    if (rc) S.shared = true;
  }
  if (rc) return rc;
  E.lp.lap("round_eval_wait");
  S.r[0] = host_round(E, S, ev.data());
  S.npend = 1;
  E.lp.lap("round_host");
  if (ends) {  // bound_poly_var_top of the length-2 vectors, on the host
    fin->resize(3 * nt);
    for (size_t c = 0; c < 3 * nt; c++) {
      const Fq lo = ev[3 + 2 * c], hi = ev[4 + 2 * c];
      (*fin)[c] = fq_add(lo, fq_mul(S.r[0], fq_sub(hi, lo)));
    }
    S.npend = 0;
    *done = true;
  }
  return 0;
}

// Two rounds in one launch (k_layer_pair), from 2^log_len entries per vector. *done: these were the layer's last
// rounds, the launch posted every vector's 2 x 2 corners and `fin` holds the final claims.
static int round_pair(const LayerEnv& E, LayerState& S, size_t log_len, FqV* fin, bool* done) {
  spg_ctx* ctx = E.ctx;
  if (S.npend > 2) return set_err(ctx, SPG_E_ARG, "paired layer round after a tripled one");
  const int lgj = (int)log_len - 1;  // round j's half length 2^lgj; round j + 1's 2^(lgj - 1)
  const size_t nt = S.nt, h = (size_t)1 << (lgj - 1), lanes = 16 * nt * h;
  const int BSp = lanes <= 64 || knob::pair_bs() == 64 ? 64 : 256;
  const unsigned Kp = (unsigned)((lanes + BSp - 1) / BSp);
  const bool ends = log_len == 2;  // the layer's last pair posts every vector's 2 x 2 corners
  const int nf = S.npend;
  PairArgs P;
  P.tr = E.dtr();
  P.coeff = E.dcoef();
  P.nt = (int)nt;
  P.log_len = lgj;
  P.nf = nf;
  P.r1 = S.r[0];
  P.r2 = S.r[1];
  P.r12 = fq_mul(S.r[0], S.r[1]);
  P.cin = E.cbuf[S.cur];
  P.cout = E.cbuf[S.cur ^ 1];
  P.partials = E.part;
  P.counter = ctx->d_counter;
  P.mb = ctx->d_mbox;
  P.seq = ++ctx->mbox_seq;
  P.ends = ends ? 1 : 0;
  P.probe = nullptr;
  {
    // algorithmic bytes: per distinct vector and element, 4 corners from 4 2^nf entries, written back when folded
    const double per = 32.0 * (4.0 * (double)(1 << nf) + (nf ? 4.0 : 0.0));
    // Fq products per element: the corners folded (12 x 3 with two pending folds, 12 with one), 15 points x 3
    KScope ks(ctx, "spark_layer_pair", per * (double)h * (double)(2 * nt + S.ngroups), 0.0,
              (double)nt * (double)h * (45.0 + (nf == 2 ? 36.0 : nf == 1 ? 12.0 : 0.0)));
    if (BSp == 64)
      hipLaunchKernelGGL(k_layer_pair<64>, dim3(Kp), dim3(64), 0, ctx->stream, P);
    else
      hipLaunchKernelGGL(k_layer_pair<256>, dim3(Kp), dim3(256), 0, ctx->stream, P);
  }
  if (nf) S.cur ^= 1;
  FqV ev(15 + (ends ? 12 * nt : 0));
  const hipError_t le = hipGetLastError();
  E.lp.lap(ends ? "pair_launch_end" : "pair_launch");
  const int rc = le != hipSuccess ? set_err(ctx, SPG_E_HIP, std::string("layer pair: ") + hipGetErrorString(le))
                                  : mbox_wait(ctx, P.seq, ev.data(), (int)ev.size());
  if (rc) return rc;
  E.lp.lap(ends ? "pair_wait_end" : "pair_wait");
  Fq ej[3], ej1[3];  // (the grid's layout and its decoding: hostmath.hpp)
  pair_round_j(ev.data(), ej);
  const Fq rj = host_round(E, S, ej);
  pair_round_j1(ev.data(), rj, ej1);
  const Fq rj1 = host_round(E, S, ej1);
  E.lp.lap("pair_host");
  if (ends) {  // the 2 x 2 cube of every vector folded at (r_j, r_j+1): the layer's final claims
    fin->resize(3 * nt);
    for (size_t c = 0; c < 3 * nt; c++) (*fin)[c] = fold_corners2(&ev[15 + 4 * c], rj, rj1);  // vector c % 3 of triple c / 3
    S.npend = 0;
    E.lp.lap("pair_fin");
    *done = true;
    return 0;
  }
  S.npend = 2;
  S.r[0] = rj;
  S.r[1] = rj1;
  return 0;
}

// Three rounds in one launch (k_layer_triple), from 2^log_len entries per vector. *done: these were the layer's last
// rounds, the launch posted every vector's 2 x 2 x 2 corners and `fin` holds the final claims.
static int round_triple(const LayerEnv& E, LayerState& S, size_t log_len, FqV* fin, bool* done) {
  spg_ctx* ctx = E.ctx;
  const int lgj = (int)log_len - 1;  // round j's half length 2^lgj; h = 2^(lgj - 2) elements per vector
  const size_t nt = S.nt, h = (size_t)1 << (lgj - 2), El = nt * h;
  const int BSt = El <= 1 ? 64 : 256;
  const unsigned Kt = (unsigned)((El + BSt / 64 - 1) / (BSt / 64));
  const bool ends = log_len == 3;  // the layer's last triple posts every vector's 2 x 2 x 2 corners
  const int nf = S.npend;
  TripleArgs P;
  P.tr = E.dtr();
  P.coeff = E.dcoef();
  P.nt = (int)nt;
  P.log_len = lgj;
  P.nf = nf;
  P.r1 = S.r[0];
  P.r2 = S.r[1];
  P.r3 = S.r[2];
  P.r12 = fq_mul(S.r[0], S.r[1]);
  P.r13 = fq_mul(S.r[0], S.r[2]);
  P.r23 = fq_mul(S.r[1], S.r[2]);
  P.r123 = fq_mul(P.r12, S.r[2]);
  P.cin = E.cbuf[S.cur];
  P.cout = E.cbuf[S.cur ^ 1];
  P.partials = E.part;
  P.counter = ctx->d_counter;
  P.mb = ctx->d_mbox;
  P.seq = ++ctx->mbox_seq;
  P.ends = ends ? 1 : 0;
  P.probe = nullptr;
  {
    // algorithmic bytes: per distinct vector and element, 8 corners from 8 2^nf entries, written back when folded
    const double per = 32.0 * (8.0 * (double)(1 << nf) + (nf ? 8.0 : 0.0));
    // Fq products per element: the 24 corners folded (2^nf - 1 each), 64 points x 3
    KScope ks(ctx, "spark_layer_triple", per * (double)h * (double)(2 * nt + S.ngroups), 0.0,
              (double)nt * (double)h * (192.0 + 24.0 * (double)((1 << nf) - 1)));
    if (BSt == 64)
      hipLaunchKernelGGL(k_layer_triple<64>, dim3(Kt), dim3(64), 0, ctx->stream, P);
    else
      hipLaunchKernelGGL(k_layer_triple<256>, dim3(Kt), dim3(256), 0, ctx->stream, P);
  }
  if (nf) S.cur ^= 1;
  FqV ev(64 + (ends ? 24 * nt : 0));  // F(t, s, u) = ev[t + 4 s + 16 u], then the corners
  const hipError_t le = hipGetLastError();
  E.lp.lap(ends ? "triple_launch_end" : "triple_launch");
  const int rc = le != hipSuccess ? set_err(ctx, SPG_E_HIP, std::string("layer triple: ") + hipGetErrorString(le))
                                  : mbox_wait(ctx, P.seq, ev.data(), (int)ev.size());
  if (rc) return rc;
  E.lp.lap(ends ? "triple_wait_end" : "triple_wait");
  Fq ej[3], ej1[3], ej2[3], L[4], M[4];  // (the grid's layout and its decoding: hostmath.hpp)
  triple_round_j(ev.data(), ej);
  const Fq rj = host_round(E, S, ej);
  lagrange4(rj, L);
  triple_round_j1(ev.data(), L, ej1);
  const Fq rj1 = host_round(E, S, ej1);
  lagrange4(rj1, M);
  triple_round_j2(ev.data(), L, M, ej2);
  const Fq rj2 = host_round(E, S, ej2);
  E.lp.lap("triple_host");
  if (ends) {  // the 2 x 2 x 2 cube of every vector folded at (r_j, r_j+1, r_j+2): the layer's final claims
    fin->resize(3 * nt);
    auto fold3 = [&](size_t c0, size_t c1) {
      for (size_t c = c0; c < c1; c++) (*fin)[c] = fold_corners3(&ev[64 + 8 * c], rj, rj1, rj2);  // vector c % 3 of triple c / 3
    };
    // 7 products per vector: 500 for 24 circuits, ~8 us on one core; spread over the pool from 48 vectors
    const size_t nv = 3 * nt;
    const int K = nv >= 48 ? (int)std::min<size_t>(nv / 16, (size_t)pool().size() + 1) : 1;
    if (K == 1)
      fold3(0, nv);
    else
      pool().parallel_for(K, [&](int k) { fold3(nv * k / K, nv * (k + 1) / K); });
    S.npend = 0;
    E.lp.lap("triple_fin");
    *done = true;
    return 0;
  }
  S.npend = 3;
  S.r[0] = rj;
  S.r[1] = rj1;
  S.r[2] = rj2;
  return 0;
}

// Rounds while the vectors (2^log_len entries here) have more than one entry; `local` rounds sum over the ranks; with
// close_after the layer's (or the shard's) final entries follow in `fin`. status: this rank already failed (skip mode).
static int run_rounds(const LayerEnv& E, LayerState& S, size_t log_len, bool local, bool close_after, FqV* fin,
                      int status) {
  if (status) {  // the first local round's exchange carries the failure to every rank
    if (!local || log_len == 0) return status;
    Fq none[3] = {fq_zero(), fq_zero(), fq_zero()};
    S.shared = true;
    return comm_sum_fq(E.ctx, E.sh, status, none, 3);
  }
  const bool multi = knob::layer_quad() && !local && close_after;
  while (log_len > 0) {
    const int step = plan_step(S.nt, S.ngroups, multi, log_len, S.npend);
    if (step == 0) return set_err(E.ctx, SPG_E_ARG, "layer rounds: no launch plan");
    bool done = false;
    const int rc = step == 3   ? round_triple(E, S, log_len, fin, &done)
                   : step == 2 ? round_pair(E, S, log_len, fin, &done)
                               : round_single(E, S, log_len, local, close_after, fin, &done);
    if (rc) return rc;
    if (done) return 0;
    log_len -= (size_t)step;
  }
  return close_after ? layer_close(E, S, *fin) : 0;
}

// A layer's descriptors and eq vector. The triples and coefficients ride in the eq-table launch's arguments when they
// fit (no copy command on the stream), through page-locked staging otherwise; the eq table goes to cbuf[0]. `sharded`:
// the local eq share, eq(rand)[W i' + r] = eq(rand_hi)[i'] * eq(rand_lo)[r], of hl entries. rc: skip mode.
static int layer_setup(const LayerEnv& E, const std::vector<Triple>& tr, const FqV& coeffs, const FqV& rand,
                       bool sharded, size_t hl, int rc) {
  spg_ctx* ctx = E.ctx;
  KBlob blob;  // 2.3 KB on the stack (contexts on other threads prove concurrently)
  const size_t blob_bytes = E.tr_bytes + coeffs.size() * sizeof(Fq);
  const bool in_args = blob_bytes <= sizeof(blob.w) && !knob::layer_desc_copy();
  if (in_args) {
    memset(blob.w, 0, E.tr_bytes);
    memcpy(blob.w, tr.data(), tr.size() * sizeof(Triple));
    memcpy((uint8_t*)blob.w + E.tr_bytes, coeffs.data(), coeffs.size() * sizeof(Fq));
    blob.nwords = (int)(blob_bytes / 4);
  } else if (!rc) {  // free again here (the previous layer ended with a mailbox wait after its last launch)
    uint8_t* st = (uint8_t*)pinned_get(ctx, blob_bytes + 64);
    if (!st) {
      rc = set_err(ctx, SPG_E_NOMEM, "layer staging");
    } else {
      memcpy(st, tr.data(), tr.size() * sizeof(Triple));
      memcpy(st + E.tr_bytes, coeffs.data(), coeffs.size() * sizeof(Fq));
      if (hipMemcpyAsync(E.ddesc, st, blob_bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = set_err(ctx, SPG_E_HIP, "layer descriptors upload");
    }
  }
  const KBlob* bp = in_args ? &blob : nullptr;
  if (rc) return rc;  // skip mode: no device work this layer
  if (!sharded) return dev_eq_table(ctx, rand.data(), (int)rand.size(), E.cbuf[0], bp, E.ddesc);
  const size_t lgW = lg2(E.W), nh = rand.size() - lgW;
  rc = dev_eq_table(ctx, rand.data(), (int)nh, E.cbuf[0], bp, E.ddesc);
  Fq sc = fq_one();
  for (size_t k = 0; k < lgW; k++)
    sc = fq_mul(sc, ((E.rank >> (lgW - 1 - k)) & 1) ? rand[nh + k] : fq_sub(fq_one(), rand[nh + k]));
  if (!rc) hipLaunchKernelGGL(k_scale, dim3(nblk(hl)), dim3(256), 0, ctx->stream, E.cbuf[0], hl, sc);
  return rc;
}

// After a sharded layer's local rounds every vector has one entry per rank left (`mine`: this rank's, rank q's entry
// is global index q): gathers them, and points the triples at the W gathered entries of each vector for the
// replicated rounds. rc: skip mode. A failure of the exchange is known to every rank (S.shared).
static int layer_gather(const LayerEnv& E, LayerState& S, std::vector<Triple>& tr, FqV& mine, int rc) {
  spg_ctx* ctx = E.ctx;
  hipStream_t s = ctx->stream;
  const size_t nt = tr.size(), W = E.W;
  mine.resize(3 * nt, fq_zero());
  std::vector<uint8_t> all;
  rc = comm_allgather(ctx, E.sh, rc, mine.data(), 3 * nt * sizeof(Fq), all);
  if (rc) {
    S.shared = true;
    return rc;
  }
  const Fq* g = (const Fq*)all.data();
  uint8_t* st = (uint8_t*)pinned_get(ctx, 3 * nt * W * sizeof(Fq) + E.tr_bytes + 64);
  if (!st) return set_err(ctx, SPG_E_NOMEM, "gather staging");
  Fq* hv = (Fq*)(st + E.tr_bytes);
  for (size_t c = 0; c < nt; c++)
    for (size_t k = 0; k < 3; k++)
      for (size_t q = 0; q < W; q++) hv[(3 * c + k) * W + q] = g[q * 3 * nt + 3 * c + k];
  Fq* gbuf = E.gbuf;
  for (size_t c = 0; c < nt; c++) {
    const bool own_c = tr[c].C != nullptr;
    tr[c] = {gbuf + 3 * c * W, gbuf + (3 * c + 1) * W, own_c ? gbuf + (3 * c + 2) * W : nullptr};
  }
  memcpy(st, tr.data(), nt * sizeof(Triple));
  if (hipMemcpyAsync(E.ddesc, st, nt * sizeof(Triple), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(gbuf, hv, 3 * nt * W * sizeof(Fq), hipMemcpyHostToDevice, s) != hipSuccess ||
      // the product circuits' shared eq vector (every product triple gathered the same entries)
      (E.nc && hipMemcpyAsync(E.cbuf[S.cur], gbuf + 2 * W, W * sizeof(Fq), hipMemcpyDeviceToDevice, s) != hipSuccess))
    return set_err(ctx, SPG_E_HIP, "gathered entries upload");
  return 0;
}

// The layer's final claims fin = (A[0], B[0], C[0]) per triple into the proof and the transcript (ndotp dot-product
// circuits after the nc product circuits); returns challenge_r_layer
static Fq layer_finals(const LayerEnv& E, LayerState& S, const FqV& fin, size_t ndotp, BatchedProofP* out) {
  const size_t nc = E.nc;
  Tr& t = E.t;
  for (size_t c = 0; c < nc; c++) {
    S.proof.left.push_back(fin[3 * c]);
    S.proof.right.push_back(fin[3 * c + 1]);
  }
  for (size_t c = 0; c < nc; c++) {
    t.scalar("claim_prod_left", S.proof.left[c]);
    t.scalar("claim_prod_right", S.proof.right[c]);
  }
  if (ndotp) {
    for (size_t k = 0; k < ndotp; k++)
      for (int i = 0; i < 3; i++) out->dotp[i].push_back(fin[3 * (nc + k) + i]);
    for (size_t k = 0; k < ndotp; k++) {
      t.scalar("claim_dotp_left", out->dotp[0][k]);
      t.scalar("claim_dotp_right", out->dotp[1][k]);
      t.scalar("claim_dotp_weight", out->dotp[2][k]);
    }
  }
  return t.challenge("challenge_r_layer");
}

// the workspace of a prove's layers: nt_max triples, eq vectors of up to c_len entries, trees sharded over W ranks
static int layer_env_init(LayerEnv& E, size_t nt_max, size_t c_len, size_t W, int rank) {
  spg_ctx* ctx = E.ctx;
  E.cbuf[0] = (Fq*)ws_get(ctx, Ws::LayerC, std::max(c_len, W) * sizeof(Fq) + 64);
  E.cbuf[1] = (Fq*)ws_get(ctx, Ws::LayerC2, std::max(c_len, W) * sizeof(Fq) + 64);
  // triples, then their coefficients, in one buffer (one upload per layer)
  E.tr_bytes = (nt_max * sizeof(Triple) + 63) & ~(size_t)63;
  E.ddesc = (uint8_t*)ws_get(ctx, Ws::LayerTriples, E.tr_bytes + nt_max * sizeof(Fq) + 64);
  E.part = (Fq*)ws_get(ctx, Ws::LayerPart, 3 * 2048 * sizeof(Fq) + 64);  // K <= 2048 workgroups per round
  E.gbuf = W > 1 ? (Fq*)ws_get(ctx, Ws::LayerGather, 3 * nt_max * W * sizeof(Fq) + 64) : nullptr;
  E.W = W;
  E.rank = rank;
  if (!E.cbuf[0] || !E.cbuf[1] || !E.ddesc || !E.part || (W > 1 && !E.gbuf))
    return set_err(ctx, SPG_E_NOMEM, "batched_prove");
  return 0;
}

// ProductCircuitEvalProofBatched::prove (product_tree.rs:271-396) over the nc product circuits of `ts` (M leaves
// each, claims = their ProductCircuit::evaluate) and, at layer 0, the dot-product circuits `dotp` (three device
// vectors of M/2 entries each, folded in place) with claims `dotp_claims`. Every launch applies the folds pending
// from the launch before it and evaluates one to three rounds (layer.hpp).
// A layer whose vectors are sharded (global half length >= W) runs its first lg(half / W) rounds on the local
// shares (pairs (i, i + len) stay on one rank while W | len; the round's (e0, e2, e3) are summed over the ranks),
// then gathers the W remaining entries of every vector (k_layer_close without the fold when no round ran) and
// runs the last lg W rounds replicated, exactly like an unsharded layer of that length.
int batched_prove(spg_ctx* ctx, const TreeSh& ts, size_t nc, size_t M, FqV claims, const std::vector<Triple>& dotp,
                  const FqV& dotp_claims, Tr& t, BatchedProofP* out, FqV* rand_out, const Shard& sh) {
  const size_t L = lg2(M), W = (size_t)ts.W, lgW = lg2(W), m = ts.m, lgm = lg2(m);
  auto off = [](size_t MM, size_t k) { return 2 * MM - 2 * (MM >> k); };
  const size_t nt_max = nc + dotp.size();
  if (3 * nt_max + 1 > kMboxScalars) return set_err(ctx, SPG_E_ARG, "batched_prove: too many circuits for the mailbox");
  const size_t half_max = std::max<size_t>(M / 2 / W, 1);  // the longest eq vector held here
  Laps lp;
  lp.title = "ProductCircuitEvalProofBatched::prove";
  LayerEnv E{ctx, t, sh, lp, nc};
  if (int rc = layer_env_init(E, nt_max, half_max, W, ts.r)) return rc;
  FqV rand;
  // W > 1: a failure on this rank alone (allocation, HIP, mailbox) is not returned at once -- the peers would wait
  // in the next exchange. The rank stops working (`fail`, skip mode) but keeps the exchange sequence, whose
  // shape depends only on public sizes, until its status reaches every rank: in the next sharded round's
  // exchange, or in the status exchange that ends the function. A failure learned in an exchange is known to
  // every rank (LayerState::shared) and returns at once.
  int fail = 0;
  for (size_t layer = L; layer-- > 0;) {
    const size_t half = M >> (layer + 1);  // |left| = |right| = |C| (global)
    // where this layer's vectors live: local shares (sharded), the replicated top tree, or the whole tree
    const bool sharded = W > 1 && layer < lgm;
    const size_t hl = sharded ? half / W : half;  // entries of each vector held here
    int rc = fail;
    if (!rc && sharded && failpoint(ctx, "spark_layer")) rc = set_err(ctx, SPG_E_HIP, "failpoint spark_layer");
    const bool with_dotp = layer == 0 && !dotp.empty();
    std::vector<Triple> tr;
    for (size_t c = 0; c < nc; c++) {
      Fq* v = sharded || W == 1 ? ts.loc + c * 2 * m + off(m, layer) : ts.top + c * 2 * W + off(W, layer - lgm);
      tr.push_back({v, v + hl, nullptr});  // C: the shared eq vector
    }
    if (with_dotp) {
      claims.insert(claims.end(), dotp_claims.begin(), dotp_claims.end());
      for (auto& d : dotp) tr.push_back(d);
    }
    FqV coeffs = t.challenges("rand_coeffs_next_layer", claims.size());
    LayerState S;
    S.nt = tr.size();
    S.ngroups = (nc ? 1 : 0) + (tr.size() - nc);
    for (size_t i = 0; i < claims.size(); i++) S.e = fq_add(S.e, fq_mul(claims[i], coeffs[i]));
    rc = layer_setup(E, tr, coeffs, rand, sharded, hl, rc);
    if (rc && W == 1) return rc;
    lp.lap("layer_setup");
    FqV fin;
    if (sharded) {
      FqV mine;
      rc = run_rounds(E, S, lg2(hl), true, true, &mine, rc);
      if (rc && S.shared) return rc;
      rc = layer_gather(E, S, tr, mine, rc);
      if (rc && S.shared) return rc;
      rc = run_rounds(E, S, lgW, false, true, &fin, rc);
    } else {
      rc = run_rounds(E, S, lg2(hl), false, true, &fin, rc);
    }
    if (rc && (W == 1 || S.shared)) return rc;
    if (rc) {  // this rank alone: skip mode until an exchange carries it
      fail = rc;
      continue;
    }
    const Fq r_layer = layer_finals(E, S, fin, with_dotp ? dotp.size() : 0, out);
    const LayerProofP& lpf = S.proof;
    claims.assign(nc, fq_zero());
    for (size_t c = 0; c < nc; c++) claims[c] = fq_add(lpf.left[c], fq_mul(r_layer, fq_sub(lpf.right[c], lpf.left[c])));
    rand.assign(1, r_layer);
    rand.insert(rand.end(), S.r_prod.begin(), S.r_prod.end());
    out->layers.push_back(std::move(S.proof));
    lp.lap("layer_finals");
  }
  if (W > 1) {  // every rank's status, so a failure still pending here fails every rank alike
    std::vector<uint8_t> none;
    const int rc = comm_allgather(ctx, sh, fail, nullptr, 0, none);
    if (rc) return rc;
  }
  lp.print();
  *rand_out = rand;
  return 0;
}

int cubic_layer(spg_ctx* ctx, const std::vector<Triple>& tr, size_t nc, const Fq* c_shared, size_t log_len,
                const FqV& coeffs, const Fq& e, Tr& t, LayerProofP* proof, FqV* r, FqV* fin) {
  const size_t nt = tr.size(), len = (size_t)1 << log_len;
  if (!nt || coeffs.size() != nt || nc > nt || (nc && !c_shared))
    return set_err(ctx, SPG_E_ARG, "cubic_layer: one coefficient per triple, a shared vector for the pairs");
  if (3 * nt + 1 > kMboxScalars) return set_err(ctx, SPG_E_ARG, "cubic_layer: too many triples for the mailbox");
  Laps lp;
  lp.title = "SumcheckInstanceProof::prove_cubic_batched";
  const Shard sh;
  LayerEnv E{ctx, t, sh, lp, nc};
  if (int rc = layer_env_init(E, nt, len, 1, 0)) return rc;
  LayerState S;
  S.nt = nt;
  S.ngroups = (nc ? 1 : 0) + (nt - nc);
  S.e = e;
  // the descriptors as for a prover's layer (the launch writes the one-entry eq() of no variables into cbuf[0]), then
  // the caller's shared vector in its place
  int rc = layer_setup(E, tr, coeffs, FqV(), false, len, 0);
  if (rc) return rc;
  if (nc) SPG_HIP(ctx, hipMemcpyAsync(E.cbuf[0], c_shared, len * sizeof(Fq), hipMemcpyDeviceToDevice, ctx->stream));
  rc = run_rounds(E, S, log_len, false, true, fin, 0);
  if (rc) return rc;
  *r = S.r_prod;
  *proof = std::move(S.proof);
  lp.print();
  return 0;
}

}  // namespace spg
