// spg — what the product-circuit seams (prodc.hip) share with the SPARK prover (spark.hip), both through layers.hip: the tree layout, the
// batched layer prover and its proof objects. The kernels and launch forms live in layers.hip / layer.hpp; prodc.hip
// only arranges caller vectors into the prover's layout and calls these.
#pragma once
#include <vector>

#include "ctx.hpp"
#include "host.hpp"

namespace spg {

// one term k A B C of a batched cubic sumcheck; C == nullptr: the eq vector shared by the product circuits
struct Triple {
  Fq *A, *B, *C;
};

struct LayerProofP {
  std::vector<FqV> polys;  // CompressedUniPoly per round
  FqV left, right;
};
struct BatchedProofP {  // ProductCircuitEvalProofBatched
  std::vector<LayerProofP> layers;
  FqV dotp[3];
  void ser(Writer& w) const {
    w.u64(layers.size());
    for (auto& l : layers) {
      w.u64(l.polys.size());
      for (auto& p : l.polys) w.fqs(p);
      w.fqs(l.left);
      w.fqs(l.right);
    }
    for (int i = 0; i < 3; i++) w.fqs(dotp[i]);
  }
};

// A set of nc product circuits (M leaves each), possibly sharded over the W ranks of a proof (see "sharded
// proof" at SparkProver, spark.hip): rank r holds leaves i = W i' + r as a local tree of m = M / W leaves (levels of
// >= 2 entries at loc + c 2m, the usual back-to-back layout), and every rank holds the global levels of <= W
// entries as a replicated "top" tree (circuit c at top + c 2W, W entries first). W == 1: loc is the whole tree.
struct TreeSh {
  Fq* loc = nullptr;
  size_t m = 0;
  Fq* top = nullptr;
  int W = 1, r = 0;
};

// ProductCircuit::new (product_tree.rs:36-58) of nc circuits whose M leaves are in place (circuit stride 2M, level k
// at 2M - 2(M >> k)): the levels above the leaves, and every circuit's evaluate() into tops (device, nc scalars)
int tree_build(spg_ctx* ctx, Fq* tree, size_t nc, size_t M, Fq* tops);
// DotProductCircuit::evaluate of every triple (n entries per vector) into out (host)
int dotp_evaluate(spg_ctx* ctx, const std::vector<Triple>& dotp, size_t n, Fq* out);
// ProductCircuitEvalProofBatched::prove (product_tree.rs:271-396), see layers.hip
int batched_prove(spg_ctx* ctx, const TreeSh& ts, size_t nc, size_t M, FqV claims, const std::vector<Triple>& dotp,
                  const FqV& dotp_claims, Tr& t, BatchedProofP* out, FqV* rand_out, const Shard& sh);
// One layer's sumcheck (SumcheckInstanceProof::prove_cubic_batched, sumcheck.rs:264-434) over caller vectors of
// 2^log_len entries, all of whose variables are bound: triples 0 .. nc-1 (C == nullptr) share the vector c_shared (2^log_len
// device scalars, copied; required when nc > 0). e: the claim. proof->polys, *r: one entry per round; fin: (A[0], B[0],
// C[0]) of every triple after the last round. The vectors are left partly folded: their bound values are `fin`.
int cubic_layer(spg_ctx* ctx, const std::vector<Triple>& tr, size_t nc, const Fq* c_shared, size_t log_len,
                const FqV& coeffs, const Fq& e, Tr& t, LayerProofP* proof, FqV* r, FqV* fin);

}  // namespace spg
