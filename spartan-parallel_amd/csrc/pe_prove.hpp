// spg — the PolyEvalProof provers of SNARK::prove on host polynomials (src/dense_mlpoly.rs:531-780, 1046-1130), in
// polyeval.hip beside the spg_poly_eval_* entries: the grouping walk of pe_plan.hpp, the L.Z bounds on the host pool,
// then one DotProductProofLog per proof slot, serialised into w as bincode(Vec<PolyEvalProof>) / bincode(PolyEvalProof).
#pragma once
#include "proto.hpp"

namespace spg {

// PolyEvalProof::prove_batched_points (:531-622): one polynomial at the points r_list
int prove_batched_points(spg_ctx* ctx, ProverGens& g, const FqV& Z, const std::vector<FqV>& r_list, const FqV& Zr,
                         Tr& t, Tape& tape, Writer& w);
// PolyEvalProof::prove_batched_instances (:689-780): polynomial i at r_list[i], fitted to its variables
int prove_batched_instances(spg_ctx* ctx, ProverGens& g, const std::vector<const FqV*>& polys,
                            const std::vector<FqV>& r_list, const FqV& Zr, Tr& t, Tape& tape, Writer& w);
// The L.Z bounds of PolyEvalProof::prove_uni_batched_instances (:1046-1130), all in one pool burst. The shift proof
// also reads its evaluations from them: sum_k LZ[k] r^k = sum_i Z[i] r^i.
std::vector<FqV> uni_bounds(const std::vector<const FqV*>& polys, const Fq& r);
// PolyEvalProof::prove_uni_batched_instances from the bounds of uni_bounds(polys, r)
int prove_uni_batched(spg_ctx* ctx, ProverGens& g, const std::vector<const FqV*>& polys, const std::vector<FqV>& LZs,
                      const Fq& r, const FqV& Zr, Tr& t, Tape& tape, Writer& w);

}  // namespace spg
