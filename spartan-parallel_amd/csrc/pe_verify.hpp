// spg — PolyEvalProof::verify* (src/dense_mlpoly.rs:492-528, 624-685, 782-857, 962-1044, 1132-1203) on proof bytes, one
// call at a time: the Verifier members of verify.hip (pe_verify, pe_plain_batched_points, pe_plain_batched_instances,
// pe_batched_disjoint, pe_uni_batched, with their row MSMs and DotProductProofLog checks) behind one function each, for
// the spg_poly_eval_verify* and spg_pe_verify_* entries of polyeval.hip.
// Each returns 0 or SPG_E_VERIFY with the failed check in spg_last_error.
#pragma once
#include "proto.hpp"

namespace spg {

// PolyEvalProof::verify (C_Zr given) or verify_plain (Zr given) of bincode(PolyEvalProof)
int pe_verify_one(spg_ctx* ctx, ProverGens& g, Tr& t, const FqV& r, const Pt* C_Zr, const Fq* Zr,
                  const std::vector<Pt>& comm, const uint8_t* proof, size_t len);
// verify_plain_batched_points / verify_plain_batched_instances of bincode(Vec<PolyEvalProof>)
int pe_verify_points(spg_ctx* ctx, ProverGens& g, Tr& t, const std::vector<FqV>& r_list, const FqV& Zr_list,
                     const std::vector<Pt>& comm, const uint8_t* proof, size_t len);
int pe_verify_instances(spg_ctx* ctx, ProverGens& g, Tr& t, const std::vector<FqV>& r_list, const FqV& Zr_list,
                        const std::vector<std::vector<Pt>>& comms, const std::vector<size_t>& nv_list,
                        const uint8_t* proof, size_t len);
// verify_batched_instances_disjoint_rounds (:962-1044) of bincode(Vec<PolyEvalProof>) and verify_uni_batched_instances
// (:1132-1203) of bincode(PolyEvalProof): V::pe_batched_disjoint and V::pe_uni_batched. C_Zr: the commitments to the
// evaluations, compressed (one that does not decompress fails the verification)
int pe_verify_disjoint(spg_ctx* ctx, ProverGens& g, Tr& t, const std::vector<size_t>& np_list,
                       const std::vector<size_t>& ni_list, const FqV& rq, const FqV& ry, const std::vector<Pt>& C_Zr,
                       const std::vector<std::vector<Pt>>& comms, const uint8_t* proof, size_t len);
int pe_verify_uni(spg_ctx* ctx, ProverGens& g, Tr& t, const Fq& r, const std::vector<Pt>& C_Zr,
                  const std::vector<std::vector<Pt>>& comms, const std::vector<size_t>& sizes, const uint8_t* proof,
                  size_t len);

}  // namespace spg
