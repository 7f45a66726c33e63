// spg — what SparseMatPolynomial::multi_commit and SparseMatPolyEvalProof::prove derive from sizes alone, written once.
// Host-only (no HIP types): spark.hip includes it, and hostcheck.cpp exports it to the CPU suite.
//   SparseMatPolyCommitmentGens::new      src/sparse_mlpoly.rs:289-317      SparkShape: nv_ops, nv_mem, nv_der
//   multi_sparse_to_dense_rep, Derefs     :368-425, :51-67                  SparkShape: the comb lengths, der_len
//   ProductCircuit::new, top levels       src/product_tree.rs:36-58         tree_tops_host (sharded proofs)
#pragma once
#include <algorithm>

#include "hostmath.hpp"

namespace spg {

// N, the ops of each batched matrix: its entries padded to a power of two, at least 2; cells of the memory both sides
// address (matrices of 2^nvx x 2^nvy)
inline size_t spark_num_ops(size_t max_nnz) { return std::max<size_t>(2, npow2(max_nnz)); }
inline size_t spark_num_cells(size_t nvx, size_t nvy) { return (size_t)1 << std::max<size_t>(std::max(nvx, nvy), 1); }

// B batched matrices of N (padded) entries each over `cells` memory cells, against generators made for matrices of
// 2^gens_nvx x 2^gens_nvy, gens_nnz entries and gens_batch matrices
struct SparkShape {
  size_t nv_ops, nv_mem, nv_der;  // variables of the three PolyCommitmentGens (views of one derived stream)
  size_t ops_len, mem_len;        // comb_ops: [row addr | row read_ts | col addr | col read_ts | val], zero-padded
  size_t der_len;                 // comb_mem: [row audit | col audit]; derefs: [row | col], zero-padded
  SparkShape(size_t B, size_t N, size_t cells, size_t gens_nvx, size_t gens_nvy, size_t gens_nnz, size_t gens_batch)
      : nv_ops(lg2(npow2(gens_nnz)) + lg2(npow2(gens_batch * 5))),
        nv_mem(std::max(gens_nvx, gens_nvy) + 1),
        nv_der(lg2(npow2(gens_nnz)) + lg2(npow2(gens_batch * 2))),
        ops_len(npow2(5 * B * N)),
        mem_len(2 * cells),
        der_len(npow2(2 * B * N)) {}
  // generators of the derived stream (its blinding generator is one more): the widest Hyrax row of the three
  size_t gens_n() const {
    size_t n = 0;
    for (size_t nv : {nv_ops, nv_mem, nv_der}) n = std::max(n, (size_t)1 << (nv - nv / 2));
    return n;
  }
  // mem_nv: the variables the memory side needs
  bool fits(size_t mem_nv) const { return lg2(ops_len) <= nv_ops && lg2(der_len) <= nv_der && mem_nv <= nv_mem; }
  // Hyrax row commitments of comb_ops and comb_mem (DensePolynomial::commit: 2^(nv / 2) rows)
  size_t ops_rows() const { return (size_t)1 << (lg2(ops_len) / 2); }
  size_t mem_rows() const { return (size_t)1 << (lg2(mem_len) / 2); }
};

// The refusals check the sizes' ranges before they form a SparkShape (whose lengths would overflow outside them).
// multi_commit's own sizes, matrices of 2^nvx x 2^nvy (cells = 2^max(nvx, nvy, 1): a 1 x 1 matrix still needs only one
// memory variable of the generators): null, or why the batch cannot be committed
inline const char* spark_commit_refusal(size_t B, size_t N, size_t cells, size_t nvx, size_t nvy, size_t gens_nvx,
                                        size_t gens_nvy, size_t gens_nnz, size_t gens_batch) {
  if (2 * B * N >= 0xffffffffULL || cells > 0xffffffffULL) return "SPARK batch too large";
  if (!SparkShape(B, N, cells, gens_nvx, gens_nvy, gens_nnz, gens_batch).fits(std::max(nvx, nvy) + 1))
    return "SPARK generators (gens_nnz, gens_batch) too small for the batch";
  return nullptr;
}
// a commitment read back (spark_from_comm): the shapes multi_commit gives are N a power of two >= 2, cells a power of
// two, and one Hyrax row commitment per row of comb_ops and comb_mem. Null, or why it is refused
inline const char* spark_comm_refusal(size_t B, size_t N, size_t cells, size_t ops_rows, size_t mem_rows,
                                      size_t gens_nvx, size_t gens_nvy, size_t gens_nnz, size_t gens_batch) {
  if (!B || N < 2 || !is_pow2(N) || !cells || !is_pow2(cells) || B > (1u << 20) || N > (1ull << 32) ||
      cells > (1ull << 32))
    return "SPARK commitment sizes do not fit the generators";
  const SparkShape sp(B, N, cells, gens_nvx, gens_nvy, gens_nnz, gens_batch);
  if (!sp.fits(lg2(sp.mem_len))) return "SPARK commitment sizes do not fit the generators";
  if (ops_rows != sp.ops_rows() || mem_rows != sp.mem_rows()) return "SPARK commitment row counts do not match its sizes";
  return nullptr;
}

// The top lg W levels of a product circuit whose W-entry level is sharded one entry per rank (the product of rank q's
// local tree is entry q): v[0 .. W) = that level, then the levels above it back to back (ProductCircuit::compute_layer:
// entry i times entry i + len / 2) in the trees' layout, 2W entries in all. Returns the circuit's evaluate().
inline Fq tree_tops_host(Fq* v, size_t W) {
  size_t o = 0;
  for (size_t len = W; len > 2; len /= 2) {
    for (size_t i = 0; i < len / 2; i++) v[o + len + i] = fq_mul(v[o + i], v[o + i + len / 2]);
    o += len;
  }
  return fq_mul(v[o], v[o + 1]);
}

}  // namespace spg
