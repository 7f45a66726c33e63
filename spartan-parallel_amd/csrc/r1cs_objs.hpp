// spg — the device-resident R1CS handles of the C-ABI: the instance's matrices and the witness sections. Made and freed
// by r1cs_objects.hip; read by the table setup (r1cs_tables.hip), the prover (r1cs.hip) and the seams (r1cs_seams.hip).
// Plain host types: no HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "field.hpp"

// R1CSInstance resident in HBM: per matrix instance p, CSR of A_p, B_p, C_p (SpMV) and one merged CSC
// (rows tagged 0/1/2) for the transposed eq-weighted product.
struct spg_r1cs_inst {
  size_t num_instances = 0, max_num_cons = 0, num_vars = 0;
  std::vector<size_t> num_cons;
  std::vector<uint64_t> rp_off, cp_off;  // [3p+m] offsets into rowptr ; [p] offsets into colptr
  std::vector<size_t> nnz;               // [3p+m]
  uint32_t* d_rowptr = nullptr;          // absolute entry indices
  uint32_t* d_col = nullptr;
  spg::Fq* d_val = nullptr;
  uint32_t* d_colptr = nullptr;
  uint32_t* d_crow = nullptr;            // row * 4 + tag
  spg::Fq* d_cval = nullptr;
};

// ProverWitnessSecInfo list resident in HBM: w_mat[p] flattened (q-major), sections concatenated.
static const uint64_t kNotResident = ~0ULL;  // instance held by another rank
struct spg_r1cs_witness {
  size_t nws = 0;
  std::vector<std::vector<size_t>> num_proofs, num_inputs;  // [w][p]
  std::vector<std::vector<uint64_t>> off;                   // [w][p] element offset into d_w
  // [w][p] device address of the instance's w_mat: d_w + off, or a caller's resident device buffer used in place
  // (witness_from_parts); nullptr: held by another rank
  std::vector<std::vector<const spg::Fq*>> ptr;
  spg::Fq* d_w = nullptr;
  size_t total = 0;
};
