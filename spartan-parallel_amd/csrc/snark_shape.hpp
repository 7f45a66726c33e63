// spg — the public shape of SNARK::prove and SNARK::verify (src/lib.rs:971-2746, 2750-3881): everything both sides
// derive from the sizes alone, written once. Host-only (no HIP types): snark.hip and verify.hip include it, and
// hostcheck.cpp exports it to the CPU suite.
//   parameter appends                     lib.rs:1086-1153 / 2855-2920      append_snark_params, append_comm_map
//   block sort, padding, pairwise sort    lib.rs:1155-1296 / 2922-3009      SnarkShape
//   ProverWitnessSecInfo::merge           lib.rs:546-604 / 606-698          merge_order
//   perm_w0 = (tau, r, r^2, ...)          lib.rs:1299-1320                  perm_w0
//   ShiftProofs polynomial list           lib.rs:2611-2668 / 3772-3853      shift_pairs
//   IOProofs evaluation points            lib.rs:194-272 / 283-359          io_points
#pragma once
#include <algorithm>
#include <vector>

#include "hostmath.hpp"

namespace spg {

const size_t INIT_PHY_MEM_WIDTH = 4, INIT_VIR_MEM_WIDTH = 4, PHY_MEM_WIDTH = 4, VIR_MEM_WIDTH = 8, W3_WIDTH = 8;

// indices sorted by decreasing size, ties in index order, the first `keep` of them
inline std::vector<size_t> sorted_desc(const std::vector<size_t>& sizes, size_t keep) {
  std::vector<size_t> o(sizes.size());
  for (size_t i = 0; i < o.size(); i++) o[i] = i;
  std::stable_sort(o.begin(), o.end(), [&](size_t x, size_t y) { return sizes[x] > sizes[y]; });
  o.resize(keep);
  return o;
}

struct SnarkShape {
  size_t niu = 0;
  size_t P = 0;               // blocks with at least one execution
  std::vector<size_t> order;  // sorted instance i is block order[i] (num_proofs descending, ties in block order)
  std::vector<size_t> bnp, bnp_pad, bnv, bphy, bvir;  // per sorted instance
  size_t bmax = 0, consis = 0;
  size_t t_iphy = 0, t_ivir = 0, t_phy = 0, t_vir = 0;  // padded totals (0 stays 0)
  std::vector<size_t> pw_order;  // pairwise instances (0 consis, 1 phy, 2 vir) by decreasing size, empty ones dropped
  size_t pairwise_size = 0, perm_size = 0, pw_nv = 0;
  size_t w2_size(size_t p) const { return npow2(2 * niu + 2 * bphy[p] + 4 * bvir[p]); }

  SnarkShape(const spg_snark_inputs& a, const size_t* nproofs, const size_t* nvars, const size_t* phy_ops,
             const size_t* vir_ops)
      : niu(a.num_inputs_unpadded) {
    const size_t Bb = a.block_num_instances_bound;
    for (size_t b = 0; b < Bb; b++) P += nproofs[b] > 0;
    order = sorted_desc(std::vector<size_t>(nproofs, nproofs + Bb), P);
    for (size_t b : order) {
      bnp.push_back(nproofs[b]);
      bnp_pad.push_back(npow2(nproofs[b]));
      bnv.push_back(nvars[b]);
      bphy.push_back(phy_ops[b]);
      bvir.push_back(vir_ops[b]);
    }
    bmax = npow2(a.block_max_num_proofs);
    consis = npow2(a.consis_num_proofs);
    auto padded = [](size_t n) { return n ? npow2(n) : (size_t)0; };
    t_iphy = padded(a.total_num_init_phy_mem_accesses);
    t_ivir = padded(a.total_num_init_vir_mem_accesses);
    t_phy = padded(a.total_num_phy_mem_accesses);
    t_vir = padded(a.total_num_vir_mem_accesses);
    pw_order = sorted_desc({consis, t_phy, t_vir}, 1 + (t_phy > 0) + (t_vir > 0));
    pairwise_size = std::max({consis, t_phy, t_vir});
    perm_size = std::max({consis, t_iphy, t_ivir, t_phy, t_vir});
    pw_nv = std::max<size_t>(8, a.mem_addr_ts_bits_size);
  }
};

// Block b's witness rows hold nvars[b] entries, and every section of its R1CS instance is that wide: the row's io and
// memory-operation part (2 niu + 2 phy + 4 vir entries, which the w2 recurrences read on the host) and every column
// its matrices name (col % stride, stride = num_vars: the section width of the matrices) must lie inside them. The
// reference indexes its vectors there and panics; the device kernels would skip such entries (k_spmv, k_abc) and the
// host would read past a row's end. block_cols_needed reads the matrices once (entries[3 b + m] / nnz[3 b + m]:
// matrix m of block b, spg_r1cs_instance's layout): need[b] = 1 + the largest in-section column block b names, 0
// without entries. block_width_violation returns the first executed block that breaks either rule, or -1.
inline std::vector<size_t> block_cols_needed(size_t Bb, size_t stride, const spg_sparse_entry* const* entries,
                                             const size_t* nnz) {
  std::vector<size_t> need(Bb, 0);
  for (size_t k = 0; k < 3 * Bb; k++)
    for (size_t e = 0; e < nnz[k]; e++) need[k / 3] = std::max<size_t>(need[k / 3], entries[k][e].col % stride + 1);
  return need;
}
inline long block_width_violation(size_t Bb, const size_t* nproofs, const size_t* nvars, const size_t* phy_ops,
                                  const size_t* vir_ops, size_t niu, size_t stride, const size_t* need) {
  for (size_t b = 0; b < Bb; b++)
    if (nproofs[b] && (nvars[b] < 2 * niu + 2 * phy_ops[b] + 4 * vir_ops[b] || nvars[b] > stride || need[b] > nvars[b]))
      return (long)b;
  return -1;
}

// the parameters of the program, in the reference's order (block_max_num_proofs is appended twice there)
template <class T>
void append_snark_params(T& t, const spg_snark_inputs& a, const size_t* nproofs, const size_t* nvars,
                         const size_t* phy_ops, const size_t* vir_ops) {
  const size_t Bb = a.block_num_instances_bound;
  auto app = [&](const char* l, size_t v) { t.scalar(l, fq_from_u64(v)); };
  app("func_input_width", a.func_input_width);
  app("input_offset", a.input_offset);
  app("output_offset", a.output_offset);
  app("output_exec_num", a.output_exec_num);
  app("num_ios", a.num_ios);
  for (size_t b = 0; b < Bb; b++) app("block_num_vars", nvars[b]);
  app("mem_addr_ts_bits_size", a.mem_addr_ts_bits_size);
  app("num_inputs_unpadded", a.num_inputs_unpadded);
  app("block_num_instances_bound", Bb);
  app("block_max_num_proofs", a.block_max_num_proofs);
  for (size_t b = 0; b < Bb; b++) app("block_num_phy_ops", phy_ops[b]);
  for (size_t b = 0; b < Bb; b++) app("block_num_vir_ops", vir_ops[b]);
  app("total_num_init_phy_mem_accesses", a.total_num_init_phy_mem_accesses);
  app("total_num_init_vir_mem_accesses", a.total_num_init_vir_mem_accesses);
  app("total_num_phy_mem_accesses", a.total_num_phy_mem_accesses);
  app("total_num_vir_mem_accesses", a.total_num_vir_mem_accesses);
  app("block_max_num_proofs", a.block_max_num_proofs);
  for (size_t b = 0; b < Bb; b++) app("block_num_proofs", nproofs[b]);
}
template <class T>
void append_comm_map(T& t, const std::vector<std::vector<size_t>>& block_comm_map) {
  for (auto& lm : block_comm_map)
    for (size_t l : lm) t.scalar("block_comm_map", fq_from_u64(l));
}
// the public input / output after the instance commitments
template <class T>
void append_snark_io(T& t, const spg_snark_inputs& a, const FqV& input, const Fq& output) {
  t.scalar("input_block_num", fq_from_u64(a.input_block_num));
  t.scalar("output_block_num", fq_from_u64(a.output_block_num));
  t.scalars("input_list", input);
  t.scalar("output_list", output);
}

inline FqV perm_w0(const Fq& tau, const Fq& r, size_t niu, size_t num_ios) {
  FqV w = {tau};
  Fq rt = r;
  for (size_t i = 1; i < 2 * niu; i++) {
    w.push_back(rt);
    rt = fq_mul(rt, r);
  }
  w.resize(num_ios, fq_zero());
  return w;
}

// ProverWitnessSecInfo::merge / VerifierWitnessSecInfo::merge: the instances of several components interleaved by
// decreasing num_proofs, ties to the earlier component. sizes[c] = num_proofs of component c (each list descending);
// inst_map[k] = the component the k-th merged instance comes from (its next unread instance). False when an
// instance has no proofs: no order exists, and nothing past a list's end is read.
inline bool merge_order(const std::vector<const std::vector<size_t>*>& sizes, std::vector<size_t>* inst_map) {
  std::vector<size_t> ptr(sizes.size(), 0);
  size_t total = 0;
  for (auto c : sizes) total += c->size();
  inst_map->clear();
  while (inst_map->size() < total) {
    size_t best = 0, nc = 0;
    for (size_t i = 0; i < sizes.size(); i++)
      if (ptr[i] < sizes[i]->size() && (*sizes[i])[ptr[i]] > best) {
        best = (*sizes[i])[ptr[i]];
        nc = i;
      }
    if (best == 0) return false;
    inst_map->push_back(nc);
    ptr[nc]++;
  }
  return true;
}
// the polynomial pairs (original, shifted) of the shift proof in order, each with the number of leading entries
// opened in its header and its length in scalars before padding
struct ShiftPair {
  enum Kind { kPermExecW3, kBlockW3, kMemW3, kAddrPhy, kAddrVir } kind;
  size_t idx;  // kBlockW3: sorted instance; kMemW3: 0 init phy, 1 init vir, 2 phy, 3 vir
  size_t header, size;
};
inline std::vector<ShiftPair> shift_pairs(const SnarkShape& s) {
  std::vector<ShiftPair> v = {{ShiftPair::kPermExecW3, 0, 6, W3_WIDTH * s.consis}};
  for (size_t p = 0; p < s.P; p++) v.push_back({ShiftPair::kBlockW3, p, 8, W3_WIDTH * s.bnp_pad[p]});
  if (s.t_iphy) v.push_back({ShiftPair::kMemW3, 0, 6, W3_WIDTH * s.t_iphy});
  if (s.t_ivir) v.push_back({ShiftPair::kMemW3, 1, 6, W3_WIDTH * s.t_ivir});
  if (s.t_phy) {
    v.push_back({ShiftPair::kAddrPhy, 0, 4, PHY_MEM_WIDTH * s.t_phy});
    v.push_back({ShiftPair::kMemW3, 2, 6, W3_WIDTH * s.t_phy});
  }
  if (s.t_vir) {
    v.push_back({ShiftPair::kAddrVir, 0, 6, VIR_MEM_WIDTH * s.t_vir});
    v.push_back({ShiftPair::kMemW3, 3, 6, W3_WIDTH * s.t_vir});
  }
  return v;
}

// the points of the exec-inputs polynomial the IO proof opens (as indices into its consis x num_ios entries) and the
// values claimed there: the two valid bits, the input and output block numbers, the output, every live input
struct IoPoints {
  std::vector<size_t> idx;
  FqV Zr;
  size_t r_len;
  std::vector<FqV> r_list() const {  // every index as its r_len bits, high bit first
    std::vector<FqV> l;
    for (size_t x : idx) {
      FqV bits(r_len);
      for (size_t i = 0; i < r_len; i++) bits[i] = ((x >> (r_len - 1 - i)) & 1) ? fq_one() : fq_zero();
      l.push_back(bits);
    }
    return l;
  }
};
inline IoPoints io_points(const spg_snark_inputs& a, size_t consis, const uint8_t* live, size_t live_n, const FqV& input,
                          const Fq& output) {
  const size_t niu = a.num_inputs_unpadded;
  std::vector<size_t> in_idx;
  for (size_t i = 0; i + 2 < live_n; i++) in_idx.push_back(2 + a.input_offset + i);
  if (live_n > 1 && live[1]) in_idx.insert(in_idx.begin(), 5);
  if (live_n > 0 && live[0]) in_idx.insert(in_idx.begin(), 6);
  FqV live_in;
  for (size_t i = 0; i < live_n && i < input.size(); i++)
    if (live[i]) live_in.push_back(input[i]);
  in_idx.resize(live_in.size());
  const size_t oe = a.output_exec_num * a.num_ios;
  IoPoints p;
  p.r_len = lg2(consis * a.num_ios);
  p.idx = {0, oe, 2, oe + 2 + (niu - 1), oe + 2 + (niu - 1) + a.output_offset - 1};
  p.idx.insert(p.idx.end(), in_idx.begin(), in_idx.end());
  p.Zr = {fq_one(), fq_one(), fq_from_u64(a.input_block_num), fq_from_u64(a.output_block_num), output};
  p.Zr.insert(p.Zr.end(), live_in.begin(), live_in.end());
  return p;
}

}  // namespace spg
