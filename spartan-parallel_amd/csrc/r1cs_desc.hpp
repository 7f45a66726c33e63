// spg — the descriptors of the R1CS table kernels (r1cs_tables.hip) and the one place each is built from sizes. The
// prover's table setup and the seams (r1cs_seams.hip) call these builders, so a descriptor is the same wherever its
// kernel is launched from. Host-only (no HIP types): hostcheck.cpp exports the builders to the CPU suite
// (tests/test_r1cs_tables_host.py).
#pragma once
#include "hostmath.hpp"
#include "pqx.hpp"
#include "r1cs_objs.hpp"

namespace spg {

struct ZDesc {
  uint64_t dom_off, z_off;
  uint32_t lg_q, ni, lg_ni, pad;
};
struct SecDesc {
  const Fq* w;  // the instance's w_mat (spg_r1cs_witness::ptr)
  uint32_t np, ni;
};
struct SpDesc {
  uint64_t dom_off, out_off;
  uint32_t pi, lg_q, nrows, lg_rows, ni, lg_ni;
};
struct MatDesc {
  uint64_t rp[3];
  uint64_t cp;
};
struct AbcDesc {
  uint64_t dom_off, out_off;
  uint32_t pi, ni, lg_ni, pad;
};
// every witness polynomial's L.Z bound of one proof in two launches (instead of two per polynomial): job k's
// partial rows are blocks [b0, b0 + nbx * S) of the first launch, its column sums blocks
// [c0, c0 + ceil(Rs / kSumCols)) of the second
struct BoundDesc {
  const Fq* Z;
  uint32_t offL, Ls, Rs, chunk, S, offP, o, b0, c0;
};
constexpr int kBoundMax = 32;
struct BoundJobs {
  BoundDesc d[kBoundMax];
  int n;
};
constexpr int kSumCols = 16;  // columns per block of the second launch

// a ragged table's shape: instance p owns rows[p] x secs x cols[p] elements, packed in order (total: all of them);
// the four padded maxima are the Pqx fields the folds halve. The caller allocates d.
inline PqxDev pqx_shape(const std::vector<size_t>& rows, size_t secs, const std::vector<size_t>& cols,
                        size_t num_instances, size_t max_num_proofs, size_t num_witness_secs, size_t max_num_inputs) {
  PqxDev T;
  const size_t n = rows.size();
  T.zlen = n;
  T.off.resize(n);
  T.anp = rows;
  T.anw.assign(n, secs);
  T.ani = cols;
  for (size_t p = 0; p < n; p++) {
    T.off[p] = T.total;
    T.total += rows[p] * secs * cols[p];
  }
  T.num_instances = num_instances;
  T.max_num_proofs = max_num_proofs;
  T.num_witness_secs = num_witness_secs;
  T.max_num_inputs = max_num_inputs;
  T.num_proofs = rows;
  T.num_inputs = cols;
  return T;
}
// a table of n instances holding one element each (what remains of a Pqx table when only the instance
// variables are left unbound); its index / index_high behave exactly like the full table's at (p,0,0,0)
inline PqxDev compact_table(Fq* d, size_t n, size_t P) {
  const std::vector<size_t> ones(n, 1);
  PqxDev T = pqx_shape(ones, 1, ones, npow2(n), 1, 1, 1);
  T.d = d;
  T.num_proofs.assign(P, 1);
  T.num_inputs.assign(P, 1);
  return T;
}

// where the matrices of every instance of the handle start (k_spmv, k_abc and k_sparse_eval index it by the global
// matrix index)
inline std::vector<MatDesc> mat_descs(const spg_r1cs_inst& inst) {
  std::vector<MatDesc> md(inst.num_instances);
  for (size_t p = 0; p < inst.num_instances; p++) {
    for (int m = 0; m < 3; m++) md[p].rp[m] = inst.rp_off[3 * p + m];
    md[p].cp = inst.cp_off[p];
  }
  return md;
}

// k_spmv's list over the instances a caller holds: proofs / cons / inputs are their sizes and off their offsets in the
// output tables (a pqx_shape(proofs, 1, cons) table's off), both local; pi is global, p0 + p (p0: the first held
// instance) or 0 when one matrix triple serves every instance. log_ni: the prover's form; the multiply_vec_block seam
// passes false and gets lg_ni = 0 (k_spmv does not read it).
inline std::vector<SpDesc> sp_descs(const std::vector<size_t>& proofs, const std::vector<size_t>& cons,
                                    const std::vector<size_t>& inputs, const std::vector<size_t>& off, size_t p0,
                                    bool single, bool log_ni) {
  std::vector<SpDesc> spd(proofs.size());
  for (size_t p = 0; p < spd.size(); p++) {
    spd[p].dom_off = off[p];
    spd[p].out_off = off[p];
    spd[p].pi = (uint32_t)(single ? 0 : p0 + p);
    spd[p].lg_q = (uint32_t)lg2(proofs[p]);
    spd[p].nrows = (uint32_t)cons[p];
    spd[p].lg_rows = (uint32_t)lg2(cons[p]);
    spd[p].ni = (uint32_t)inputs[p];
    spd[p].lg_ni = log_ni ? (uint32_t)lg2(inputs[p]) : 0;
  }
  return spd;
}

// k_abc's list over the matrices pi0, pi0 + 1, ..: inputs are their widths and off their offsets in the output table (a
// pqx_shape(ones, secs, inputs) table's ani and off)
inline std::vector<AbcDesc> abc_descs(const std::vector<size_t>& inputs, const std::vector<size_t>& off, size_t pi0) {
  std::vector<AbcDesc> ad(inputs.size());
  for (size_t p = 0; p < ad.size(); p++) {
    ad[p].dom_off = off[p];
    ad[p].out_off = off[p];
    ad[p].pi = (uint32_t)(pi0 + p);
    ad[p].ni = (uint32_t)inputs[p];
    ad[p].lg_ni = (uint32_t)lg2(inputs[p]);
    ad[p].pad = 0;
  }
  return ad;
}

}  // namespace spg
