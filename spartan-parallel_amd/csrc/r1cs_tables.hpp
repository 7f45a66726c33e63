// spg — the device tables of R1CSProof::prove and the kernels that make them (r1cs_tables.hip): the Z fill, Az / Bz / Cz
// (k_spmv), ABC (k_abc), the matrix evaluations and the witness polynomials' L.Z bounds. The launch functions below are
// the only host code that launches those kernels; the prover (r1cs.hip), spg_r1cs_sat_check and the seams
// (r1cs_seams.hip) all go through them, with descriptors from r1cs_desc.hpp.
#pragma once
#include <string>
#include <vector>

#include "ctx.hpp"
#include "r1cs_desc.hpp"

namespace spg {

// ---- launches on ctx->stream. scope: open the kernel's profiling scope (a seam that times itself passes false); the
// caller reads hipGetLastError().
// k_z_fill, or k_z_fill_tiled when every instance's row is whole 256-element tiles (scope z_fill)
void launch_z_fill(spg_ctx* ctx, bool tiled, const ZDesc* dz, int n, const SecDesc* dsec, int nws, Fq* Z, size_t total);
// k_spmv<tiled> over n instances, total outputs per table (scope spmv_block; visits: matrix entries read)
void launch_spmv(spg_ctx* ctx, bool scope, bool tiled, const SpDesc* dsd, int n, const MatDesc* dmd,
                 const spg_r1cs_inst& inst, const SecDesc* dsec, int nws, uint32_t Y, Fq* Az, Fq* Bz, Fq* Cz,
                 size_t total, double visits);
// k_abc<split> over n matrices, total outputs per table; split: A, B, C apart into ABC, outB, outC (scope
// eval_table_abc)
void launch_abc(spg_ctx* ctx, bool scope, bool split, const AbcDesc* dad, int n, const MatDesc* dmd,
                const spg_r1cs_inst& inst, const Fq* eq, uint32_t Y, const Fq& rA, const Fq& rB, const Fq& rC, Fq* ABC,
                Fq* outB, Fq* outC, size_t total, double visits);
// k_sparse_eval over nblk blocks of rows per matrix, then k_sum_segments (scope sparse_eval; visits, rows: its model)
void launch_sparse_eval(spg_ctx* ctx, const MatDesc* dmd, const uint32_t* drows, const spg_r1cs_inst& inst,
                        const Fq* eq_rx, const Fq* eq_ry, Fq* part, unsigned nblk, Fq* out, double visits, double rows);
// k_bound_part_multi and k_sum_cols_multi of every batch of at most kBoundMax jobs (scope poly_bound)
struct BoundBatch {
  BoundJobs jobs;
  uint32_t nb, nc;  // blocks of the two launches
};
void launch_bound(spg_ctx* ctx, const std::vector<BoundBatch>& batches, const Fq* L, Fq* part, Fq* out);

// The Z fill. k_spmv gathers from the witness itself, so the fill only has to land before phase 2. On the second
// stream it is queued once phase 1's round SPG_Z_AFTER (default 4) has been evaluated, and runs beside the later,
// smaller rounds: overlapping k_spmv or the first, HBM-bound rounds, the kernels slow each other (rocprof and same-box
// A/Bs: DESIGN §4, round 4). SPG_Z_SIDE=0 fills it in order at setup. Whatever way the prove returns, `stream` is
// ordered after the fill before anything later reuses the Z slot (the destructor joins).
struct ZFill {
  spg_ctx* c = nullptr;
  const ZDesc* dz = nullptr;
  const SecDesc* dsec = nullptr;
  int n = 0, nws = 0;  // local instances, witness sections
  Fq* Z = nullptr;
  size_t total = 0;
  bool tiled = false;  // k_z_fill_tiled: every instance's row is whole 256-element tiles
  bool side = false;
  bool queued = false, armed = false;
  int queue();
  int join();
  ~ZFill() { join(); }
};

// the sizes of one prove
struct Shape {
  size_t np, nq, nx, nw, ny;                       // variables of p, q, x (constraints), w (sections), y (inputs)
  size_t PLn;                                      // this rank's instances [p0, p1)
  std::vector<size_t> l_proofs, l_inputs, l_cons;  // their proofs, inputs and constraints
  size_t num_cons;                                 // the padded maximum of constraints
  bool single;                                     // one matrix triple shared by every instance
};

// The arguments of spg_r1cs_prove / spg_r1cs_sat_check once checked, and this rank's instances [p0, p1)
struct R1csSizes {
  size_t P = 0, max_np = 0, Y = 0, nws = 0;
  std::vector<size_t> num_proofs, num_inputs;
  size_t p0 = 0, p1 = 0;
};

// The table setup of a prove, over the rank's instances: shapes, workspace, descriptors, k_spmv, k_abc and the
// satisfiability check of the tables. No generators, transcript or tape: spg_r1cs_sat_check runs it on its own, the
// Prover holds one.
struct R1csTables {
  spg_ctx* ctx;
  const spg_r1cs_inst& inst;
  const spg_r1cs_witness& wit;
  const R1csSizes sz;
  Shape sh;
  // Z; Az with Bz, Cz of its shape; the matrices' descriptors (k_spmv, k_abc)
  PqxDev Zp, Az;
  Fq *Bz = nullptr, *Cz = nullptr;
  MatDesc* dmd = nullptr;

  R1csTables(spg_ctx* c, const spg_r1cs_inst& in, const spg_r1cs_witness& w, const R1csSizes& s);
  // Z (p, q_rev, w, x_rev) and Az, Bz, Cz (p, q_rev, 0, x_rev) for the local instances: shapes, workspace (want_z: the
  // Z table too) and every setup descriptor in one host-to-device copy; zf: the Z fill, made ready
  int setup_desc(ZFill& zf, bool want_z);
  // Az, Bz, Cz = multiply_vec_block: outputs, CSR row pointers, and per visited entry its column, value and z gather
  int launch_spmv();
  // ABC = r_A A + r_B B + r_C C at eq_rx over the matrices pi0, .. of ABC's shape: one descriptor flush, k_abc
  int launch_abc(const PqxDev& ABC, size_t pi0, const Fq* eq_rx, const Fq& rA, const Fq& rB, const Fq& rC);
  // Az * Bz == Cz over this rank's tables (satcheck.hip), merged over the ranks in one framed allgather outside the
  // prove's exchange plan: every rank gets the same report, with p the caller's instance index
  // (rc: this rank's status so far; non-zero skips its launch and fails every rank)
  int sat_check(int rc, spg_sat_report* out);

 private:
  // descriptors are staged in desc_host (256-byte aligned, at most 1 MB per proof; kept alive until the stream is
  // synchronised) and go up to the device in one copy per flush_desc(); a staged descriptor's device address is valid
  // for kernels launched after that flush
  std::vector<uint8_t> desc_host;
  size_t desc_cur = 0, desc_done = 0;
  uint8_t* desc_dev = nullptr;
  template <class D>
  int stage_desc(const std::vector<D>& v, D** dptr);
  int flush_desc();
  SpDesc* dsd_ = nullptr;
  SecDesc* dsec_ = nullptr;
  bool spmv_tiled_ = false;
  double visits_ = 0;
};

}  // namespace spg
