// spg — every environment variable the library reads, declared once. This header is the only place in csrc/ that
// calls getenv (tests/test_knobs.py scans for it). A new switch is one row of SPG_KNOBS below; a new launch form adds
// its row plus an entry in the form list of the matching GPU test.
//
// A row is X(id, "NAME", kind, default, lo, hi, live, "description") and gives two accessors, knob::id() and
// knob::id_is_set(). Kinds, with their parse rule as a pure function of (text or nullptr, default, lo, hi):
//   ON       bool    on unless set to 0                    (!text || atoi(text) != 0)
//   OFF      bool    off unless set to non-zero            (text && atoi(text) != 0)
//   PRESENT  bool    set at all, whatever the value        (text != nullptr)
//   INT      int     atoi(text), clamped to [lo, hi] when set; the default is returned as it stands
//   LONG     long    atol(text), likewise
//   GB       size_t  bytes: (size_t)atof(text) << 30 -- whole gigabytes, the fraction is dropped
//   STR      const char*  the text itself
//   COSTS    StepCosts    sscanf "%d,%d,%d" over the default: fields the text leaves out keep their default
// live = 0: the value is fixed at the knob's own first use (a function-local static, so bench.py and the tests can set
// a variable in-process before the first call that reads it); nothing reads the table as a whole. live = 1: re-read on
// every call (scripts/perf_small_msm.py sweeps SPG_SMSM_C in one process; the pool, pin and debug variables were
// always read where they are used).
//
// Oddities kept as they were:
//   * SPG_TRACE is a level, but the level-1 laps (hostpoly.hpp Laps, spg_snark_prove's call time) test whether it is
//     set: SPG_TRACE=0 prints them. proto.hip's cumulative laps ask for the level while the library loads, so the
//     level (every >= 2 and >= 3 test) is fixed at library load, not at first use; whether it is set, at first use.
//   * SPG_VEC_MIN=0 switches the 8-lane host sums off everywhere (host.hpp, proto.hip, comb.hip).
//   * negative LONG values reach their sites as huge size_t counts (the sites cast, as they always did); the limits
//     derived at the sites are taken there: SPG_PAIR_MAX by SPG_PAIR_BS (layers.hip), SPG_TRIPLE_MAX at 384,
//     SPG_P1_PAIR_MAX / SPG_P2_PAIR_MAX at kP1PairMax (r1cs.hip), SPG_VMSM_C to 4..14 when non-zero (vmsm.hpp),
//     SPG_H2D_CHUNK_KB at the upload chunk, SPG_SMSM_C outside 4..9 ignored (msm.hip).
//   * SPG_COMB_C, SPG_POOL_THREADS, SPG_TRACE: unset (kUnset) differs from every value, 0 included: the sites ask
//     _is_set() (the window by size, the workers by the CPUs, no laps at all).
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

namespace spg {
namespace knob {

constexpr long kNoLo = LONG_MIN, kNoHi = LONG_MAX;
struct StepCosts {
  int c[3];
};
using CStr = const char*;
// the default of a number whose site asks _is_set(): unset is not the same as any value (it reads as 0 where read)
struct Unset {
  constexpr operator int() const { return 0; }
};
constexpr Unset kUnset{};

// clang-format off
#define SPG_KNOBS(X) \
  /* ---- deployment */ \
  X(pin, "SPG_PIN", ON, true, kNoLo, kNoHi, 1, "spg_init pins the host pool's workers to one L3 domain local to the GPU") \
  X(pool_threads, "SPG_POOL_THREADS", INT, kUnset, kNoLo, kNoHi, 1, "host pool workers besides the caller; unset: min(7, usable CPUs - 1)") \
  X(pool_spin_us, "SPG_POOL_SPIN_US", INT, 20000, kNoLo, kNoHi, 1, "how long an idle pool worker spins before it parks") \
  X(local_world_size, "LOCAL_WORLD_SIZE", INT, 0, kNoLo, kNoHi, 1, "(external, torchrun) processes of this node: divides the usable CPUs, orders the pin domains") \
  X(local_rank, "LOCAL_RANK", INT, 0, kNoLo, kNoHi, 1, "(external, torchrun) this process' slot among the pin domains") \
  X(trace, "SPG_TRACE", INT, kUnset, kNoLo, kNoHi, 0, "set: host-time breakdowns on stderr; >= 2: commitment, Bullet and pool counters; >= 3: a line per proof") \
  X(trace_events, "SPG_TRACE_EVENTS", PRESENT, false, kNoLo, kNoHi, 0, "every lap's end on stderr with its CLOCK_MONOTONIC time (scripts/kernel_gaps.py)") \
  X(copy_trace, "SPG_COPY_TRACE", OFF, false, kNoLo, kNoHi, 0, "count hipMemcpyAsync calls per source line, printed after each SNARK::prove") \
  X(comb, "SPG_COMB", ON, true, kNoLo, kNoHi, 0, "row batches use the generator set's comb table; 0: the bucket pipeline") \
  X(comb_gb, "SPG_COMB_GB", GB, 144.0, kNoLo, kNoHi, 0, "process-wide cap on comb-table memory; unset: also keep headroom free beside a table") \
  X(comb_pad, "SPG_COMB_PAD", ON, true, kNoLo, kNoHi, 0, "comb entries padded to one 128-byte line where the padded table fits") \
  X(comb_pad_gb, "SPG_COMB_PAD_GB", GB, 64.0, kNoLo, kNoHi, 0, "largest padded comb table; larger ones stay packed") \
  X(comb_c, "SPG_COMB_C", INT, kUnset, 10, 13, 0, "window width of every comb table up to 16384 generators; unset: 13 up to 1024 generators, 12 above") \
  X(comb_c_wide, "SPG_COMB_C_WIDE", INT, 9, 9, 10, 0, "window width of comb tables over more than 16384 generators") \
  X(comb_c_big, "SPG_COMB_C_BIG", INT, 13, 12, 13, 0, "window width of comb tables of exactly 16384 generators (unless SPG_COMB_C is set)") \
  X(halved_enc, "SPG_HALVED_ENC", ON, true, kNoLo, kNoHi, 0, "comb row batches come back as halves and are encoded on the host pool as doubles; 0: device encodings") \
  X(big_comb, "SPG_BIG_COMB", ON, true, kNoLo, kNoHi, 0, "single MSMs of >= 2^14 points from the comb table; 0: msm_big's buckets") \
  X(big_comb_g, "SPG_BIG_COMB_G", LONG, 2, kNoLo, kNoHi, 0, "window groups per scalar of msm_single_comb: 1, 2, else 4") \
  X(bullet_host_max, "SPG_BULLET_HOST_MAX", LONG, 32, kNoLo, kNoHi, 0, "DotProductProofLog sizes proved on the host pool; larger ones one device launch per round") \
  X(vmsm_host_max, "SPG_VMSM_HOST_MAX", LONG, 64, kNoLo, kNoHi, 0, "variable-base MSMs of fewer points run on the host pool; spg_set_vmsm_host_max overrides per context") \
  X(vmsm_c, "SPG_VMSM_C", INT, 0, kNoLo, kNoHi, 0, "forces the variable-base MSM's window width (taken into 4..14); 0: by size") \
  X(verify_vmsm, "SPG_VERIFY_VMSM", OFF, false, kNoLo, kNoHi, 0, "the verifier's row-commitment MSMs through spg_msm_var_batch instead of the host Pippenger") \
  X(host_enc_max, "SPG_HOST_ENC_MAX", LONG, 384, kNoLo, kNoHi, 0, "row-commit batches of at most this many points are encoded on the host pool") \
  X(host_commit_max, "SPG_HOST_COMMIT_MAX", LONG, 0, kNoLo, kNoHi, 0, "row batches of at most this many scalars are committed on the host pool (0: off)") \
  X(host_prefetch, "SPG_HOST_PREFETCH", LONG, 3, kNoLo, kNoHi, 0, "host fixed-base bursts prefetch the table entry this many additions ahead (0: off)") \
  X(host_ifma, "SPG_HOST_IFMA", ON, true, kNoLo, kNoHi, 0, "8-lane AVX-512 IFMA host sums where the CPU has them; 0: scalar additions") \
  X(rccl_timeout_s, "SPG_RCCL_TIMEOUT_S", LONG, 600, 1, kNoHi, 0, "bounded wait of one RCCL exchange, seconds; past it the communicator is aborted") \
  X(h2d, "SPG_H2D", OFF, false, kNoLo, kNoHi, 0, "witness uploads through upload workers instead of one pageable hipMemcpyAsync") \
  X(h2d_threads, "SPG_H2D_THREADS", INT, 8, kNoLo, kNoHi, 0, "upload workers (at most the usable CPUs)") \
  X(h2d_chunk_kb, "SPG_H2D_CHUNK_KB", LONG, 0, kNoLo, kNoHi, 0, "upload chunk in KB (0: about two chunks per worker, 256 KB .. 4 MB)") \
  X(h2d_trace, "SPG_H2D_TRACE", PRESENT, false, kNoLo, kNoHi, 0, "one stderr line per streamed upload") \
  X(mapped_buckets, "SPG_MAPPED_BUCKETS", ON, true, kNoLo, kNoHi, 0, "kernels leave host-finished parts in mapped host memory; 0: device buffer and download") \
  /* ---- test and debug hooks */ \
  X(failpoint, "SPG_FAILPOINT", STR, nullptr, kNoLo, kNoHi, 0, "name of the site that fails on purpose (tests/test_gpu_dist.py)") \
  X(failpoint_rank, "SPG_FAILPOINT_RANK", INT, 0, kNoLo, kNoHi, 0, "the rank SPG_FAILPOINT fires on") \
  X(debug_tr, "SPG_DEBUG_TR", PRESENT, false, kNoLo, kNoHi, 1, "prover and verifier print their first challenges") \
  X(debug_snark, "SPG_DEBUG_SNARK", PRESENT, false, kNoLo, kNoHi, 1, "SNARK::prove prints transcript checkpoints (compared with the oracle's)") \
  X(big_probe, "SPG_BIG_PROBE", PRESENT, false, kNoLo, kNoHi, 0, "msm_big: per-workgroup phase timestamps on stderr") \
  /* ---- A/B and parity forms: MSM pipelines */ \
  X(msm_big, "SPG_MSM_BIG", ON, true, kNoLo, kNoHi, 0, "one large MSM through msm_big.hip; 0: the batch pipeline") \
  X(big_c, "SPG_BIG_C", INT, 11, 8, 14, 0, "msm_big's window width") \
  X(big_items, "SPG_BIG_ITEMS", ON, true, kNoLo, kNoHi, 0, "msm_big accumulates a lane per entry run; 0: a quad per chunk") \
  X(big_spt, "SPG_BIG_SPT", INT, 1, 1, kNoHi, 0, "msm_big digit blocks: scalars per thread") \
  X(smsm_quad, "SPG_SMSM_QUAD", ON, true, kNoLo, kNoHi, 0, "small-MSM kernels in the quad form (4 lanes per point)") \
  X(smsm_c, "SPG_SMSM_C", INT, 0, kNoLo, kNoHi, 1, "window width of the latency-path MSM when in 4..9; else by size") \
  X(item_k, "SPG_ITEM_K", INT, 16, 1, kNoHi, 0, "batch MSM: entries summed per work item") \
  X(seg_m, "SPG_SEG_M", INT, 8, 1, kNoHi, 0, "batch MSM: buckets per running-sum segment") \
  X(rows_cmax, "SPG_ROWS_CMAX", INT, 16, kNoLo, kNoHi, 0, "batch MSM: widest window whose digits one workgroup per MSM sorts in LDS") \
  X(seg_quad_max, "SPG_SEG_QUAD_MAX", LONG, 16384, kNoLo, kNoHi, 0, "batch MSM: segment sums in the quad form up to this many segments") \
  X(final_sl, "SPG_FINAL_SL", INT, 0, kNoLo, kNoHi, 0, "batch MSM: slots of the final scan (32, 64, 128); 0: by the number of MSMs") \
  X(vmsm_ch, "SPG_VMSM_CH", INT, 1024, 1, kNoHi, 0, "variable-base MSM: entries per chunk (default 4 per lane)") \
  X(comb_wgs, "SPG_COMB_WGS", LONG, 2048, kNoLo, kNoHi, 0, "msm_comb: workgroups aimed at") \
  X(comb_gmax, "SPG_COMB_GMAX", LONG, 4, kNoLo, kNoHi, 0, "msm_comb: most window groups per scalar") \
  X(comb_gmin, "SPG_COMB_GMIN", LONG, 1, kNoLo, kNoHi, 0, "msm_comb: fewest window groups per scalar (2 or 4; else 1)") \
  X(finals_k, "SPG_FINALS_K", INT, 8, 1, kNoHi, 0, "bucket finals: most chunks per bucket set") \
  X(slice_min, "SPG_SLICE_MIN", LONG, 64, kNoLo, kNoHi, 0, "host fixed-base bursts: fewest units per pool slice") \
  X(enc_split, "SPG_ENC_SPLIT", ON, true, kNoLo, kNoHi, 0, "several small host commitments in one burst get a pool slice each") \
  X(vec_min, "SPG_VEC_MIN", LONG, 16, kNoLo, kNoHi, 0, "shortest run of a host job that takes the 8-lane sums; 0: never, anywhere") \
  X(axpy_pool, "SPG_AXPY_POOL", ON, true, kNoLo, kNoHi, 0, "the batched openings' random combinations on the host pool; 0: the calling thread") \
  /* ---- A/B and parity forms: Bullet / DotProductProofLog */ \
  X(bullet_comb, "SPG_BULLET_COMB", ON, true, kNoLo, kNoHi, 0, "device Bullet rounds and the Cx MSM from the comb table; 0: the bucket kernel") \
  X(bcomb_g, "SPG_BCOMB_G", INT, 0, kNoLo, kNoHi, 0, "Bullet comb: window groups per scalar (4, 8, 11); else by size") \
  X(bcomb_bs, "SPG_BCOMB_BS", INT, 0, kNoLo, kNoHi, 0, "Bullet comb: threads per workgroup (64, 128, 256); else by size") \
  X(bcomb_r, "SPG_BCOMB_R", INT, 0, kNoLo, kNoHi, 0, "Bullet comb: points a workgroup leaves for the host (a power of two); else by size") \
  X(bcomb_notree, "SPG_BCOMB_NOTREE", INT, 0, kNoLo, kNoHi, 0, "Bullet rounds of at most this many points per MSM skip the LDS tree") \
  X(bullet_dev, "SPG_BULLET_DEV", ON, true, kNoLo, kNoHi, 0, "DotProductProofLogs above the host size keep their Bullet state on the device") \
  X(bullet_ahead, "SPG_BULLET_AHEAD", ON, true, kNoLo, kNoHi, 0, "round 0 of the device Bullet rounds is launched ahead, with the Cx MSM") \
  X(bullet_overlap, "SPG_BULLET_OVERLAP", ON, true, kNoLo, kNoHi, 0, "host Bullet folds of n >= 256 run on the pool beside the challenge's inversion") \
  X(dotlog_early, "SPG_DOTLOG_EARLY", ON, true, kNoLo, kNoHi, 0, "DotProductProofLog's Cy beside Cx and beta in round 0's burst; 0: bursts of their own") \
  X(delta_dev, "SPG_DELTA_DEV", ON, true, kNoLo, kNoHi, 0, "a device DotProductProofLog's delta scalars from the device Bullet state; 0: host cw and upload") \
  X(delta_comb, "SPG_DELTA_COMB", ON, true, kNoLo, kNoHi, 0, "the device delta MSM from the comb table") \
  /* ---- A/B and parity forms: sumcheck and the R1CS prover */ \
  X(sc_quad_max, "SPG_SC_QUAD_MAX", LONG, 65536, kNoLo, kNoHi, 0, "round evaluations over at most this many points take the quad form (0: never)") \
  X(sc_grid, "SPG_SC_GRID", INT, 1024, 1, 4096, 0, "most workgroups of a round's evaluation (at most kScGridMax)") \
  X(eq_lds, "SPG_EQ_LDS", ON, true, kNoLo, kNoHi, 0, "eq tables by the LDS kernel; 0: one lane per entry") \
  X(eq_multi, "SPG_EQ_MULTI", ON, true, kNoLo, kNoHi, 0, "eq tables needed together share one launch, up to three per launch") \
  X(p1_rows, "SPG_P1_ROWS", ON, true, kNoLo, kNoHi, 0, "phase-1 x rounds over rows of >= 128 points take the row-factored kernel") \
  X(tape_ahead, "SPG_TAPE_AHEAD", ON, true, kNoLo, kNoHi, 0, "ZKRounds computes every round's randomness-only points in one burst at init") \
  X(sc_fuse, "SPG_SC_FUSE", ON, true, kNoLo, kNoHi, 0, "a round's fold rides in the next round's evaluation; 0: the separate fold launch") \
  X(z_tiled, "SPG_Z_TILED", ON, true, kNoLo, kNoHi, 0, "k_z_fill_tiled when every instance's row is whole 256-element tiles") \
  X(z_side, "SPG_Z_SIDE", ON, true, kNoLo, kNoHi, 0, "the Z fill runs on the second stream beside phase 1; 0: in order") \
  X(z_after, "SPG_Z_AFTER", LONG, 4, kNoLo, kNoHi, 0, "the phase-1 round whose evaluation the side-stream Z fill is queued after") \
  X(spmv_tiled, "SPG_SPMV_TILED", ON, true, kNoLo, kNoHi, 0, "k_spmv<true> when every instance's q rows are whole 256-row tiles") \
  X(p1_pair, "SPG_P1_PAIR", ON, true, kNoLo, kNoHi, 0, "two phase-1 rounds per launch (k_phase1_pair); 0: one per launch") \
  X(p1_pair_max, "SPG_P1_PAIR_MAX", LONG, 8192, kNoLo, kNoHi, 0, "points of a phase-1 pair's second round (at most kP1PairMax)") \
  X(sigma_ahead, "SPG_SIGMA_AHEAD", ON, true, kNoLo, kNoHi, 0, "every point of the three sigma protocols in one host burst ahead of the transcript sequence") \
  X(q_bound_all, "SPG_Q_BOUND_ALL", ON, true, kNoLo, kNoHi, 0, "every q fold of Z in one pass (k_pqx_bound_q); 0: one launch per challenge") \
  X(p2_pair, "SPG_P2_PAIR", ON, true, kNoLo, kNoHi, 0, "two phase-2 y rounds per launch (k_phase2_pair); 0: one per launch") \
  X(p2_pair_max, "SPG_P2_PAIR_MAX", LONG, 8192, kNoLo, kNoHi, 0, "elements of a phase-2 pair (at most kP1PairMax)") \
  X(wit_in_place, "SPG_WIT_IN_PLACE", ON, true, kNoLo, kNoHi, 0, "witness parts resident on this device are read in place, not copied") \
  X(cq_side, "SPG_CQ_SIDE", ON, true, kNoLo, kNoHi, 1, "SNARK::prove's commit queue runs its other rows on the second stream") \
  /* ---- A/B and parity forms: SPARK layers */ \
  X(tree_top, "SPG_TREE_TOP", LONG, 1024, kNoLo, kNoHi, 0, "product-tree levels of more products per circuit get a grid-wide launch each") \
  X(layer_onewg, "SPG_LAYER_ONEWG", INT, 512, kNoLo, kNoHi, 0, "fused layer rounds of at most this many elements run in one workgroup") \
  X(layer_ept, "SPG_LAYER_EPT", INT, 2, 1, kNoHi, 0, "fused layer rounds: elements per thread of the wider grids") \
  X(layer_quad, "SPG_LAYER_QUAD", ON, true, kNoLo, kNoHi, 0, "layer rounds a quad per element; 0: a lane per element") \
  X(layer_ends, "SPG_LAYER_ENDS", ON, true, kNoLo, kNoHi, 0, "a layer's last round posts the final entries itself") \
  X(layer_pair, "SPG_LAYER_PAIR", ON, true, kNoLo, kNoHi, 0, "two layer rounds per launch where they are small") \
  X(layer_triple, "SPG_LAYER_TRIPLE", ON, true, kNoLo, kNoHi, 0, "three layer rounds per launch where they are small") \
  X(wide_min, "SPG_WIDE_MIN", LONG, 524288, kNoLo, kNoHi, 0, "thread-elements from which a layer round takes the throughput form") \
  X(pair_bs, "SPG_PAIR_BS", INT, 0, kNoLo, kNoHi, 0, "64: paired launches over 64-thread workgroups") \
  X(pair_max, "SPG_PAIR_MAX", LONG, 4096, kNoLo, kNoHi, 0, "elements of a paired launch (at most 6144; 1536 with SPG_PAIR_BS=64)") \
  X(triple_max, "SPG_TRIPLE_MAX", LONG, 384, kNoLo, kNoHi, 0, "elements of a tripled launch (at most 384)") \
  X(step_costs, "SPG_STEP_COSTS", COSTS, (StepCosts{{18, 25, 30}}), kNoLo, kNoHi, 0, "relative wall of a single / paired / tripled round trip, for the launch plan") \
  X(layer_desc_copy, "SPG_LAYER_DESC_COPY", PRESENT, false, kNoLo, kNoHi, 1, "layer descriptors always by a copy, never in the kernel arguments")
// clang-format on

// ---- the parse rules
inline bool parse_on(const char* t, bool, long, long) { return !t || atoi(t) != 0; }
inline bool parse_off(const char* t, bool, long, long) { return t && atoi(t) != 0; }
inline bool parse_present(const char* t, bool, long, long) { return t != nullptr; }
inline int parse_int(const char* t, int d, long lo, long hi) {
  return t ? (int)std::max(lo, std::min(hi, (long)atoi(t))) : d;
}
inline long parse_long(const char* t, long d, long lo, long hi) { return t ? std::max(lo, std::min(hi, atol(t))) : d; }
inline size_t parse_gb(const char* t, double d, long, long) { return (size_t)(t ? atof(t) : d) * ((size_t)1 << 30); }
inline const char* parse_str(const char* t, const char* d, long, long) { return t ? t : d; }
inline StepCosts parse_costs(const char* t, StepCosts d, long, long) {
  if (t) sscanf(t, "%d,%d,%d", &d.c[0], &d.c[1], &d.c[2]);
  return d;
}

#define SPG_KNOB_T_ON bool
#define SPG_KNOB_T_OFF bool
#define SPG_KNOB_T_PRESENT bool
#define SPG_KNOB_T_INT int
#define SPG_KNOB_T_LONG long
#define SPG_KNOB_T_GB size_t
#define SPG_KNOB_T_STR CStr
#define SPG_KNOB_T_COSTS StepCosts
#define SPG_KNOB_P_ON parse_on
#define SPG_KNOB_P_OFF parse_off
#define SPG_KNOB_P_PRESENT parse_present
#define SPG_KNOB_P_INT parse_int
#define SPG_KNOB_P_LONG parse_long
#define SPG_KNOB_P_GB parse_gb
#define SPG_KNOB_P_STR parse_str
#define SPG_KNOB_P_COSTS parse_costs

// ---- the accessors (id_dflt: for a site's static_assert against the constant its default stands for)
#define SPG_KNOB_ACCESSORS(id, name, kind, dflt, lo, hi, live, desc)                  \
  constexpr auto id##_dflt = dflt;                                                    \
  inline SPG_KNOB_T_##kind id() {                                                     \
    if (live) return SPG_KNOB_P_##kind(getenv(name), dflt, lo, hi);                   \
    static const SPG_KNOB_T_##kind v = SPG_KNOB_P_##kind(getenv(name), dflt, lo, hi); \
    return v;                                                                         \
  }                                                                                   \
  inline bool id##_is_set() {                                                         \
    if (live) return getenv(name) != nullptr;                                         \
    static const bool s = getenv(name) != nullptr;                                    \
    return s;                                                                         \
  }
SPG_KNOBS(SPG_KNOB_ACCESSORS)
#undef SPG_KNOB_ACCESSORS

// ---- the table as data (hostcheck.cpp's spgh_knob_table; tests/test_knobs.py)
struct Row {
  const char* name;
  const char* kind;
  std::string dflt;
  long lo, hi;  // the clamp applied when set (kNoLo / kNoHi: none)
  bool live;
  const char* desc;
};
inline std::string dflt_text(bool b) { return b ? "on" : "off"; }
inline std::string dflt_text(int v) { return std::to_string(v); }
inline std::string dflt_text(long v) { return std::to_string(v); }
inline std::string dflt_text(double gb) { return std::to_string((long)gb); }
inline std::string dflt_text(const char* s) { return s ? s : "unset"; }
inline std::string dflt_text(Unset) { return "unset"; }
inline std::string dflt_text(const StepCosts& c) {
  return std::to_string(c.c[0]) + "," + std::to_string(c.c[1]) + "," + std::to_string(c.c[2]);
}
inline std::vector<Row> table() {
  std::vector<Row> t;
#define SPG_KNOB_ROW(id, name, kind, dflt, lo, hi, live, desc) t.push_back(Row{name, #kind, dflt_text(dflt), lo, hi, live != 0, desc});
  SPG_KNOBS(SPG_KNOB_ROW)
#undef SPG_KNOB_ROW
  return t;
}

}  // namespace knob
}  // namespace spg
