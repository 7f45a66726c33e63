// spg — every workspace slot of a context, declared once. ws_get(ctx, Ws::X, bytes) hands out one cached device block
// per row (and per stream, ctx.hpp); a new buffer is one row of SPG_WS_SLOTS below. Numbers follow from the position
// in the table and nothing outside ws_get may depend on them. Pure host header (hostcheck.cpp's spgh_ws_table).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace spg {

//  X(name, "owner file", "what it holds")
#define SPG_WS_SLOTS(X) \
  /* fixed-base MSM pipelines */ \
  X(MsmScalars, "msm.hip", "uploaded scalars (and the row outputs behind them)") \
  X(MsmHist, "msm.hip", "bucket histogram") \
  X(MsmOff, "msm.hip", "bucket offsets (exclusive scan of the histogram)") \
  X(MsmCursor, "msm.hip", "per-bucket fill cursors") \
  X(MsmItems, "msm.hip", "work items per bucket") \
  X(MsmItemOff, "msm.hip", "item offsets") \
  X(MsmEntries, "msm.hip", "bucket entries (point indices)") \
  X(MsmItemKey, "msm.hip", "bucket key of each work item") \
  X(MsmPartial, "msm.hip", "partial sums per work item") \
  X(MsmSegT, "msm.hip", "running-sum segments T") \
  X(MsmSegS, "msm.hip", "running-sum segments S") \
  X(MsmScanTmp, "msm.hip", "hipcub scan temporary") \
  X(MsmOut, "msm.hip", "compressed results") \
  X(MsmLatBuckets, "msm.hip", "bucket sums of the latency path") \
  X(MsmSmallExt, "msm.hip", "extended results of small batched rows") \
  X(MsmLatExt, "msm.hip", "extended results of the latency path") \
  X(MsmRowExt, "msm.hip", "extended results per row ahead of encoding") \
  X(MsmRunT, "msm.hip", "per-group running sums of the final reduction") \
  X(MsmOneExt, "msm.hip", "the single extended result of one commitment") \
  X(MsmBigDigits, "msm_big.hip", "signed digits") \
  X(MsmBigHist, "msm_big.hip", "bucket histogram") \
  X(MsmBigOff, "msm_big.hip", "bucket offsets") \
  X(MsmBigEntries, "msm_big.hip", "bucket entries") \
  X(MsmBigChunks, "msm_big.hip", "chunk descriptors") \
  X(MsmBigFirst, "msm_big.hip", "first chunk of each bucket") \
  X(MsmBigSums, "msm_big.hip", "chunk sums") \
  X(MsmBigScanTmp, "msm_big.hip", "hipcub scan temporary") \
  X(MsmBigGroupCnt, "msm_big.hip", "group completion counters") \
  X(VmsmScalars, "msm_var.hip", "uploaded scalars") \
  X(VmsmDigits, "msm_var.hip", "signed digits") \
  X(VmsmHist, "msm_var.hip", "bucket histogram") \
  X(VmsmOff, "msm_var.hip", "bucket offsets") \
  X(VmsmEntries, "msm_var.hip", "bucket entries") \
  X(VmsmChunks, "msm_var.hip", "chunk descriptors") \
  X(VmsmNumChunks, "msm_var.hip", "chunks per MSM") \
  X(VmsmFirst, "msm_var.hip", "first chunk of each bucket") \
  X(VmsmSums, "msm_var.hip", "chunk sums") \
  X(VmsmGroupCnt, "msm_var.hip", "group completion counters") \
  X(VmsmScanTmp, "msm_var.hip", "hipcub scan temporary") \
  X(VmsmGroups, "msm_var.hip", "group sums") \
  X(VmsmDesc, "msm_var.hip", "MSM descriptors and block map") \
  X(CombPart, "comb.hip", "partial sums of comb rows split over workgroups") \
  /* sigma protocols and Bullet */ \
  X(ProtoScalars, "proto.hip", "uploaded scalars of a sigma-protocol MSM batch") \
  X(ProtoIdx, "proto.hip", "generator indices") \
  X(ProtoBuckets, "proto.hip", "bucket sums of the batch") \
  X(ProtoBulletState, "proto.hip", "Bullet reduction's vectors (aa[2], cw[2])") \
  X(ProtoDotScalars, "proto.hip", "scalars of a host-side dot-product commitment") \
  /* sumchecks */ \
  X(ScEqHalves, "sumcheck.hip", "the two half tables of a split eq polynomial") \
  X(PqxA, "sumcheck.hip", "Pqx instance descriptors, first operand") \
  X(PqxB, "sumcheck.hip", "Pqx instance descriptors, second operand") \
  /* R1CSProof::prove */ \
  X(R1csAz, "r1cs_tables.hip", "Az") \
  X(R1csBz, "r1cs_tables.hip", "Bz") \
  X(R1csCz, "r1cs_tables.hip", "Cz") \
  X(R1csZ, "r1cs_tables.hip", "the Z table") \
  X(R1csAbc, "r1cs.hip", "the bound ABC table of phase 2") \
  X(R1csTp, "r1cs.hip", "eq table over p") \
  X(R1csTq, "r1cs.hip", "eq table over q") \
  X(R1csTx, "r1cs.hip", "eq table over x") \
  X(R1csEqRx, "r1cs.hip", "eq(rx)") \
  X(R1csEqP, "r1cs.hip", "eq(rp)") \
  X(R1csPart, "r1cs.hip", "per-workgroup round partials") \
  X(R1csOut3, "r1cs.hip", "a round's three evaluations") \
  X(R1csDesc, "r1cs_tables.hip", "instance descriptors") \
  X(R1csL, "r1cs.hip", "L vectors of the witness openings") \
  X(R1csBoundPart, "r1cs.hip", "partial bound rows") \
  X(R1csBoundOut, "r1cs.hip", "bound rows (LZ)") \
  X(R1csEvRx, "r1cs_seams.hip", "eq(rx) of the matrix evaluations") \
  X(R1csEvRy, "r1cs_seams.hip", "eq(ry) of the matrix evaluations") \
  X(R1csEvPart, "r1cs_seams.hip", "partial matrix evaluations") \
  X(R1csEvOut, "r1cs_seams.hip", "matrix evaluations") \
  X(R1csEvDesc, "r1cs_seams.hip", "matrix descriptors") \
  X(R1csC1, "r1cs.hip", "phase 1 claim vectors") \
  X(R1csC2, "r1cs.hip", "phase 2 claim vectors") \
  X(R1csTq2, "r1cs.hip", "second eq table over q") \
  X(R1csTx2, "r1cs.hip", "second eq table over x") \
  X(R1csAbc2, "r1cs.hip", "second ABC table") \
  X(R1csEqQ, "r1cs.hip", "eq(rq)") \
  X(SatRec, "satcheck.hip", "the first unsatisfied row's record") \
  X(SatDesc, "satcheck.hip", "instance descriptors") \
  /* Hyrax commitments and PolyEvalProof */ \
  X(Commit, "hyrax.hip", "compressed row commitments of one chunk") \
  X(CommitBk, "hyrax.hip", "bucket sums of latency-path rows") \
  X(CommitExt, "hyrax.hip", "extended row commitments ahead of encoding") \
  X(MultiExt, "hyrax.hip", "extended commitments of commit_rows_many") \
  X(MultiOut, "hyrax.hip", "compressed commitments of commit_rows_many") \
  X(BoundL, "hyrax.hip", "L of poly_eval_prove") \
  X(BoundPart, "hyrax.hip", "partial bound rows") \
  X(Bound, "hyrax.hip", "the bound row LZ") \
  X(PeJobs, "polyeval.hip", "bound jobs") \
  X(PeSums, "polyeval.hip", "sum descriptors") \
  X(PeL, "polyeval.hip", "L vectors") \
  X(PePart, "polyeval.hip", "partial bound rows") \
  X(PeOut, "polyeval.hip", "bound rows") \
  X(PeBlinds, "polyeval.hip", "row blinds") \
  X(PeRagTerms, "polyeval.hip", "terms of ragged sums") \
  /* product circuits and layer sumchecks */ \
  X(SegPart, "layers.hip, spark.hip", "per-workgroup partial dot products") \
  X(Seg, "layers.hip, spark.hip", "dot products per segment") \
  X(LayerC, "layers.hip", "claim vector, first buffer") \
  X(LayerC2, "layers.hip", "claim vector, second buffer") \
  X(LayerTriples, "layers.hip", "triple descriptors and coefficients") \
  X(LayerPart, "layers.hip", "per-workgroup round partials") \
  X(LayerGather, "layers.hip", "entries gathered from the ranks of a sharded layer") \
  X(ProdcDesc, "prodc.hip", "uploaded descriptors") \
  X(ProdcTmp, "prodc.hip", "copies of the layers a proof folds in place") \
  X(ProdcTops, "prodc.hip", "circuit products") \
  /* SPARK */ \
  X(SparkMemRx, "spark.hip", "eq(rx) over the cells") \
  X(SparkMemRy, "spark.hip", "eq(ry) over the cells") \
  X(SparkDerefs, "spark.hip", "derefs, zero-padded") \
  X(SparkTreeOps, "spark.hip", "product trees of the ops circuits") \
  X(SparkTreeMem, "spark.hip", "product trees of the memory circuits") \
  X(SparkDotp, "spark.hip", "inputs of the dot-product circuits") \
  X(SparkEqOps, "spark.hip", "eq(rand_ops)") \
  X(SparkEqMem, "spark.hip", "eq(rand_mem)") \
  X(SparkTops, "spark.hip", "circuit products") \
  X(SparkTopOps, "spark.hip", "sharded top levels of the ops circuits") \
  X(SparkTopMem, "spark.hip", "sharded top levels of the memory circuits") \
  X(SparkTsKeys, "spark.hip", "AddrTimestamps sort keys, ops and counts") \
  X(SparkTsTemp, "spark.hip", "hipcub sort / scan temporary") \
  /* SNARK, verifier, seams */ \
  X(SnarkRowsIn, "snark.hip", "staged scalars of the witness rows outside the early group") \
  X(SnarkEarlyIn, "snark.hip", "staged scalars of the early group (the block witnesses)") \
  X(SnarkEarlyOut, "snark.hip", "compressed row commitments of the early group") \
  X(SnarkEarlyExt, "snark.hip", "halved comb points of the early group, encoded on the host") \
  X(VerifyZ, "verify.hip", "uploaded evaluation vector") \
  X(EqsIn, "eqcheck.hip", "packed equations") \
  X(EqsProd, "eqcheck.hip", "term products") \
  X(EqsOut, "eqcheck.hip", "verdicts") \
  X(SeamPart, "seams.hip", "per-workgroup round partials") \
  X(SeamTmp, "seams.hip", "scratch vector of a seam") \
  X(SeamRev, "seams.hip", "uploaded reversed table") \
  X(SeamRevDesc, "seams.hip", "reversed-table descriptors") \
  X(SeamEq, "seams.hip", "eq table of a seam")

enum class Ws : uint16_t {
#define SPG_WS_ENUM(name, owner, what) name,
  SPG_WS_SLOTS(SPG_WS_ENUM)
#undef SPG_WS_ENUM
  kCount
};

struct WsRow {
  const char* name;
  const char* owner;
  const char* what;
};
inline const WsRow* ws_table() {
  static const WsRow t[] = {
#define SPG_WS_ROW(name, owner, what) {#name, owner, what},
      SPG_WS_SLOTS(SPG_WS_ROW)
#undef SPG_WS_ROW
  };
  return t;
}
inline const char* ws_name(Ws s) { return s < Ws::kCount ? ws_table()[(size_t)s].name : "?"; }

}  // namespace spg
