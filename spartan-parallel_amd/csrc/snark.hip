// spg — SNARK::prove (src/lib.rs:971-2746): the orchestration around the device-resident R1CSProof, SPARK
// and Hyrax kernels.
//
//   SNARK::multi_encode / encode      src/lib.rs:793-829, src/r1csinstance.rs:654-737    spg_snark_encode
//   witness upload (block_vars, exec inputs stay in HBM)                                  spg_snark_witness_new
//   SNARK::prove                      src/lib.rs:971-2746                                 spg_snark_prove
//     instance commitments -> transcript, block / pairwise sort and padding             (host, O(#instances))
//     permutation / memory witnesses w2, w3, w3_shifted    lib.rs:1299-1955, 831-968    (host, O(Q * 8))
//     Hyrax commitments of every witness polynomial        lib.rs:1957-2221             commit_dev (device MSMs)
//     three R1CSProof::prove + multi_evaluate + R1CSEvalProof                             r1cs.hip, r1cs_seams.hip / spark.hip
//     perm product, shift and IO PolyEvalProofs            lib.rs:2534-2693, 187-446    polyeval.hip (pe_prove.hpp)
// The host side is the transcript, the small witness recurrences and the bincode writer; every O(N) table
// (block_vars, Az/Bz/Cz, SPARK dense representations) lives in HBM. SnarkProver::run calls one stage per section
// of the reference; what the verifier derives from the same public sizes is in snark_shape.hpp.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "hostpoly.hpp"
#include "knobs.hpp"
#include "pe_plan.hpp"
#include "pe_prove.hpp"
#include "proto.hpp"
#include "satcheck.hpp"
#include "snark_shape.hpp"

using namespace spg;

namespace {

typedef std::vector<FqV> Rows;  // w_mat of one instance: rows (executions) of scalars

FqV flatten(const Rows& m) {
  FqV v;
  for (auto& r : m) v.insert(v.end(), r.begin(), r.end());
  return v;
}
Rows shift_rows(const Rows& m, size_t width) {
  Rows s(m.begin() + 1, m.end());
  s.push_back(FqV(width, fq_zero()));
  return s;
}
FqV pad_pow2(FqV v) {  // DensePolynomial::new pads to a power of two (dense_mlpoly.rs:152-161)
  v.resize(npow2(std::max<size_t>(v.size(), 1)), fq_zero());
  return v;
}

}  // namespace

// ------------------------------------------------------------------------------------ handles
// SNARK::encode / multi_encode of one R1CS instance: the host matrices, the SPARK decommitments in HBM, the
// device instance (unsorted, for multi_evaluate) and a cache of the sorted device instance.
struct spg_snark_comp {
  size_t num_instances = 0, max_num_cons = 0, num_vars = 0;
  std::vector<size_t> num_cons, nnz;
  std::vector<std::vector<spg_sparse_entry>> mats;  // [3p + m]
  std::vector<std::vector<size_t>> label_map;
  std::vector<spg_spark*> sparks;
  spg_r1cs_inst* dev = nullptr;
  spg_r1cs_inst* dev_sorted = nullptr;
  std::vector<size_t> sorted_order;
  std::vector<size_t> cols_needed;  // block_cols_needed for section width cols_needed_stride (spg_snark_prove's check)
  size_t cols_needed_stride = 0;
  spg_r1cs_instance view(const std::vector<size_t>& order, std::vector<const spg_sparse_entry*>* ptrs,
                         std::vector<size_t>* nnz_o, std::vector<size_t>* nc_o) const {
    ptrs->clear();
    nnz_o->clear();
    nc_o->clear();
    for (size_t i : order) {
      nc_o->push_back(num_cons[i]);
      for (int m = 0; m < 3; m++) {
        ptrs->push_back(mats[3 * i + m].data());
        nnz_o->push_back(mats[3 * i + m].size());
      }
    }
    spg_r1cs_instance ci;
    ci.num_instances = order.size();
    ci.max_num_cons = max_num_cons;
    ci.num_vars = num_vars;
    ci.num_cons = nc_o->data();
    ci.nnz = nnz_o->data();
    ci.entries = ptrs->data();
    return ci;
  }
};

// the run-time inputs of SNARK::prove, with block_vars and exec_inputs resident in HBM
struct spg_snark_wit {
  spg_snark_inputs a;  // sizes and scalars (pointer fields below are owned copies)
  std::vector<uint8_t> liveness;
  FqV input;
  Fq output;
  std::vector<size_t> phy_ops, vir_ops, nvars, nproofs;
  std::vector<Rows> block_io;  // [b][q] first 2 * num_inputs_unpadded entries of every block_vars row
  std::vector<Fq*> d_block_vars;
  std::vector<size_t> d_block_bytes;  // their allocation sizes (dev_cache_put on free)
  Rows exec, init_phy, init_vir, addr_phy, addr_vir, ts_bits;
  Fq* d_exec = nullptr;
};

// R1CSProof bincode + challenges (rp, rq_rev, rx, rw||ry)
struct SatOut {
  std::vector<uint8_t> bytes;
  FqV ch[4];
};

namespace {

int snark_comp_free(spg_ctx* ctx, spg_snark_comp* C) {
  if (!C) return SPG_OK;
  for (auto* s : C->sparks) spg_spark_free(ctx, s);
  spg_r1cs_inst_free(ctx, C->dev);
  spg_r1cs_inst_free(ctx, C->dev_sorted);
  delete C;
  return SPG_OK;
}

// R1CSProof::prove through the device prover (r1cs.hip)
int sat_prove(spg_ctx* ctx, spg_r1cs_gens* gens, spg_r1cs_inst* inst, size_t P, size_t max_np,
              const std::vector<size_t>& num_proofs, size_t max_ni, const std::vector<size_t>& num_inputs,
              const std::vector<WPart>& secs, spg_r1cs_witness** W, spg_transcript* t, spg_random_tape* tape,
              SatOut* out) {
  Laps lp;
  lp.title = "sat_prove";
  lp.on = lp.on && knob::trace() >= 2;
  int rc = witness_from_parts(ctx, secs, W);
  if (rc) return rc;
  lp.lap("witness_from_parts");
  lp.print();
  // output staging kept across proves: a fresh 4 MB vector is zero-filled on every call, and when glibc serves it from
  // new pages that is ~1000 page faults (~0.8 ms in the SNARK's kernel trace, the device idle meanwhile)
  static thread_local std::vector<uint8_t> buf;
  static thread_local std::vector<uint64_t> ch;
  if (buf.size() < ((size_t)1 << 22)) buf.resize((size_t)1 << 22);
  if (ch.size() < 4 * 4096) ch.resize(4 * 4096);
  size_t len = 0, chl[4] = {0, 0, 0, 0};
  rc = spg_r1cs_prove(ctx, gens, inst, P, max_np, num_proofs.data(), max_ni, num_inputs.data(), *W, t, tape,
                      buf.data(), buf.size(), &len, ch.data(), chl);
  if (rc) return rc;
  out->bytes.assign(buf.begin(), buf.begin() + len);
  size_t o = 0;
  for (int k = 0; k < 4; k++) {
    out->ch[k].clear();
    for (size_t i = 0; i < chl[k]; i++) out->ch[k].push_back(ld_fq(&ch[4 * (o + i)]));
    o += chl[k];
  }
  return 0;
}

// R1CSInstance::multi_evaluate on the unsorted device instance (3 evals per instance)
int multi_eval(spg_ctx* ctx, spg_snark_comp* C, const FqV& rx, const FqV& ry, FqV* out) {
  std::vector<uint64_t> a(4 * rx.size()), b(4 * ry.size()), o(4 * 3 * C->num_instances);
  for (size_t i = 0; i < rx.size(); i++) st_fq(&a[4 * i], rx[i]);
  for (size_t i = 0; i < ry.size(); i++) st_fq(&b[4 * i], ry[i]);
  int rc = spg_r1cs_multi_evaluate(ctx, C->dev, a.data(), rx.size(), b.data(), ry.size(), o.data());
  if (rc) return rc;
  out->clear();
  for (size_t i = 0; i < 3 * C->num_instances; i++) out->push_back(ld_fq(&o[4 * i]));
  return 0;
}
// multi_evaluate_bound_rp (r1csinstance.rs:597-630) from the unsorted list and the sort order
void bound_rp(const FqV& list, const std::vector<size_t>& order, const FqV& rp, Fq out[3]) {
  for (int m = 0; m < 3; m++) {
    FqV v;
    for (size_t i : order) v.push_back(list[3 * i + m]);
    out[m] = dense_eval_host(v, rp);
  }
}

int ensure_sorted(spg_ctx* ctx, spg_snark_comp* C, const std::vector<size_t>& order) {
  if (C->dev_sorted && C->sorted_order == order) return 0;
  spg_r1cs_inst_free(ctx, C->dev_sorted);
  C->dev_sorted = nullptr;
  std::vector<const spg_sparse_entry*> ptrs;
  std::vector<size_t> nnz, nc;
  spg_r1cs_instance ci = C->view(order, &ptrs, &nnz, &nc);
  int rc = spg_r1cs_inst_new(ctx, &ci, &C->dev_sorted);
  if (rc) return rc;
  C->sorted_order = order;
  return 0;
}

// R1CSCommitment::append_to_transcript (r1csinstance.rs:64-70) of group g
void append_r1cs_comm(const spg_snark_comp* C, size_t g, Tr& t) {
  t.u64("num_cons", C->num_instances * C->max_num_cons);
  t.u64("num_vars", C->num_vars);
  spark_comm_append(C->sparks[g], t);
}

struct SecInfo {  // sizes + data pointers for merges (ProverWitnessSecInfo::merge / concat, lib.rs:546-604)
  std::vector<size_t> num_proofs, num_inputs;
  std::vector<const Fq*> src;  // host or device data of each instance
  std::vector<const FqV*> poly;  // host polynomial (nullptr for device-only data)
  void push(size_t np, size_t ni, const Fq* data, const FqV* p) {
    num_proofs.push_back(np);
    num_inputs.push_back(ni);
    src.push_back(data);
    poly.push_back(p);
  }
};
// im (optional): the component each merged instance came from
int merge(spg_ctx* ctx, const std::vector<const SecInfo*>& comps, SecInfo* s, std::vector<size_t>* im = nullptr) {
  std::vector<const std::vector<size_t>*> sizes;
  for (auto c : comps) sizes.push_back(&c->num_proofs);
  std::vector<size_t> map;
  if (!merge_order(sizes, &map)) return set_err(ctx, SPG_E_ARG, "witness section sizes: an instance without proofs");
  *s = SecInfo();
  std::vector<size_t> ptr(comps.size(), 0);
  for (size_t c : map) {
    const size_t k = ptr[c]++;
    s->push(comps[c]->num_proofs[k], comps[c]->num_inputs[k], comps[c]->src[k], comps[c]->poly[k]);
  }
  if (im) *im = map;
  return 0;
}
SecInfo concat(const std::vector<const SecInfo*>& comps) {
  SecInfo s;
  for (auto c : comps)
    for (size_t k = 0; k < c->num_proofs.size(); k++) s.push(c->num_proofs[k], c->num_inputs[k], c->src[k], c->poly[k]);
  return s;
}
WPart wpart(const SecInfo& s) { return {s.num_proofs, s.num_inputs, s.src}; }

// Hyrax commitments of the witness polynomials of SNARK::prove, deferred so that all rows of one width go to
// the device in one MSM launch; flush() appends them to the transcript in the order they were added (every
// commitment between challenge_r and the block R1CSProof depends only on the witness and tau, r).
struct CQ {
  struct Item {
    const FqV* host;
    const Fq* dev;
    size_t len;
    std::vector<Pt>* out;
  };
  std::vector<Item> items;
  // Early group: device-resident polynomials (the block witnesses) whose rows are committed by one batch MSM
  // launched before the host builds the permutation witnesses, so the device works while the host does;
  // flush() only downloads those rows. Their commitments depend on the witness alone, never on the
  // transcript, and they are recomputed in every prove.
  std::vector<const Fq*> early_dev;
  size_t early_L = 0;
  uint8_t* early_out = nullptr;
  const Ext* early_ext = nullptr;  // halved comb points (encoded on the host at flush), else early_out's encodings
  // the rows of every item outside the early group: launched (uploads and points), then finished (encodings; the
  // host may encode the early group in between)
  std::vector<std::vector<Pt>> rows;
  std::vector<RowJob> jobs;
  RowsPending pend;

  // the Hyrax row width of a polynomial of `len` scalars: 2^(nv - nv / 2)
  static size_t row_width(size_t len) { return (size_t)1 << (lg2(len) - lg2(len) / 2); }
  // ctx->stream is `s` until the scope ends, on every path out of it
  struct StreamScope {
    spg_ctx* c;
    hipStream_t prev;
    StreamScope(spg_ctx* ctx, hipStream_t s) : c(ctx), prev(ctx->stream) { c->stream = s; }
    ~StreamScope() { c->stream = prev; }
  };
  bool is_early(const Item& it) const {
    return it.dev && std::find(early_dev.begin(), early_dev.end(), it.dev) != early_dev.end();
  }
  void add(const FqV& v, std::vector<Pt>* out) { items.push_back({&v, nullptr, v.size(), out}); }
  void add_dev(const Fq* d, size_t len, std::vector<Pt>* out) { items.push_back({nullptr, d, len, out}); }

  int launch_early(spg_ctx* ctx, ProverGens& g, const std::vector<std::pair<const Fq*, size_t>>& its) {
    size_t R = 0, total = 0;
    for (auto& it : its) {
      if (R && row_width(it.second) != R) return 0;  // one width only; otherwise flush() groups them as usual
      R = row_width(it.second);
      total += it.second;
    }
    // the one-launch batch path of commit_rows only (rows wider than the latency path, one chunk)
    if (its.empty() || R <= 256 || R > g.n_pc || total / R > ((size_t)1 << 24) / R) return 0;
    Fq* d = (Fq*)ws_get(ctx, Ws::SnarkEarlyIn, total * sizeof(Fq) + 64);
    uint8_t* out = (uint8_t*)ws_get(ctx, Ws::SnarkEarlyOut, 32 * (total / R) + 64);
    if (!d || !out) return set_err(ctx, SPG_E_NOMEM, "early commit staging");
    SPG_HIP(ctx, hipEventRecord(ctx->ev_pre, ctx->stream));  // flush()'s side stream starts from here
    size_t o = 0;
    for (auto& it : its) {
      SPG_HIP(ctx, hipMemcpyAsync(d + o, it.first, it.second * sizeof(Fq), hipMemcpyDeviceToDevice, ctx->stream));
      o += it.second;
    }
    // the comb rows with halved scalars: flush() encodes the points' doubles on the host in one batch (~50 us on the
    // pool for 1024 rows) instead of a k_compress_ext launch (~140 us of dependent squarings per lane)
    Ext* ext = knob::halved_enc() && total / R >= kHalvedMin ? (Ext*)ws_get(ctx, Ws::SnarkEarlyExt, sizeof(Ext) * (total / R) + 64) : nullptr;
    int rc = ext ? msm_comb(ctx, g.dev, 0, d, R, total / R, nullptr, nullptr, -1, ext, true) : kCombSkip;
    if (rc == kCombSkip) {
      ext = nullptr;
      rc = msm_batch_device(ctx, g.dev, 0, d, R, total / R, nullptr, out, nullptr, (long)(g.n_pc + 1));
    }
    if (rc) return rc;
    early_ext = ext;
    for (auto& it : its) early_dev.push_back(it.first);
    early_L = total / R;
    early_out = out;
    return 0;
  }

  int rows_launch(spg_ctx* ctx, ProverGens& g, const std::vector<size_t>& widths) {
    // one staging range per width, every width's rows committed together (the latency-path widths share one
    // encoding launch and one download)
    size_t total = 0;
    for (auto& it : items)
      if (!is_early(it)) total += it.len;
    Fq* d = (Fq*)ws_get(ctx, Ws::SnarkRowsIn, total * sizeof(Fq) + 64);
    if (total && !d) return set_err(ctx, SPG_E_NOMEM, "commit staging");
    rows.assign(widths.size(), {});
    jobs.clear();
    size_t o = 0;
    for (size_t w = 0; w < widths.size(); w++) {
      const size_t R = widths[w], o0 = o;
      for (auto& it : items) {
        if (is_early(it) || row_width(it.len) != R) continue;
        if (it.host)
          SPG_HIP(ctx, hipMemcpyAsync(d + o, it.host->data(), it.len * sizeof(Fq), hipMemcpyHostToDevice, ctx->stream));
        else
          SPG_HIP(ctx, hipMemcpyAsync(d + o, it.dev, it.len * sizeof(Fq), hipMemcpyDeviceToDevice, ctx->stream));
        o += it.len;
      }
      rows[w].resize((o - o0) / R);
      jobs.push_back({d + o0, R, (o - o0) / R, rows[w].data()});
    }
    return commit_rows_many_launch(ctx, g, jobs, &pend);
  }
  int rows_finish(spg_ctx* ctx, ProverGens& g, const std::vector<size_t>& widths) {
    int rc = commit_rows_many_finish(ctx, g, jobs, pend);
    if (rc) return rc;
    for (size_t w = 0; w < widths.size(); w++) {
      size_t ro = 0;
      for (auto& it : items) {
        if (is_early(it) || row_width(it.len) != widths[w]) continue;
        std::copy(rows[w].begin() + ro, rows[w].begin() + ro + it.out->size(), it.out->begin());
        ro += it.out->size();
      }
    }
    rows.clear();
    jobs.clear();
    return 0;
  }
  // the early group's encodings, downloaded (or encoded on the host from the halved points) into its items
  int early_collect(spg_ctx* ctx) {
    std::vector<Pt> enc(early_L);
    if (early_ext) {
      Ext* h = (Ext*)enc_stage_get(ctx, early_L * sizeof(Ext));
      if (!h) return set_err(ctx, SPG_E_NOMEM, "encoding staging");
      SPG_HIP(ctx, hipMemcpyAsync(h, early_ext, early_L * sizeof(Ext), hipMemcpyDeviceToHost, ctx->stream));
      SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
      encode_halved_host(h, early_L, enc.data());
      early_ext = nullptr;
    } else {
      SPG_HIP(ctx, hipMemcpyAsync(enc.data(), early_out, 32 * early_L, hipMemcpyDeviceToHost, ctx->stream));
      SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    size_t o = 0;
    for (const Fq* d : early_dev)  // rows in launch order
      for (auto& it : items)
        if (it.dev == d) {
          std::copy(enc.begin() + o, enc.begin() + o + it.out->size(), it.out->begin());
          o += it.out->size();
        }
    early_dev.clear();
    early_L = 0;
    return 0;
  }

  int flush(spg_ctx* ctx, ProverGens& g, Tr& t) {
    std::vector<size_t> widths;
    for (auto& it : items) {
      const size_t R = row_width(it.len);
      it.out->assign((size_t)1 << (lg2(it.len) / 2), Pt());
      if (!is_early(it) && std::find(widths.begin(), widths.end(), R) == widths.end()) widths.push_back(R);
    }
    // While the early MSM runs, the other rows go to the device on the second stream: their uploads and
    // latency-path MSMs then overlap it instead of queueing behind it. Rows of at most kSideMaxR scalars take
    // commit_rows' latency path, whose workspace slots, mapped buckets and staging the batch pipeline of the early
    // MSM never touches; wider rows stay on the main stream.
    static const size_t kSideMaxR = 256;
    bool side = knob::cq_side() && early_L > 0;
    for (size_t R : widths) side = side && R <= kSideMaxR;
    Laps lp;
    lp.title = "commit queue flush";
    lp.on = lp.on && knob::trace() >= 2;
    if (side) SPG_HIP(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_pre, 0));
    const hipStream_t rows_stream = side ? ctx->stream2 : ctx->stream;
    int rc;
    {
      StreamScope on(ctx, rows_stream);
      rc = rows_launch(ctx, g, widths);
    }
    if (rc) return rc;
    lp.lap(side ? "rows_side_launch" : "rows_launch");
    // the early group's encodings while the other rows' points are computed
    if (early_L && (rc = early_collect(ctx))) return rc;
    lp.lap("early_wait");
    {
      StreamScope on(ctx, rows_stream);
      rc = rows_finish(ctx, g, widths);
    }
    if (rc) return rc;
    lp.lap(side ? "rows_side_finish" : "rows_finish");
    for (auto& it : items) append_polycomm(t, "poly_commitment", *it.out);
    items.clear();
    lp.lap("append");
    lp.print();
    return 0;
  }
};

// the host witness polynomials of one section, one per instance: rows, DensePolynomial (flattened, padded), Hyrax
// commitment and the section's view for the R1CS witness
struct HostSec {
  std::vector<Rows> rows;
  std::vector<FqV> poly;
  std::vector<std::vector<Pt>> comm;
  SecInfo s;  // filled by queue(); empty for a memory list the program does not use
  explicit HostSec(size_t n = 1) : rows(n), poly(n), comm(n) {}
  // instance p's polynomial into the commit queue (the queue keeps pointers: this object stays where it is)
  void queue(CQ& q, size_t p = 0) {
    poly[p] = pad_pow2(flatten(rows[p]));
    q.add(poly[p], &comm[p]);
    s.push(rows[p].size(), rows[p][0].size(), poly[p].data(), &poly[p]);
  }
};
// (w2, w3, w3_shifted) of a permutation argument: perm-exec, the blocks, and each memory list (SNARK::mem_gen)
struct PermWit {
  HostSec w2, w3, w3s;
  explicit PermWit(size_t n = 1) : w2(n), w3(n), w3s(n) {}
  void set(size_t p, Rows r2, Rows r3) {
    w3s.rows[p] = shift_rows(r3, W3_WIDTH);
    w2.rows[p] = std::move(r2);
    w3.rows[p] = std::move(r3);
  }
  void queue(CQ& q) {  // a single instance's three commitments, in transcript order
    w2.queue(q);
    w3.queue(q);
    w3s.queue(q);
  }
};
}  // namespace

// ------------------------------------------------------------------------------------ C-ABI
extern "C" int spg_snark_encode(spg_ctx* ctx, const spg_snark_instance* si, int multi, spg_snark_comp** out) {
  if (!ctx || !si || !out || !si->inst.num_instances || !si->inst.nnz || !si->inst.entries) return SPG_E_ARG;
  const spg_r1cs_instance& ci = si->inst;
  spg_snark_comp* C = new spg_snark_comp();
  C->num_instances = ci.num_instances;
  C->max_num_cons = ci.max_num_cons;
  C->num_vars = ci.num_vars;
  C->num_cons.assign(ci.num_cons, ci.num_cons + ci.num_instances);
  for (size_t k = 0; k < 3 * ci.num_instances; k++) {
    C->nnz.push_back(ci.nnz[k]);
    C->mats.push_back(std::vector<spg_sparse_entry>(ci.entries[k], ci.entries[k] + ci.nnz[k]));
  }
  int rc = spg_r1cs_inst_new(ctx, &ci, &C->dev);
  if (rc) {
    snark_comp_free(ctx, C);
    return rc;
  }
  // R1CSCommitmentGens::new(label, P_pad, num_cons, num_vars_pad, nnz) (lib.rs:164-185, r1csinstance.rs:39-56)
  const size_t Pg = npow2(si->gens_num_instances);
  const size_t gens_nvx = lg2(Pg) + lg2(si->gens_num_cons), gens_nvy = lg2(npow2(si->gens_num_vars));
  const size_t gens_nnz = Pg * si->gens_num_nz_entries;
  const size_t nvx = lg2(ci.max_num_cons), nvy = lg2(ci.num_vars);
  std::vector<std::vector<SparsePoly>> groups;
  if (multi) {  // R1CSInstance::multi_commit: group by next_power_of_eight(nnz) (r1csinstance.rs:654-715)
    std::vector<size_t> sizes;
    for (size_t k = 0; k < 3 * ci.num_instances; k++) {
      size_t len = 1;
      while (len < npow2(ci.nnz[k])) len *= 8;
      size_t idx = std::find(sizes.begin(), sizes.end(), len) - sizes.begin();
      if (idx == sizes.size()) {
        sizes.push_back(len);
        C->label_map.push_back({});
        groups.push_back({});
      }
      C->label_map[idx].push_back(k);
      groups[idx].push_back({C->mats[k].data(), C->nnz[k]});
    }
  } else {
    groups.push_back({});
    C->label_map.push_back({});
    for (size_t k = 0; k < 3 * ci.num_instances; k++) {
      C->label_map[0].push_back(k);
      groups[0].push_back({C->mats[k].data(), C->nnz[k]});
    }
  }
  static const char kLabel[] = "gens_r1cs_eval";
  for (auto& g : groups) {
    spg_spark* S = nullptr;
    rc = spark_commit_polys(ctx, g, nvx, nvy, (const uint8_t*)kLabel, sizeof(kLabel) - 1, gens_nvx, gens_nvy, gens_nnz, 3,
                            &S);
    if (rc) {
      snark_comp_free(ctx, C);
      return rc;
    }
    C->sparks.push_back(S);
  }
  *out = C;
  return SPG_OK;
}
extern "C" int spg_snark_comp_free(spg_ctx* ctx, spg_snark_comp* C) { return snark_comp_free(ctx, C); }

// bincode(Vec<ComputationCommitment>) (as_list) or bincode(ComputationCommitment) of an encoded instance:
// R1CSCommitment { num_cons: num_instances * max_num_cons, num_vars, comm } (src/r1csinstance.rs:60-64, 700-705)
extern "C" int spg_snark_comm_bytes(spg_ctx* ctx, const spg_snark_comp* C, int as_list, uint8_t* out, size_t cap,
                                    size_t* len) {
  if (!ctx || !C || !len || C->sparks.empty()) return SPG_E_ARG;
  if (!as_list && C->sparks.size() != 1) return set_err(ctx, SPG_E_ARG, "several commitments: ask for the list");
  Writer w;
  if (as_list) w.u64(C->sparks.size());
  for (const spg_spark* S : C->sparks) {
    w.u64(C->num_instances * C->max_num_cons);
    w.u64(C->num_vars);
    spark_comm_ser(S, w);
  }
  *len = w.out.size();
  if (!out || w.out.size() > cap) return set_err(ctx, SPG_E_ARG, "commitment buffer too small");
  memcpy(out, w.out.data(), w.out.size());
  return SPG_OK;
}

// block_comm_map (src/lib.rs:2781): list g holds the matrix indices 3p + m that commitment g covers
extern "C" int spg_snark_comm_map(spg_ctx* ctx, const spg_snark_comp* C, size_t* idx, size_t idx_cap, size_t* lens,
                                  size_t lens_cap, size_t* n_lists) {
  if (!ctx || !C || !n_lists) return SPG_E_ARG;
  *n_lists = C->label_map.size();
  size_t tot = 0;
  for (auto& l : C->label_map) tot += l.size();
  if (!idx || !lens || tot > idx_cap || C->label_map.size() > lens_cap) return set_err(ctx, SPG_E_ARG, "map buffer too small");
  size_t o = 0;
  for (size_t g = 0; g < C->label_map.size(); g++) {
    lens[g] = C->label_map[g].size();
    for (size_t k : C->label_map[g]) idx[o++] = k;
  }
  return SPG_OK;
}

namespace spg {
// what SNARK::verify reads of an encoded instance (verify.hip)
spg_snark_comp* snark_comp_from_parts(size_t num_instances, size_t max_num_cons, size_t num_vars,
                                      std::vector<std::vector<size_t>> label_map, std::vector<spg_spark*> sparks) {
  spg_snark_comp* C = new spg_snark_comp();
  C->num_instances = num_instances;
  C->max_num_cons = max_num_cons;
  C->num_vars = num_vars;
  C->label_map = std::move(label_map);
  C->sparks = std::move(sparks);
  return C;
}
int snark_comp_view(const spg_snark_comp* C, SnarkCompView* v) {
  if (!C || C->sparks.empty() || C->label_map.size() != C->sparks.size()) return SPG_E_ARG;
  v->num_instances = C->num_instances;
  v->max_num_cons = C->max_num_cons;
  v->num_vars = C->num_vars;
  v->label_map = &C->label_map;
  v->sparks = &C->sparks;
  return 0;
}
}  // namespace spg

extern "C" int spg_snark_witness_new(spg_ctx* ctx, const spg_snark_inputs* a, spg_snark_wit** out) {
  if (!ctx || !a || !out || !a->block_num_instances_bound || !a->num_inputs_unpadded || !a->num_ios) return SPG_E_ARG;
  spg_snark_wit* W = new spg_snark_wit();
  W->a = *a;
  const size_t B = a->block_num_instances_bound, io = 2 * a->num_inputs_unpadded;
  W->liveness.assign(a->input_liveness, a->input_liveness + a->input_len);
  for (size_t i = 0; i < a->input_len; i++) W->input.push_back(ld_fq(a->input + 4 * i));
  W->output = ld_fq(a->output);
  W->phy_ops.assign(a->block_num_phy_ops, a->block_num_phy_ops + B);
  W->vir_ops.assign(a->block_num_vir_ops, a->block_num_vir_ops + B);
  W->nvars.assign(a->block_num_vars, a->block_num_vars + B);
  W->nproofs.assign(a->block_num_proofs, a->block_num_proofs + B);
  auto rows = [](const uint64_t* p, size_t n, size_t w, size_t keep) {
    Rows m(n, FqV(keep));
    for (size_t q = 0; q < n; q++)
      for (size_t i = 0; i < keep; i++) m[q][i] = ld_fq(p + 4 * (q * w + i));
    return m;
  };
  auto fail = [&](int rc, const char* msg) {
    h2d_sync(ctx);
    for (size_t i = 0; i < W->d_block_vars.size(); i++) dev_cache_put(ctx, W->d_block_vars[i], W->d_block_bytes[i]);
    hipFree(W->d_exec);
    delete W;
    return set_err(ctx, rc, msg);
  };
  // block_vars[i] is the witness list of the i-th instance in the prover's sort order (num_proofs descending,
  // ties in block order; lib.rs:1155-1178): the reference pairs block_vars_mat[i] with sorted instance i, so list
  // i holds num_proofs[order[i]] rows of num_vars[order[i]] entries
  std::vector<size_t> order(B);
  for (size_t i = 0; i < B; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return W->nproofs[x] > W->nproofs[y]; });
  for (size_t i = 0; i < B; i++) {
    const size_t b = order[i], n = W->nproofs[b], w = W->nvars[b];
    if (n && !a->block_vars[i]) return fail(SPG_E_ARG, "missing block_vars");
    // the io part of every row (and the memory-op part the w2 recurrences read)
    const size_t keep = std::min(w, io + 2 * W->phy_ops[b] + 4 * W->vir_ops[b]);
    W->block_io.push_back(n ? rows(a->block_vars[i], n, w, keep) : Rows());
    // resident copy, padded to next_pow2(num_proofs) rows of zeros (lib.rs:1209-1216)
    Fq* d = nullptr;
    const size_t rows_p = npow2(std::max<size_t>(n, 1));
    if (!(d = (Fq*)dev_cache_get(ctx, rows_p * w * sizeof(Fq) + 64))) return fail(SPG_E_NOMEM, "block_vars");
    W->d_block_vars.push_back(d);
    W->d_block_bytes.push_back(rows_p * w * sizeof(Fq) + 64);
    // the padding rows zeroed on the context stream, the rows themselves streamed (h2d_stream: page-locked ring, host
    // pool copies, DMA on the upload stream; disjoint bytes, and the context stream waits for the DMAs)
    if (rows_p > n && hipMemsetAsync(d + n * w, 0, (rows_p - n) * w * sizeof(Fq), ctx->stream) != hipSuccess)
      return fail(SPG_E_HIP, "block_vars upload");
    if (n) {
      const int rc = h2d_stream(ctx, d, a->block_vars[i], n * w * sizeof(Fq));
      if (rc) return fail(rc, "block_vars upload");
    }
  }
  const size_t ce = npow2(a->consis_num_proofs);
  W->exec = rows(a->exec_inputs, a->consis_num_proofs, a->num_ios, a->num_ios);
  W->exec.resize(ce, FqV(a->num_ios, fq_zero()));
  {
    FqV f = flatten(W->exec);
    if (hipMalloc(&W->d_exec, f.size() * sizeof(Fq) + 64) != hipSuccess) return fail(SPG_E_NOMEM, "exec inputs");
    if (hipMemcpy(W->d_exec, f.data(), f.size() * sizeof(Fq), hipMemcpyHostToDevice) != hipSuccess)
      return fail(SPG_E_HIP, "exec inputs upload");
  }
  if (a->total_num_init_phy_mem_accesses)
    W->init_phy = rows(a->init_phy_mems, a->total_num_init_phy_mem_accesses, INIT_PHY_MEM_WIDTH, INIT_PHY_MEM_WIDTH);
  if (a->total_num_init_vir_mem_accesses)
    W->init_vir = rows(a->init_vir_mems, a->total_num_init_vir_mem_accesses, INIT_VIR_MEM_WIDTH, INIT_VIR_MEM_WIDTH);
  if (a->total_num_phy_mem_accesses)
    W->addr_phy = rows(a->addr_phy_mems, a->total_num_phy_mem_accesses, PHY_MEM_WIDTH, PHY_MEM_WIDTH);
  if (a->total_num_vir_mem_accesses) {
    W->addr_vir = rows(a->addr_vir_mems, a->total_num_vir_mem_accesses, VIR_MEM_WIDTH, VIR_MEM_WIDTH);
    W->ts_bits = rows(a->addr_ts_bits, a->total_num_vir_mem_accesses, a->mem_addr_ts_bits_size, a->mem_addr_ts_bits_size);
  }
  // (no synchronisation: the streamed DMAs complete on their own, ahead of everything later on the context stream)
  *out = W;
  return SPG_OK;
}
extern "C" int spg_snark_witness_free(spg_ctx* ctx, spg_snark_wit* W) {
  if (!W) return SPG_OK;
  if (ctx) {
    h2d_sync(ctx);  // a streamed upload into it may still be in flight
    for (size_t i = 0; i < W->d_block_vars.size(); i++) dev_cache_put(ctx, W->d_block_vars[i], W->d_block_bytes[i]);
  } else {
    for (auto* d : W->d_block_vars) hipFree(d);
  }
  hipFree(W->d_exec);
  delete W;
  return SPG_OK;
}

namespace {

// rows are independent except their reverse-q recurrences (perm_chain): the per-row work runs on the host pool in
// chunks, the recurrences (2 products per row) afterwards in order
void par_rows(size_t n, const std::function<void(size_t)>& f) {
  const int C = n >= 64 ? 8 : 1;
  pool().parallel_for(C, [&](int c) {
    for (size_t q = n * c / C; q < n * (c + 1) / C; q++) f(q);
  });
}
Rows pad_rows(Rows m, size_t n, size_t w) {
  m.resize(n, FqV(w, fq_zero()));
  return m;
}
FqV column(const Rows& m, size_t c) {
  FqV v;
  for (auto& r : m) v.push_back(r[c]);
  return v;
}

// The reverse-q recurrence of one permutation product chain over the w3 rows (lib.rs:855-864, 1539-1611), from the
// chain's per-row ends:
//   w3[q][col + 1] = ends[q] * (w3[q + 1][col] + 1 - w3[q + 1][0])   (ends[q] itself on the last row)
//   w3[q][col]     = w3[q][0] * w3[q][col + 1]
void perm_chain(Rows& w3, size_t col, const FqV& ends) {
  for (size_t q = w3.size(); q-- > 0;) {
    FqV& w = w3[q];
    w[col + 1] = q + 1 != w3.size() ? fq_mul(ends[q], fq_sub(fq_add(w3[q + 1][col], fq_one()), w3[q + 1][0])) : ends[q];
    w[col] = fq_mul(w[0], w[col + 1]);
  }
}

// What a first-section row (valid, _, inputs, outputs) gives on its own, for perm-exec and block rows alike
// (lib.rs:1322-1366, 1420-1470): w2[0..2], the perm_w0 products w2[3 .. 2 niu), w3[0] = valid and
// w3[1] = valid * (tau - sum_{k >= 3} w2[k] - row[2])
void row_prelude(const FqV& row, const FqV& perm_w0, const Fq& tau, size_t niu, size_t w2_size, FqV* w2_out,
                 FqV* w3_out) {
  FqV w2(w2_size, fq_zero()), w3(W3_WIDTH, fq_zero());
  for (size_t i = 1; i < 2 * (niu - 1); i++) w2[2 + i] = fq_mul(perm_w0[i], row[i + 2]);
  Fq rest = fq_zero();
  for (size_t k = 3; k < w2.size(); k++) rest = fq_add(rest, w2[k]);
  w2[0] = row[0];
  w2[1] = row[0];
  for (size_t i = 0; i + 1 < niu; i++) {
    const Fq perm = i == 0 ? fq_one() : perm_w0[i];
    w2[0] = fq_add(w2[0], fq_mul(perm, row[2 + i]));
    w2[2] = fq_add(w2[2], fq_mul(perm, row[2 + (niu - 1) + i]));
  }
  w2[0] = fq_mul(w2[0], row[0]);
  w2[1] = fq_mul(fq_add(w2[1], w2[2]), row[0]);
  w3[0] = row[0];
  w3[1] = fq_mul(w3[0], fq_sub(fq_sub(tau, rest), row[2]));
  *w2_out = std::move(w2);
  *w3_out = std::move(w3);
}

// SNARK::prove (lib.rs:971-2746) as stages over named state; run() calls them in the reference's section order
struct SnarkProver {
  spg_ctx* ctx;
  spg_snark_comp *block, *pairwise, *perm_root;
  const spg_snark_wit* W;
  spg_r1cs_gens* vars_gens;
  spg_transcript* transcript;
  spg_random_tape* tape_h;
  Tr& t;
  Tape& tape;
  ProverGens& g;
  const spg_snark_inputs& a;
  const size_t niu, num_ios;
  const SnarkShape sh;
  Laps lp;
  CQ cq;
  Writer w;  // bincode(SNARK) in declaration order (lib.rs:701-756)

  Fq tau, r;
  FqV perm_w0;
  HostSec w0;                    // perm_w0 as the one-row section every instance shares
  PermWit pe, bw, mem[4];        // perm-exec, the blocks, SNARK::mem_gen of init phy / init vir / phy / vir
  HostSec iphy, ivir, aphy, aphys, avir, avirs, ts;  // the memory lists as given (padded), addr lists also shifted
  std::vector<std::vector<Pt>> c_bv;  // block_vars and exec inputs: committed from HBM
  std::vector<Pt> c_exec;
  SecInfo s_bvars, s_exec;
  spg_r1cs_witness* Wt;  // the context's cached R1CS witness, refilled in place by every sat_prove
  SatOut so;

  SnarkProver(spg_ctx* c, spg_snark_comp* b, spg_snark_comp* pw, spg_snark_comp* pr, const spg_snark_wit* wit,
              spg_r1cs_gens* vg, spg_transcript* tr, spg_random_tape* tp)
      : ctx(c), block(b), pairwise(pw), perm_root(pr), W(wit), vars_gens(vg), transcript(tr), tape_h(tp), t(tr->t),
        tape(tp->t), g(vg->g), a(wit->a), niu(a.num_inputs_unpadded), num_ios(a.num_ios),
        sh(a, wit->nproofs.data(), wit->nvars.data(), wit->phy_ops.data(), wit->vir_ops.data()), bw(sh.P),
        c_bv(sh.P), Wt(c->wt_cache) {
    lp.title = "SNARK::prove";
    ctx->wt_cache = nullptr;
  }
  ~SnarkProver() {  // the witness goes back to the context on every exit path
    if (!ctx->wt_cache) ctx->wt_cache = Wt;
    else spg_r1cs_witness_free(ctx, Wt);
  }

  void fp(const char* where) {  // SPG_DEBUG_SNARK: a fingerprint of the transcript's state
    if (!knob::debug_snark() || t.cb) return;  // (a fork of a caller-backed transcript cannot be taken)
    Tr c = t;
    Fq x = c.challenge("dbg");
    fprintf(stderr, "fp %s %08x\n", where, x.l[0]);
  }

  int run();
  int append_instance();
  int launch_early_commits();
  void draw_challenges();
  void gen_perm_exec();
  void gen_block();
  void gen_mem(size_t width, const Rows& mems, bool vir, PermWit* o);
  int queue_input_commits();
  void write_commitments();
  int sat_then_evals(spg_snark_comp* C, const std::vector<size_t>& order, bool as_list);
  // one of the three R1CSProofs as R1CSProof::prove takes it: the instance, the sizes, the witness sections, and for
  // every (sorted / merged) instance the component it came from (spg_snark_report.component)
  struct SatCall {
    const char* stage;
    spg_r1cs_inst* inst;
    size_t P, max_np, max_ni;
    std::vector<size_t> num_proofs, num_inputs, from;
    std::vector<WPart> parts;
  };
  int block_call(SatCall* c);
  int pairwise_call(SatCall* c);
  int perm_root_call(SatCall* c);
  int sat_stage(const SatCall& c);
  // the product entry of every w3 polynomial in PERM_PRODUCT's merged order, and the component of each
  int perm_prod_list(SecInfo* pw3, std::vector<size_t>* im, FqV* prod, std::vector<FqV>* r_list);
  int check(spg_snark_report* out);
  int prove_block();
  int prove_pairwise();
  int prove_perm_root();
  int prove_perm_product();
  int prove_shift();
  int prove_io();
  int finish(uint8_t* proof, size_t proof_cap, size_t* proof_len);
};

int SnarkProver::run() {
  int rc;
  t.protocol("Spartan SNARK proof");
  if ((rc = append_instance())) return rc;
  lp.lap("inst_commit+sort");
  if ((rc = launch_early_commits())) return rc;
  draw_challenges();
  gen_perm_exec();
  gen_block();
  gen_mem(INIT_PHY_MEM_WIDTH, iphy.rows[0], false, &mem[0]);
  gen_mem(INIT_VIR_MEM_WIDTH, ivir.rows[0], false, &mem[1]);
  gen_mem(PHY_MEM_WIDTH, aphy.rows[0], false, &mem[2]);
  gen_mem(VIR_MEM_WIDTH, avir.rows[0], true, &mem[3]);
  lp.lap("mem_gen");
  if ((rc = queue_input_commits())) return rc;
  lp.lap("input_commit");
  write_commitments();
  if ((rc = prove_block())) return rc;
  lp.lap("block_eval");
  if ((rc = prove_pairwise())) return rc;
  lp.lap("pairwise");
  if ((rc = prove_perm_root())) return rc;
  lp.lap("perm_root");
  if ((rc = prove_perm_product())) return rc;
  lp.lap("perm_product");
  if ((rc = prove_shift())) return rc;
  lp.lap("shift");
  if ((rc = prove_io())) return rc;
  lp.lap("io");
  return 0;
}

// INSTANCE COMMITMENTS (lib.rs:1086-1153), then the block and pairwise sort and the padded memory lists
// (lib.rs:1155-1296; the sizes are SnarkShape's)
int SnarkProver::append_instance() {
  append_snark_params(t, a, W->nproofs.data(), W->nvars.data(), W->phy_ops.data(), W->vir_ops.data());
  fp("params");
  append_comm_map(t, block->label_map);
  fp("map");
  for (size_t gi = 0; gi < block->sparks.size(); gi++) append_r1cs_comm(block, gi, t);
  fp("block");
  append_r1cs_comm(pairwise, 0, t);
  fp("pairwise");
  append_r1cs_comm(perm_root, 0, t);
  fp("perm_root");
  append_snark_io(t, a, W->input, W->output);
  iphy.rows[0] = pad_rows(W->init_phy, sh.t_iphy, INIT_PHY_MEM_WIDTH);
  ivir.rows[0] = pad_rows(W->init_vir, sh.t_ivir, INIT_VIR_MEM_WIDTH);
  aphy.rows[0] = pad_rows(W->addr_phy, sh.t_phy, PHY_MEM_WIDTH);
  avir.rows[0] = pad_rows(W->addr_vir, sh.t_vir, VIR_MEM_WIDTH);
  ts.rows[0] = pad_rows(W->ts_bits, sh.t_vir, a.mem_addr_ts_bits_size);
  // block_vars_mat[i] pairs with sorted instance i (the reference never permutes the witness list)
  int rc = ensure_sorted(ctx, block, sh.order);
  if (rc) return rc;
  return ensure_sorted(ctx, pairwise, sh.pw_order);
}

// block_vars commitments: on the device now, read back when the queue is flushed
int SnarkProver::launch_early_commits() {
  std::vector<std::pair<const Fq*, size_t>> bv;
  for (size_t p = 0; p < sh.P; p++) bv.push_back({W->d_block_vars[p], sh.bnp_pad[p] * sh.bnv[p]});
  return cq.launch_early(ctx, g, bv);
}

void SnarkProver::draw_challenges() {
  tau = t.challenge("challenge_tau");
  r = t.challenge("challenge_r");
  if (knob::debug_tr()) fprintf(stderr, "[prove] tau %08x r %08x\n", tau.l[0], r.l[0]);
  if (knob::debug_snark()) fprintf(stderr, "snark tau %08x %08x r %08x\n", tau.l[0], tau.l[1], r.l[0]);
  perm_w0 = spg::perm_w0(tau, r, niu, num_ios);
  w0.rows[0] = {perm_w0};
  w0.queue(cq);
}

// WITNESS GEN, perm-exec (lib.rs:1299-1418)
void SnarkProver::gen_perm_exec() {
  Rows w2(sh.consis), w3(sh.consis);
  par_rows(sh.consis, [&](size_t q) {
    row_prelude(W->exec[q], perm_w0, tau, niu, num_ios, &w2[q], &w3[q]);
    w3[q][4] = w2[q][0];
    w3[q][5] = w2[q][1];
  });
  perm_chain(w3, 2, column(w3, 1));
  if (knob::debug_snark())
    for (size_t q = 0; q < 2; q++)
      for (size_t i = 0; i < num_ios; i++) fprintf(stderr, "pe_w2[%zu][%zu] %08x\n", q, i, w2[q][i].l[0]);
  pe.set(0, std::move(w2), std::move(w3));
  lp.lap("perm_exec_witness");
  pe.queue(cq);
  lp.lap("perm_exec_commit");
}

// WITNESS GEN, blocks (lib.rs:1420-1741): after the row prelude, the physical (addr, data) and virtual
// (addr, data, ls, ts) memory operations of the row, each a product chain along the row whose end feeds a reverse-q
// chain of w3 (columns 4-5 physical, 6-7 virtual)
void SnarkProver::gen_block() {
  const Fq r2 = fq_mul(r, r), r3 = fq_mul(r2, r);
  const size_t io_width = 2 * niu;
  for (size_t p = 0; p < sh.P; p++) {
    const size_t np_ = sh.bphy[p], nv_ = sh.bvir[p], Q = sh.bnp_pad[p], w2_size = sh.w2_size(p);
    const Rows& bio = W->block_io[p];
    const FqV zero_row(bio.empty() ? 0 : bio[0].size(), fq_zero());
    Rows w2(Q), w3(Q);
    FqV pxs(Q), vxs(Q);  // the ends of the row's memory chains
    par_rows(Q, [&](size_t q) {  // everything of row q that does not depend on row q + 1
      const FqV& bv = q < bio.size() ? bio[q] : zero_row;
      FqV& x = w2[q];
      row_prelude(bv, perm_w0, tau, niu, w2_size, &x, &w3[q]);
      const Fq valid = bv[0];
      for (size_t i = 0; i < np_; i++) {
        const size_t PMR = io_width + 2 * i, PMC = PMR + 1;
        x[PMR] = fq_mul(r, bv[PMR + 1]);
        const Fq tt = i == 0 ? valid : x[PMC - 2];
        x[PMC] = fq_mul(tt, fq_sub(fq_sub(tau, bv[PMR]), x[PMR]));
      }
      pxs[q] = np_ == 0 ? valid : x[io_width + 2 * (np_ - 1) + 1];
      for (size_t i = 0; i < nv_; i++) {
        const size_t base = io_width + 2 * np_ + 4 * i;
        x[base] = fq_mul(r, bv[base + 1]);
        x[base + 1] = fq_mul(r2, bv[base + 2]);
        x[base + 2] = fq_mul(r3, bv[base + 3]);
        const Fq tt = i == 0 ? valid : x[base - 1];
        x[base + 3] = fq_mul(tt, fq_sub(fq_sub(fq_sub(fq_sub(tau, bv[base]), x[base]), x[base + 1]), x[base + 2]));
      }
      vxs[q] = nv_ == 0 ? valid : x[io_width + 2 * np_ + 4 * (nv_ - 1) + 3];
    });
    perm_chain(w3, 2, column(w3, 1));
    perm_chain(w3, 4, pxs);
    perm_chain(w3, 6, vxs);
    bw.set(p, std::move(w2), std::move(w3));
  }
  lp.lap("block_witness");
  for (size_t p = 0; p < sh.P; p++) bw.w2.queue(cq, p);
  for (size_t p = 0; p < sh.P; p++) {
    bw.w3.queue(cq, p);
    bw.w3s.queue(cq, p);
  }
  lp.lap("block_w_commit");
}

// SNARK::mem_gen (lib.rs:831-968) of one padded memory list (nothing for a list the program does not use)
void SnarkProver::gen_mem(size_t width, const Rows& mems, bool vir, PermWit* o) {
  const size_t total = mems.size();
  if (total == 0) return;
  Rows w2(total, FqV(width, fq_zero())), w3(total, FqV(W3_WIDTH, fq_zero()));
  const Fq r2 = fq_mul(r, r), r3 = fq_mul(r2, r);
  for (size_t q = 0; q < total; q++) {
    const FqV& m = mems[q];
    Fq rest = w2[q][3] = fq_mul(r, m[3]);
    if (vir) {
      w2[q][4] = fq_mul(r2, m[4]);
      w2[q][5] = fq_mul(r3, m[5]);
      rest = fq_add(fq_add(rest, w2[q][4]), w2[q][5]);
    }
    w3[q][0] = m[0];
    w3[q][1] = fq_mul(m[0], fq_sub(fq_sub(tau, m[2]), rest));
    w3[q][4] = fq_mul(m[0], fq_add(fq_add(m[0], m[2]), rest));
    w3[q][5] = m[0];
  }
  perm_chain(w3, 2, column(w3, 1));
  o->set(0, std::move(w2), std::move(w3));
  o->queue(cq);
}

// WITNESS COMMITMENTS (lib.rs:1957-2221): block_vars and exec inputs from HBM, the memory lists, then every queued
// commitment computed and appended to the transcript in the order it was queued
int SnarkProver::queue_input_commits() {
  for (size_t p = 0; p < sh.P; p++) {
    cq.add_dev(W->d_block_vars[p], sh.bnp_pad[p] * sh.bnv[p], &c_bv[p]);
    s_bvars.push(sh.bnp_pad[p], sh.bnv[p], W->d_block_vars[p], nullptr);
  }
  cq.add_dev(W->d_exec, sh.consis * num_ios, &c_exec);
  s_exec.push(sh.consis, num_ios, W->d_exec, nullptr);
  if (sh.t_iphy) iphy.queue(cq);
  if (sh.t_ivir) ivir.queue(cq);
  if (sh.t_phy) {
    aphy.queue(cq);
    aphys.rows[0] = shift_rows(aphy.rows[0], PHY_MEM_WIDTH);
    aphys.queue(cq);
  }
  if (sh.t_vir) {
    avir.queue(cq);
    avirs.rows[0] = shift_rows(avir.rows[0], VIR_MEM_WIDTH);
    avirs.queue(cq);
    ts.queue(cq);
  }
  return cq.flush(ctx, g, t);
}

// the commitments of bincode(SNARK), ahead of the proofs
void SnarkProver::write_commitments() {
  w.u64(sh.P);
  for (auto& c : c_bv) w.pts(c);
  w.u64(1);
  w.pts(c_exec);
  for (HostSec* s : {&aphy, &aphys, &avir, &avirs, &ts}) w.pts(s->comm[0]);
  for (HostSec* s : {&pe.w2, &pe.w3, &pe.w3s}) w.pts(s->comm[0]);
  for (HostSec* s : {&bw.w2, &bw.w3, &bw.w3s}) {
    w.u64(sh.P);
    for (auto& c : s->comm) w.pts(c);
  }
  for (PermWit& m : mem)
    for (HostSec* s : {&m.w2, &m.w3, &m.w3s}) w.pts(s->comm[0]);
}

// After an R1CSProof over the instances of C: its bytes, R1CSInstance::multi_evaluate at (rx, ry) with the rp-bound
// evaluations in the sorted `order`, the claims into the transcript, then a counted list of one R1CSEvalProof per
// commitment (as_list: the multi-commitment block instance) or the one proof over all evaluations
int SnarkProver::sat_then_evals(spg_snark_comp* C, const std::vector<size_t>& order, bool as_list) {
  w.out.insert(w.out.end(), so.bytes.begin(), so.bytes.end());
  FqV list;
  Fq brp[3];
  int rc = multi_eval(ctx, C, so.ch[2], so.ch[3], &list);
  if (rc) return rc;
  bound_rp(list, order, so.ch[0], brp);
  for (auto& e : list) t.scalar("ABCr_claim", e);
  t.challenge("challenge_c0");
  t.challenge("challenge_c1");
  t.challenge("challenge_c2");
  for (int k = 0; k < 3; k++) w.fq(brp[k]);
  w.fqs(list);
  if (!as_list) return spark_prove_core(ctx, C->sparks[0], so.ch[2], so.ch[3], list, t, tape, w);
  w.u64(C->sparks.size());
  for (size_t gi = 0; gi < C->sparks.size(); gi++) {
    FqV ev;
    for (auto l : C->label_map[gi]) ev.push_back(list[l]);
    if ((rc = spark_prove_core(ctx, C->sparks[gi], so.ch[2], so.ch[3], ev, t, tape, w))) return rc;
  }
  return 0;
}

// R1CSProof::prove of one stage; in check mode (spg_set_check_sat) the prover's message names the stage, and for
// the blocks the caller's block number
int SnarkProver::sat_stage(const SatCall& c) {
  struct Scope {
    spg_ctx* x;
    ~Scope() { x->sat_stage = nullptr, x->sat_order = nullptr; }
  } scope{ctx};
  ctx->sat_stage = c.stage;
  ctx->sat_order = c.inst == block->dev_sorted ? c.from.data() : nullptr;
  return sat_prove(ctx, vars_gens, c.inst, c.P, c.max_np, c.num_proofs, c.max_ni, c.num_inputs, c.parts, &Wt,
                   transcript, tape_h, &so);
}

// BLOCK_CORRECTNESS_EXTRACT (lib.rs:2223-2309)
int SnarkProver::block_call(SatCall* c) {
  *c = SatCall{"block", block->dev_sorted, sh.P, sh.bmax, a.num_vars, sh.bnp_pad, sh.bnv, sh.order,
               {wpart(s_bvars), wpart(w0.s), wpart(bw.w2.s), wpart(bw.w3.s), wpart(bw.w3s.s)}};
  return 0;
}
int SnarkProver::prove_block() {
  SatCall c;
  int rc = block_call(&c);
  if (!rc) rc = sat_stage(c);
  if (rc) return rc;
  lp.lap("block_sat");
  return sat_then_evals(block, sh.order, true);
}

// PAIRWISE_CHECK (lib.rs:2311-2424)
int SnarkProver::pairwise_call(SatCall* c) {
  SecInfo pw, pws;
  std::vector<size_t> im;
  int rc;
  if ((rc = merge(ctx, {&pe.w3.s, &aphy.s, &avir.s}, &pw, &im))) return rc;
  if ((rc = merge(ctx, {&pe.w3s.s, &aphys.s, &avirs.s}, &pws))) return rc;
  std::vector<const SecInfo*> comps(im.size(), &w0.s);
  for (size_t i = 0; i < im.size(); i++)
    if (im[i] == 2) comps[i] = &ts.s;
  const SecInfo tsb = concat(comps);
  const size_t n = pw.num_proofs.size();
  *c = SatCall{"pairwise", pairwise->dev_sorted, n, sh.pairwise_size, sh.pw_nv, pw.num_proofs,
               std::vector<size_t>(n, sh.pw_nv), im, {wpart(pw), wpart(pws), wpart(tsb)}};
  return 0;
}
int SnarkProver::prove_pairwise() {
  SatCall c;
  int rc = pairwise_call(&c);
  if (!rc) rc = sat_stage(c);
  if (rc) return rc;
  return sat_then_evals(pairwise, sh.pw_order, false);
}

// PERM_ROOT (lib.rs:2426-2532)
int SnarkProver::perm_root_call(SatCall* c) {
  SecInfo w1, w2s, w3s, w4;
  std::vector<size_t> im;
  int rc;
  if ((rc = merge(ctx, {&s_exec, &iphy.s, &ivir.s, &aphy.s, &avir.s}, &w1, &im))) return rc;
  if ((rc = merge(ctx, {&pe.w2.s, &mem[0].w2.s, &mem[1].w2.s, &mem[2].w2.s, &mem[3].w2.s}, &w2s))) return rc;
  if ((rc = merge(ctx, {&pe.w3.s, &mem[0].w3.s, &mem[1].w3.s, &mem[2].w3.s, &mem[3].w3.s}, &w3s))) return rc;
  if ((rc = merge(ctx, {&pe.w3s.s, &mem[0].w3s.s, &mem[1].w3s.s, &mem[2].w3s.s, &mem[3].w3s.s}, &w4))) return rc;
  const size_t n = w1.num_proofs.size();
  *c = SatCall{"perm_root", perm_root->dev, n, sh.perm_size, num_ios, w1.num_proofs, std::vector<size_t>(n, num_ios), im,
               {wpart(w0.s), wpart(w1), wpart(w2s), wpart(w3s), wpart(w4)}};
  return 0;
}
int SnarkProver::prove_perm_root() {
  SatCall c;
  int rc = perm_root_call(&c);
  if (!rc) rc = sat_stage(c);
  if (rc) return rc;
  w.out.insert(w.out.end(), so.bytes.begin(), so.bytes.end());
  FqV e;
  if ((rc = multi_eval(ctx, perm_root, so.ch[2], so.ch[3], &e))) return rc;
  t.scalar("Ar_claim", e[0]);
  t.scalar("Br_claim", e[1]);
  t.scalar("Cr_claim", e[2]);
  for (int k = 0; k < 3; k++) w.fq(e[k]);
  return spark_prove_core(ctx, perm_root->sparks[0], so.ch[2], so.ch[3], FqV(e.begin(), e.begin() + 3), t, tape, w);
}

// PERM_PRODUCT_PROOF (lib.rs:2534-2609): every w3 polynomial's product entry opened in one batched proof; the block
// w3 polynomials appear once per chain they carry (exec, then physical, then virtual memory)
int SnarkProver::perm_prod_list(SecInfo* pw3_out, std::vector<size_t>* im_out, FqV* prod_out,
                                std::vector<FqV>* r_list_out) {
  std::vector<const SecInfo*> comps = {&pe.w3.s, &mem[0].w3.s, &mem[1].w3.s, &mem[2].w3.s, &mem[3].w3.s, &bw.w3.s};
  if (a.max_block_num_phy_ops > 0) comps.push_back(&bw.w3.s);
  if (a.max_block_num_vir_ops > 0) comps.push_back(&bw.w3.s);
  std::vector<size_t> im;
  SecInfo pw3;
  int rc = merge(ctx, comps, &pw3, &im);
  if (rc) return rc;
  const size_t pm_bl_id = 6, vm_bl_id = a.max_block_num_phy_ops > 0 ? 7 : 6;
  FqV prod;
  std::vector<FqV> r_list;
  for (size_t i = 0; i < im.size(); i++) {
    const FqV& p = *pw3.poly[i];
    if (im[i] == vm_bl_id) {
      prod.push_back(p[6]);
      r_list.push_back({fq_one(), fq_one(), fq_zero()});
    } else if (im[i] == pm_bl_id) {
      prod.push_back(p[4]);
      r_list.push_back({fq_one(), fq_zero(), fq_zero()});
    } else {
      prod.push_back(p[2]);
      r_list.push_back({fq_one(), fq_zero()});
    }
  }
  *pw3_out = std::move(pw3);
  *im_out = std::move(im);
  *prod_out = std::move(prod);
  *r_list_out = std::move(r_list);
  return 0;
}
int SnarkProver::prove_perm_product() {
  SecInfo pw3;
  std::vector<size_t> im;
  FqV prod;
  std::vector<FqV> r_list;
  int rc = perm_prod_list(&pw3, &im, &prod, &r_list);
  if (rc) return rc;
  w.fqs(prod);
  return prove_batched_instances(ctx, g, pw3.poly, r_list, prod, t, tape, w);
}

// spg_snark_check: SNARK::prove's witness generation (through the input commitments, which fix tau and r as a prove
// would draw them), then everything a verifier would reject a bad witness for, evaluated without proving: the three
// R1CS instances' satisfiability (R1CSInstance::is_sat, src/r1csinstance.rs:322-357, on the device), the permutation
// products SNARK::verify multiplies (verify.hip check_perm_product), and the IO proof's opened points. All checks
// run; the report's `first` is the earliest failure in the verifier's order.
int SnarkProver::check(spg_snark_report* out) {
  memset(out, 0, sizeof(*out));
  out->io_point = -1;
  out->first = -1;
  int rc;
  t.protocol("Spartan SNARK proof");
  if ((rc = append_instance())) return rc;
  if ((rc = launch_early_commits())) return rc;
  draw_challenges();
  gen_perm_exec();
  gen_block();
  gen_mem(INIT_PHY_MEM_WIDTH, iphy.rows[0], false, &mem[0]);
  gen_mem(INIT_VIR_MEM_WIDTH, ivir.rows[0], false, &mem[1]);
  gen_mem(PHY_MEM_WIDTH, aphy.rows[0], false, &mem[2]);
  gen_mem(VIR_MEM_WIDTH, avir.rows[0], true, &mem[3]);
  if ((rc = queue_input_commits())) return rc;
  std::string first_msg;
  auto failed = [&](int code, const std::string& msg) {
    if (out->first < 0) out->first = code, first_msg = msg;
  };
  int (SnarkProver::*const calls[3])(SatCall*) = {&SnarkProver::block_call, &SnarkProver::pairwise_call,
                                                  &SnarkProver::perm_root_call};
  for (int k = 0; k < 3; k++) {
    SatCall c;
    if ((rc = (this->*calls[k])(&c))) return rc;
    if ((rc = witness_from_parts(ctx, c.parts, &Wt))) return rc;
    spg_sat_report& r = out->sat[k];
    if ((rc = spg_r1cs_sat_check(ctx, c.inst, c.P, c.max_np, c.num_proofs.data(), c.max_ni, c.num_inputs.data(), Wt, &r)))
      return rc;
    if (!r.violations) continue;
    out->component[k] = r.p < c.from.size() ? c.from[r.p] : 0;
    failed(k, std::string(c.stage) + ": " + sat_message(r) + (k == 0 ? "; block " + std::to_string(out->component[k]) : ""));
  }
  {
    SecInfo pw3;
    std::vector<size_t> im;
    FqV prod;
    std::vector<FqV> r_list;
    if ((rc = perm_prod_list(&pw3, &im, &prod, &r_list))) return rc;
    // the products of check_perm_product (verify.hip): exec against blocks, each memory's ops against its list
    Fq pe_ = fq_one(), pb = fq_one(), pmb = fq_one(), pma = fq_one(), vmb = fq_one(), vma = fq_one();
    for (size_t i = 0; i < im.size(); i++) {
      const Fq& x = prod[i];
      switch (im[i]) {
        case 0: pe_ = fq_mul(pe_, x); break;
        case 1: pmb = fq_mul(pmb, x); break;
        case 2: vmb = fq_mul(vmb, x); break;
        case 3: pma = fq_mul(pma, x); break;
        case 4: vma = fq_mul(vma, x); break;
        case 5: pb = fq_mul(pb, x); break;
        case 6:
          if (a.max_block_num_phy_ops > 0) pmb = fq_mul(pmb, x);
          else vmb = fq_mul(vmb, x);
          break;
        case 7: vmb = fq_mul(vmb, x); break;
      }
    }
    static const char* const what[3] = {"execution / block permutation products", "physical memory permutation products",
                                        "virtual memory permutation products"};
    const bool differ[3] = {!fq_eq(pe_, pb), !fq_eq(pmb, pma), !fq_eq(vmb, vma)};
    for (int k = 0; k < 3; k++) {
      out->perm_products[k] = differ[k] ? 1 : 0;
      if (differ[k]) failed(3 + k, what[k]);
    }
  }
  {
    const IoPoints io = io_points(a, sh.consis, W->liveness.data(), W->liveness.size(), W->input, W->output);
    const FqV flat = pad_pow2(flatten(W->exec));
    for (size_t k = 0; k < io.idx.size() && out->io_point < 0; k++)
      if (io.idx[k] >= flat.size() || !fq_eq(flat[io.idx[k]], io.Zr[k])) out->io_point = (int64_t)k;
    if (out->io_point >= 0) failed(6, "IO proof: opened point " + std::to_string(out->io_point) + " differs from its public value");
  }
  if (out->first >= 0) set_err(ctx, SPG_E_VERIFY, first_msg);
  return 0;
}

// SHIFT_PROOFS (lib.rs:2611-2668)
int SnarkProver::prove_shift() {
  std::vector<const FqV*> orig, shifted;
  std::vector<size_t> hl;
  for (const ShiftPair& sp : shift_pairs(sh)) {
    const HostSec *o = nullptr, *s = nullptr;
    switch (sp.kind) {
      case ShiftPair::kPermExecW3: o = &pe.w3, s = &pe.w3s; break;
      case ShiftPair::kBlockW3: o = &bw.w3, s = &bw.w3s; break;
      case ShiftPair::kMemW3: o = &mem[sp.idx].w3, s = &mem[sp.idx].w3s; break;
      case ShiftPair::kAddrPhy: o = &aphy, s = &aphys; break;
      case ShiftPair::kAddrVir: o = &avir, s = &avirs; break;
    }
    const size_t p = sp.kind == ShiftPair::kBlockW3 ? sp.idx : 0;
    orig.push_back(&o->poly[p]);
    shifted.push_back(&s->poly[p]);
    hl.push_back(sp.header);
  }
  const size_t n = orig.size();
  std::vector<std::vector<Pt>> openings(n);
  {
    std::vector<CJob> jobs;
    for (size_t p = 0; p < n; p++)
      for (size_t i = 0; i < hl[p]; i++) jobs.push_back(CJob(g.gens_1, {(*orig[p])[i]}, fq_zero()));
    std::vector<Pt> pts = commit_batch(g, jobs);
    size_t k = 0;
    for (size_t p = 0; p < n; p++)
      for (size_t i = 0; i < hl[p]; i++) {
        t.point("shift_header_entry", pts[k]);
        openings[p].push_back(pts[k++]);
      }
  }
  const Fq c = t.challenge("challenge_c");
  // the evaluations sum_k poly[k] c^k (lib.rs:2640-2655) from the uni-batched proof's L.Z bounds, computed once
  // over the pool: sum_k LZ[k] c^k, LZ[k] = sum_j c^(Rs j) poly[j Rs + k]
  std::vector<const FqV*> all(orig);
  all.insert(all.end(), shifted.begin(), shifted.end());
  const std::vector<FqV> LZs = uni_bounds(all, c);
  size_t rs_max = 0;
  for (auto& v : LZs) rs_max = std::max(rs_max, v.size());
  const FqV c_pow = pe_powers(c, rs_max);
  FqV ev(2 * n);
  for (size_t p = 0; p < 2 * n; p++) {
    Fq x = fq_zero();
    for (size_t k = 0; k < LZs[p].size(); k++) x = fq_add(x, fq_mul(LZs[p][k], c_pow[k]));
    ev[p] = x;
  }
  std::vector<CJob> jobs;
  for (auto& x : ev) jobs.push_back(CJob(g.gens_1, {x}, fq_zero()));
  std::vector<Pt> ce = commit_batch(g, jobs);
  int rc = prove_uni_batched(ctx, g, all, LZs, c, ev, t, tape, w);
  if (rc) return rc;
  w.pts(std::vector<Pt>(ce.begin(), ce.begin() + n));
  w.pts(std::vector<Pt>(ce.begin() + n, ce.end()));
  w.u64(n);
  for (auto& o : openings) w.pts(o);
  return 0;
}

// IO_PROOFS (lib.rs:194-272)
int SnarkProver::prove_io() {
  const IoPoints io = io_points(a, sh.consis, W->liveness.data(), W->liveness.size(), W->input, W->output);
  return prove_batched_points(ctx, g, pad_pow2(flatten(W->exec)), io.r_list(), io.Zr, t, tape, w);
}

// the trace lines of the whole prove, then the proof into the caller's buffer
int SnarkProver::finish(uint8_t* proof, size_t proof_cap, size_t* proof_len) {
  lp.print();
  if (knob::trace() >= 2) {
    fprintf(stderr, "[spg] sigma-protocol commitments: %zu calls, %zu commitments, %.0f us on the host\n",
                    g_commit_stats.calls, g_commit_stats.points, g_commit_stats.us);
    g_commit_stats = CommitStats();
    static uint64_t bursts0 = 0, keccak0 = 0;
    fprintf(stderr, "[spg] host pool bursts: %llu, keccak-f permutations on this thread: %llu\n",
            (unsigned long long)(pool().bursts() - bursts0), (unsigned long long)(keccak_count() - keccak0));
    bursts0 = pool().bursts();
    keccak0 = keccak_count();
  }
  if (knob::copy_trace()) print_copy_counts();
  *proof_len = w.out.size();
  if (!proof || w.out.size() > proof_cap) return set_err(ctx, SPG_E_ARG, "proof buffer too small");
  memcpy(proof, w.out.data(), w.out.size());
  return SPG_OK;
}

}  // namespace

static int snark_witness_args(spg_ctx* ctx, spg_snark_comp* block, const spg_snark_wit* W);

extern "C" int spg_snark_check(spg_ctx* ctx, spg_snark_comp* block, spg_snark_comp* pairwise, spg_snark_comp* perm_root,
                               const spg_snark_wit* W, spg_r1cs_gens* vars_gens, spg_transcript* transcript,
                               spg_snark_report* out) {
  if (!ctx || !block || !pairwise || !perm_root || !W || !vars_gens || !transcript || !out) return SPG_E_ARG;
  if (ctx->nranks > 1) return spg::set_err(ctx, SPG_E_ARG, "spg_snark_check: single-rank, as spg_snark_prove");
  if (int rc = snark_witness_args(ctx, block, W)) return rc;
  spg::HostPin pin;
  spg_random_tape tape("snark_check", spg::fq_zero());  // no blind is drawn before the proofs begin
  SnarkProver pr(ctx, block, pairwise, perm_root, W, vars_gens, transcript, &tape);
  return spg::tr_status(ctx, transcript->t, pr.check(out));
}

static int spg_snark_prove_impl(spg_ctx* ctx, spg_snark_comp* block, spg_snark_comp* pairwise, spg_snark_comp* perm_root,
                               const spg_snark_wit* W, spg_r1cs_gens* vars_gens, spg_transcript* transcript,
                               spg_random_tape* tape_h, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
  if (!ctx || !block || !pairwise || !perm_root || !W || !vars_gens || !transcript || !tape_h || !proof_len)
    return SPG_E_ARG;
  if (int rc = snark_witness_args(ctx, block, W)) return rc;
  SnarkProver pr(ctx, block, pairwise, perm_root, W, vars_gens, transcript, tape_h);
  const int rc = pr.run();
  if (rc == SPG_E_UNSAT) *proof_len = 0;  // check mode: no proof was written
  return rc ? rc : pr.finish(proof, proof_cap, proof_len);
}

// the argument checks of spg_snark_prove and spg_snark_check, before any launch
static int snark_witness_args(spg_ctx* ctx, spg_snark_comp* block, const spg_snark_wit* W) {
  if (2 * W->a.num_inputs_unpadded > W->a.num_ios) return set_err(ctx, SPG_E_ARG, "num_ios < 2 * num_inputs_unpadded");
  {  // before any launch: a block whose rows or matrices reach beyond its witness width (snark_shape.hpp)
    const size_t Bb = W->a.block_num_instances_bound;
    if (block->num_instances != Bb || block->mats.size() != 3 * Bb || !W->a.num_vars)
      return set_err(ctx, SPG_E_ARG, "block instance and witness disagree on the number of blocks");
    if (block->cols_needed_stride != W->a.num_vars) {  // the matrices are read once per encoded instance
      std::vector<const spg_sparse_entry*> ent;
      for (auto& m : block->mats) ent.push_back(m.data());
      block->cols_needed = block_cols_needed(Bb, W->a.num_vars, ent.data(), block->nnz.data());
      block->cols_needed_stride = W->a.num_vars;
    }
    if (block_width_violation(Bb, W->nproofs.data(), W->nvars.data(), W->phy_ops.data(), W->vir_ops.data(),
                              W->a.num_inputs_unpadded, W->a.num_vars, block->cols_needed.data()) >= 0)
      return set_err(ctx, SPG_E_ARG, "a block names a column beyond its block_num_vars");
  }
  return SPG_OK;
}

extern "C" int spg_snark_prove(spg_ctx* ctx, spg_snark_comp* block, spg_snark_comp* pairwise, spg_snark_comp* perm_root,
                               const spg_snark_wit* W, spg_r1cs_gens* vars_gens, spg_transcript* transcript,
                               spg_random_tape* tape_h, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
  if (!ctx || !transcript) return SPG_E_ARG;
  // SPG_TRACE: the whole call's wall time (the laps end at the io proofs; this adds the proof copy-out and the
  // release of the prove's host state)
  const bool tr = knob::trace_is_set();
  const auto t0 = std::chrono::steady_clock::now();
  int rc;
  {
    spg::HostPin pin;
    rc = spg::tr_status(ctx, transcript->t, spg_snark_prove_impl(ctx, block, pairwise, perm_root, W, vars_gens, transcript, tape_h, proof, proof_cap, proof_len));
  }
  if (tr)
    fprintf(stderr, "[spg] spg_snark_prove call: %.0f us\n",
            std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  return rc;
}
