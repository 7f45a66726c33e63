// spg — SPARK: commitments to and evaluation proofs of batched sparse matrix polynomials on MI355X.
//
//   SparseMatPolynomial::multi_commit            src/sparse_mlpoly.rs:368-425, 566-587  spg_spark_commit
//   SparseMatPolyEvalProof::prove                src/sparse_mlpoly.rs:1497-1564         spg_spark_prove
//     AddrTimestamps::deref, Derefs::commit      :255-270, :51-67                        k_gather, Hyrax rows (hyrax.hip)
//     Layers::build_hash_layer, ProductCircuit   :612-736, src/product_tree.rs:36-58    k_hash_*, tree_build (layers.hip)
//     ProductLayerProof::prove                   :1118-1263                              batched_prove (layers.hip)
//     HashLayerProof::prove                      :805-918                                k_seg_dot, poly_eval_prove (hyrax.hip)
// The sizes both derive from the batch and the generators: spark_shape.hpp.
//
// HBM layout (B = 3 x instances matrices, N = next_pow2(max nnz), cells = 2^max(nvx, nvy)):
//   addr / read_ts : u32 [2][B][N] (rows, then cols)    audit : u32 [2][cells]
//   val            : Fq [B][N]
//   comb_ops (Fq)  : [row addr | row read_ts | col addr | col read_ts | val] (each B x N), zero-padded to 2^k
//   comb_mem (Fq)  : [row audit | col audit]
//   product trees  : circuit c at c * 2M, its M hashed leaves first (the levels' layout: layers.hip)
// All O(N) work stays in HBM; the host runs the transcript and one UniPoly per sumcheck round.
#include <algorithm>
#include <memory>

#include <hipcub/hipcub.hpp>

#include "hostpoly.hpp"
#include "knobs.hpp"
#include "prodc.hpp"
#include "proto.hpp"
#include "segsum.hpp"
#include "spark_shape.hpp"
#include "sumcheck.hpp"

namespace spg {

// ------------------------------------------------------------------------------------ kernels
__global__ void k_u32_to_fq(const uint32_t* __restrict__ in, Fq* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = fq_from_u64(in[i]);
}

// derefs[s][b][i] = mem_s[addr[s][b][i]]  (s = 0: rows with eq(rx), s = 1: cols with eq(ry))
__global__ void k_gather(const uint32_t* __restrict__ addr, const Fq* __restrict__ mem_rx, const Fq* __restrict__ mem_ry,
                         size_t BN, Fq* __restrict__ out) {
  size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * BN) return;
  out[t] = (t < BN ? mem_rx : mem_ry)[addr[t]];
}

// hash(addr, val, ts) = ts * r_hash^2 + val * r_hash + addr - r_multiset  (sparse_mlpoly.rs:621-626)
__device__ __forceinline__ Fq hash3(const Fq& a, const Fq& v, const Fq& ts, const Fq& rh, const Fq& rh2, const Fq& rms) {
  return fq_sub(fq_add(fq_add(fq_mul(ts, rh2), fq_mul(v, rh)), a), rms);
}
// leaves of the 4B ops circuits (row read b, row write b, col read b, col write b), written into the trees.
// Sharded proofs (W ranks) keep the leaves i = W i' + r of rank r: local leaf i' of m = N / W (W = 1: all)
__global__ void k_hash_ops(const uint32_t* __restrict__ addr, const uint32_t* __restrict__ rts,
                           const Fq* __restrict__ derefs, size_t B, int logN, int logm, uint32_t W, uint32_t r, Fq rh,
                           Fq rh2, Fq rms, Fq* __restrict__ tree) {
  const size_t N = (size_t)1 << logN, m = (size_t)1 << logm;
  size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * B * m) return;
  size_t sb = t >> logm, il = t & (m - 1);  // sb = side * B + b
  size_t s = sb >= B, b = sb - s * B, g = sb * N + il * W + r;
  Fq a = fq_from_u64(addr[g]), ts = fq_from_u64(rts[g]), v = derefs[g];
  tree[((2 * s) * B + b) * 2 * m + il] = hash3(a, v, ts, rh, rh2, rms);
  tree[((2 * s + 1) * B + b) * 2 * m + il] = hash3(a, v, fq_add(ts, fq_one()), rh, rh2, rms);
}
// leaves of the 4 memory circuits (row init, row audit, col init, col audit); cell i = W i' + r as above
__global__ void k_hash_mem(const uint32_t* __restrict__ audit, const Fq* __restrict__ mem_rx,
                           const Fq* __restrict__ mem_ry, int logC, int logm, uint32_t W, uint32_t r, Fq rh, Fq rh2,
                           Fq rms, Fq* __restrict__ tree) {
  const size_t cells = (size_t)1 << logC, m = (size_t)1 << logm;
  size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * m) return;
  size_t s = t >> logm, il = t & (m - 1), i = il * W + r;
  Fq a = fq_from_u64(i), v = (s ? mem_ry : mem_rx)[i];
  tree[(2 * s) * 2 * m + il] = hash3(a, v, fq_zero(), rh, rh2, rms);
  tree[(2 * s + 1) * 2 * m + il] = hash3(a, v, fq_from_u64(audit[s * cells + i]), rh, rh2, rms);
}
// AddrTimestamps::new (sparse_mlpoly.rs:219-253) on the device: read_ts[t] = #{t' < t : addr[t'] = addr[t]} and
// audit[a] = #{t : addr[t] = a} over the ops in batch order. counts -> exclusive scan = each address's first
// rank; a stable radix sort of (addr, t) lists every address's ops in order, so sorted position j holds op t with
// read_ts = j - start[addr].
__global__ void k_ts_count(const uint32_t* __restrict__ addr, size_t n, uint32_t* __restrict__ cnt) {
  size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n) atomicAdd(&cnt[addr[t]], 1u);
}
__global__ void k_iota(uint32_t* __restrict__ v, size_t n) {
  size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n) v[t] = (uint32_t)t;
}
__global__ void k_ts_rank(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ ops,
                          const uint32_t* __restrict__ start, size_t n, uint32_t* __restrict__ rts) {
  size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n) rts[ops[j]] = (uint32_t)j - start[keys[j]];
}

// the dot-product circuits' inputs in one launch: circuit piece j = (2b + h) * 3 + k of length nl is this rank's
// interleaved share (i * W + r) of half h of instance b's row derefs (k = 0), col derefs (k = 1) or values (k = 2)
__global__ void k_dotp_gather(Fq* __restrict__ dst, const Fq* __restrict__ derefs, const Fq* __restrict__ val,
                              size_t BN, size_t N, size_t hN, size_t nl, uint32_t W, uint32_t r) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nl) return;
  const uint32_t j = blockIdx.y, k = j % 3, h = (j / 3) & 1, b = j / 6;
  const Fq* src = (k < 2 ? derefs + k * BN : val) + b * N + h * hN;
  dst[(size_t)j * nl + i] = src[i * W + r];
}
// sum_i base[s * seglen + i] * eq[i] for segments s = blockIdx.y (DensePolynomial::evaluate on HBM)
__global__ void __launch_bounds__(256) k_seg_dot(const Fq* __restrict__ base, size_t seglen, const Fq* __restrict__ eq,
                                                 size_t n, Fq* __restrict__ partials) {
  const size_t s = blockIdx.y;
  Fq acc = fq_zero(), z = fq_zero(), z2 = fq_zero();
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    acc = fq_add(acc, fq_mul(base[s * seglen + i], eq[i]));
  block_sum3_sp(acc, z, z2);
  if (threadIdx.x == 0) partials[s * gridDim.x + blockIdx.x] = acc;
}

// ------------------------------------------------------------------------------------ host helpers

// out[s] = sum_i base[s * seglen + i] * eq[i], i < n, s < nseg; sharded: rank r sums its balanced share of i.
// Several such dot sets queued back to back into disjoint workspace ranges: one download (and, sharded, one
// summing allgather) for all of them instead of one per set.
struct SegDotJob {
  const Fq* base;
  size_t seglen, nseg;
  const Fq* d_eq;
  size_t n;
  FqV* out;
};
static int seg_dots_multi(spg_ctx* ctx, const std::vector<SegDotJob>& jobs, const Shard& sh = Shard()) {
  std::vector<unsigned> nbs(jobs.size(), 0);
  size_t tot_part = 0, tot_res = 0;
  bool all_local = true;
  for (size_t k = 0; k < jobs.size(); k++) {
    const SegDotJob& j = jobs[k];
    const size_t nm = shard_begin(j.n, sh.n, sh.rank + 1) - shard_begin(j.n, sh.n, sh.rank);
    if (nm) nbs[k] = (unsigned)std::min<size_t>(nblk(nm), std::max<size_t>(1, 2048 / j.nseg));
    else all_local = false;
    tot_part += j.nseg * nbs[k];
    tot_res += j.nseg;
  }
  FqV all(tot_res, fq_zero());
  int rc = 0;
  if (tot_part) {
    Fq* part = (Fq*)ws_get(ctx, Ws::SegPart, tot_part * sizeof(Fq) + 64);
    Fq* dres = (Fq*)ws_get(ctx, Ws::Seg, tot_res * sizeof(Fq) + 64);
    if (!part || !dres) rc = set_err(ctx, SPG_E_NOMEM, "seg_dots");
    if (!rc && !all_local && hipMemsetAsync(dres, 0, tot_res * sizeof(Fq), ctx->stream) != hipSuccess)
      rc = set_err(ctx, SPG_E_HIP, "seg_dots memset");
    size_t po = 0, ro = 0;
    for (size_t k = 0; !rc && k < jobs.size(); k++) {
      const SegDotJob& j = jobs[k];
      if (nbs[k]) {
        const size_t i0 = shard_begin(j.n, sh.n, sh.rank), nm = shard_begin(j.n, sh.n, sh.rank + 1) - i0;
        KScope ks(ctx, "spark_evaluate", 32.0 * nm * j.nseg + 32.0 * nm);
        hipLaunchKernelGGL(k_seg_dot, dim3(nbs[k], (unsigned)j.nseg), dim3(256), 0, ctx->stream, j.base + i0, j.seglen,
                           j.d_eq + i0, nm, part + po);
        hipLaunchKernelGGL(k_sum_seg, dim3((unsigned)j.nseg), dim3(256), 0, ctx->stream, part + po, (int)nbs[k],
                           dres + ro);
        if (hipGetLastError() != hipSuccess) rc = set_err(ctx, SPG_E_HIP, "seg_dots launch");
      }
      po += j.nseg * nbs[k];
      ro += j.nseg;
    }
    if (!rc) rc = d2h_fq(ctx, dres, all.data(), tot_res);
  }
  rc = comm_sum_fq(ctx, sh, rc, all.data(), tot_res);
  if (rc) return rc;
  size_t ro = 0;
  for (const SegDotJob& j : jobs) {
    j.out->assign(all.begin() + ro, all.begin() + ro + j.nseg);
    ro += j.nseg;
  }
  return 0;
}

// n-to-1 reduction of claimed evaluations (sparse_mlpoly.rs:92-112, 868-883)
static void combine_evals(const FqV& evals, const FqV& r, const char* label, Tr& t, FqV* r_joint, Fq* eval) {
  FqV ch = t.challenges(label, lg2(evals.size()));
  FqV v = evals;
  for (size_t i = ch.size(); i-- > 0;) {  // bound_poly_var_bot with challenge i
    size_t n = v.size() / 2;
    for (size_t k = 0; k < n; k++) v[k] = fq_add(v[2 * k], fq_mul(ch[i], fq_sub(v[2 * k + 1], v[2 * k])));
    v.resize(n);
  }
  *eval = v[0];
  *r_joint = ch;
  r_joint->insert(r_joint->end(), r.begin(), r.end());
}

}  // namespace spg

using namespace spg;

// ------------------------------------------------------------------------------------ the commitment
extern "C" int spg_spark_free(spg_ctx* ctx, spg_spark* S) {
  if (!S) return SPG_OK;
  hipFree(S->d_addr);
  hipFree(S->d_rts);
  hipFree(S->d_audit);
  hipFree(S->d_val);
  hipFree(S->d_comb_ops);
  hipFree(S->d_comb_mem);
  spg_gens_free(ctx, S->dev);
  delete S;
  return SPG_OK;
}

namespace spg {
namespace {

// a handle under construction: freed on every early exit, released to the caller at the end
struct SparkFree {
  spg_ctx* ctx;
  void operator()(spg_spark* S) const { spg_spark_free(ctx, S); }
};
using SparkPtr = std::unique_ptr<spg_spark, SparkFree>;

SparkPtr spark_new(spg_ctx* ctx, size_t B, size_t N, size_t cells, const SparkShape& sp) {
  SparkPtr S(new spg_spark(), SparkFree{ctx});
  S->B = B;
  S->N = N;
  S->cells = cells;
  S->comb_ops_len = sp.ops_len;
  S->comb_mem_len = sp.mem_len;
  S->der_len = sp.der_len;
  return S;
}
// the three PolyCommitmentGens share one label: prefixes of one derived stream
int spark_gens(spg_ctx* ctx, spg_spark* S, const SparkShape& sp, const uint8_t* label, size_t label_len) {
  const int rc = spg_gens_derive(ctx, label, label_len, sp.gens_n() + 1, &S->dev);
  if (rc) return rc;
  S->g_ops = gens_view(S->dev, sp.nv_ops);
  S->g_mem = gens_view(S->dev, sp.nv_mem);
  S->g_der = gens_view(S->dev, sp.nv_der);
  return 0;
}

// the dense representation's addresses ([2][B][N]: rows, then cols) and values on the host (multi_sparse_to_dense_rep,
// sparse_mlpoly.rs:368-425); padding ops read address 0
int dense_rep_host(spg_ctx* ctx, const std::vector<SparsePoly>& polys, size_t nvx, size_t nvy, size_t N,
                   std::vector<uint32_t>* addr, std::vector<Fq>* val) {
  const size_t B = polys.size();
  addr->assign(2 * B * N, 0);
  val->assign(B * N, fq_zero());
  for (size_t k = 0; k < B; k++) {
    const spg_sparse_entry* E = polys[k].e;
    if (polys[k].nnz && !E) return SPG_E_ARG;
    for (size_t i = 0; i < polys[k].nnz; i++) {
      if (E[i].row >= ((uint64_t)1 << nvx) || E[i].col >= ((uint64_t)1 << nvy))
        return set_err(ctx, SPG_E_ARG, "sparse entry outside the matrix");
      (*addr)[k * N + i] = (uint32_t)E[i].row;
      (*addr)[B * N + k * N + i] = (uint32_t)E[i].col;
      memcpy((*val)[k * N + i].l, E[i].val, 32);
    }
  }
  return 0;
}
// .. uploaded, beside the device vectors the next two steps fill
int spark_upload(spg_ctx* ctx, spg_spark* S, const std::vector<uint32_t>& addr, const std::vector<Fq>& val) {
  auto up = [&](void** d, const void* h, size_t bytes) -> bool {
    return hipMalloc(d, bytes + 64) == hipSuccess && hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  if (!up((void**)&S->d_addr, addr.data(), addr.size() * 4) || hipMalloc(&S->d_rts, addr.size() * 4 + 64) != hipSuccess ||
      hipMalloc(&S->d_audit, 2 * S->cells * 4 + 64) != hipSuccess ||
      !up((void**)&S->d_val, val.data(), val.size() * sizeof(Fq)) ||
      hipMalloc(&S->d_comb_ops, S->comb_ops_len * sizeof(Fq)) != hipSuccess ||
      hipMalloc(&S->d_comb_mem, S->comb_mem_len * sizeof(Fq)) != hipSuccess)
    return set_err(ctx, SPG_E_NOMEM, "spark upload");
  return 0;
}
// AddrTimestamps::new (sparse_mlpoly.rs:219-253) for the row and the column side, on the device (see k_ts_count)
int addr_timestamps(spg_ctx* ctx, spg_spark* S) {
  hipStream_t s = ctx->stream;
  const size_t BN = S->B * S->N, cells = S->cells;
  int bits = 1;
  while (((size_t)1 << bits) < cells) bits++;
  uint32_t* tmpk = (uint32_t*)ws_get(ctx, Ws::SparkTsKeys, 3 * BN * 4 + 4 * (cells + 1) + 64);
  size_t sort_bytes = 0, scan_bytes = 0;
  hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                     (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)BN, 0, bits, s);
  hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)cells, s);
  void* tmps = ws_get(ctx, Ws::SparkTsTemp, std::max(sort_bytes, scan_bytes) + 64);
  if (!tmpk || !tmps) return set_err(ctx, SPG_E_NOMEM, "timestamps workspace");
  uint32_t *keys = tmpk, *ops_in = tmpk + BN, *ops = tmpk + 2 * BN, *start = tmpk + 3 * BN;
  int rc = 0;
  for (size_t side = 0; side < 2 && !rc; side++) {
    const uint32_t* ad = S->d_addr + side * BN;
    uint32_t* au = S->d_audit + side * cells;
    if (hipMemsetAsync(au, 0, cells * 4, s) != hipSuccess) rc = SPG_E_HIP;
    hipLaunchKernelGGL(k_ts_count, dim3(nblk(BN)), dim3(256), 0, s, ad, BN, au);
    if (hipcub::DeviceScan::ExclusiveSum(tmps, scan_bytes, au, start, (int)cells, s) != hipSuccess) rc = SPG_E_HIP;
    hipLaunchKernelGGL(k_iota, dim3(nblk(BN)), dim3(256), 0, s, ops_in, BN);
    if (hipcub::DeviceRadixSort::SortPairs(tmps, sort_bytes, ad, keys, ops_in, ops, (int)BN, 0, bits, s) != hipSuccess)
      rc = SPG_E_HIP;
    hipLaunchKernelGGL(k_ts_rank, dim3(nblk(BN)), dim3(256), 0, s, keys, ops, start, BN, S->d_rts + side * BN);
  }
  if (rc || hipGetLastError() != hipSuccess) return set_err(ctx, SPG_E_HIP, "spark timestamps");
  return 0;
}
// comb_ops = merge(row addr, row read_ts, col addr, col read_ts, val); comb_mem = row audit ++ col audit
int comb_vectors(spg_ctx* ctx, spg_spark* S) {
  hipStream_t s = ctx->stream;
  const size_t BN = S->B * S->N, cells = S->cells;
  int rc = 0;
  if (hipMemsetAsync(S->d_comb_ops, 0, S->comb_ops_len * sizeof(Fq), s) != hipSuccess) rc = SPG_E_HIP;
  hipLaunchKernelGGL(k_u32_to_fq, dim3(nblk(BN)), dim3(256), 0, s, S->d_addr, S->d_comb_ops, BN);
  hipLaunchKernelGGL(k_u32_to_fq, dim3(nblk(BN)), dim3(256), 0, s, S->d_rts, S->d_comb_ops + BN, BN);
  hipLaunchKernelGGL(k_u32_to_fq, dim3(nblk(BN)), dim3(256), 0, s, S->d_addr + BN, S->d_comb_ops + 2 * BN, BN);
  hipLaunchKernelGGL(k_u32_to_fq, dim3(nblk(BN)), dim3(256), 0, s, S->d_rts + BN, S->d_comb_ops + 3 * BN, BN);
  if (hipMemcpyAsync(S->d_comb_ops + 4 * BN, S->d_val, BN * sizeof(Fq), hipMemcpyDeviceToDevice, s) != hipSuccess)
    rc = SPG_E_HIP;
  hipLaunchKernelGGL(k_u32_to_fq, dim3(nblk(2 * cells)), dim3(256), 0, s, S->d_audit, S->d_comb_mem, 2 * cells);
  if (rc || hipGetLastError() != hipSuccess) return set_err(ctx, SPG_E_HIP, "spark dense representation");
  return 0;
}

}  // namespace

// SparseMatPolynomial::multi_commit (sparse_mlpoly.rs:566-587) over `polys` (num_vars_x / num_vars_y of the
// matrices) with SparseMatPolyCommitmentGens::new(label, gens_nvx, gens_nvy, gens_nnz, gens_batch)
int spark_commit_polys(spg_ctx* ctx, const std::vector<SparsePoly>& polys, size_t nvx, size_t nvy,
                       const uint8_t* label, size_t label_len, size_t gens_nvx, size_t gens_nvy, size_t gens_nnz,
                       size_t gens_batch, spg_spark** out, const Shard& sh) {
  if (!ctx || polys.empty() || !label || !out) return SPG_E_ARG;
  const size_t B = polys.size();
  size_t max_nnz = 0;
  for (auto& p : polys) max_nnz = std::max(max_nnz, p.nnz);
  const size_t N = spark_num_ops(max_nnz), cells = spark_num_cells(nvx, nvy);
  if (const char* why = spark_commit_refusal(B, N, cells, nvx, nvy, gens_nvx, gens_nvy, gens_nnz, gens_batch))
    return set_err(ctx, SPG_E_ARG, why);
  const SparkShape sp(B, N, cells, gens_nvx, gens_nvy, gens_nnz, gens_batch);
  std::vector<uint32_t> addr;
  std::vector<Fq> val;
  if (int rc = dense_rep_host(ctx, polys, nvx, nvy, N, &addr, &val)) return rc;
  SparkPtr S = spark_new(ctx, B, N, cells, sp);
  int rc = spark_upload(ctx, S.get(), addr, val);
  if (!rc) rc = addr_timestamps(ctx, S.get());
  if (!rc) rc = comb_vectors(ctx, S.get());
  if (!rc) rc = spark_gens(ctx, S.get(), sp, label, label_len);
  if (!rc) rc = commit_dev(ctx, S->g_ops, S->d_comb_ops, lg2(S->comb_ops_len), &S->comm_ops, sh);
  if (!rc) rc = commit_dev(ctx, S->g_mem, S->d_comb_mem, lg2(S->comb_mem_len), &S->comm_mem, sh);
  if (rc) return rc;
  *out = S.release();
  return SPG_OK;
}

int spark_from_comm(spg_ctx* ctx, size_t B, size_t N, size_t cells, const std::vector<Pt>& comm_ops,
                    const std::vector<Pt>& comm_mem, const uint8_t* label, size_t label_len, size_t gens_nvx,
                    size_t gens_nvy, size_t gens_nnz, size_t gens_batch, spg_spark** out) {
  if (const char* why = spark_comm_refusal(B, N, cells, comm_ops.size(), comm_mem.size(), gens_nvx, gens_nvy, gens_nnz,
                                           gens_batch))
    return set_err(ctx, SPG_E_ARG, why);
  const SparkShape sp(B, N, cells, gens_nvx, gens_nvy, gens_nnz, gens_batch);
  SparkPtr S = spark_new(ctx, B, N, cells, sp);
  if (int rc = spark_gens(ctx, S.get(), sp, label, label_len)) return rc;
  S->comm_ops = comm_ops;
  S->comm_mem = comm_mem;
  *out = S.release();
  return SPG_OK;
}

// bincode(SparseMatPolyCommitment) (sparse_mlpoly.rs:319-325)
void spark_comm_ser(const spg_spark* S, Writer& w) {
  w.u64(S->B);
  w.u64(S->N);
  w.u64(S->cells);
  w.pts(S->comm_ops);
  w.pts(S->comm_mem);
}
// SparseMatPolyCommitment::append_to_transcript (sparse_mlpoly.rs:327-339)
void spark_comm_append(const spg_spark* S, Tr& t) {
  t.u64("batch_size", S->B);
  t.u64("num_ops", S->N);
  t.u64("num_mem_cells", S->cells);
  append_polycomm(t, "comm_comb_ops", S->comm_ops);
  append_polycomm(t, "comm_comb_mem", S->comm_mem);
}

}  // namespace spg

extern "C" int spg_spark_commit(spg_ctx* ctx, const spg_r1cs_instance* ci, const uint8_t* label, size_t label_len,
                                size_t gens_nnz, size_t gens_batch, spg_spark** out, uint8_t* comm, size_t comm_cap,
                                size_t* comm_len) {
  if (!ctx || !ci || !label || !out || !comm_len || !ci->num_instances || !ci->nnz || !ci->entries) return SPG_E_ARG;
  if (!is_pow2(ci->max_num_cons) || !is_pow2(ci->num_vars)) return set_err(ctx, SPG_E_ARG, "sizes must be powers of 2");
  std::vector<SparsePoly> polys;
  for (size_t k = 0; k < 3 * ci->num_instances; k++) polys.push_back({ci->entries[k], ci->nnz[k]});
  const size_t nvx = lg2(ci->max_num_cons), nvy = lg2(ci->num_vars);
  spg_spark* S = nullptr;
  int rc = spark_commit_polys(ctx, polys, nvx, nvy, label, label_len, nvx, nvy, gens_nnz, gens_batch, &S,
                              ctx_shard(ctx));
  if (rc) return rc;
  Writer w;
  spark_comm_ser(S, w);
  *comm_len = w.out.size();
  *out = S;
  if (!comm || w.out.size() > comm_cap) return set_err(ctx, SPG_E_ARG, "commitment buffer too small");
  memcpy(comm, w.out.data(), w.out.size());
  return SPG_OK;
}

namespace spg {
namespace {

// SparseMatPolyEvalProof::prove (sparse_mlpoly.rs:1497-1564). run() calls the stages in protocol order; what one stage
// leaves for a later one (and for the bincode at the end) is a member.
//
// Sharded proof (sh.n = W > 1 processes, one GPU each; SURVEY 8e "SPARK product trees: shard by the low index
// bits"): every rank holds the whole dense representation and runs the same transcript. The O(N) work splits:
//   derefs commitment  Hyrax rows split over the ranks, 32-byte rows allgathered (commit_rows_sh)
//   hash layer, trees  rank r hashes leaves i = W i' + r of each circuit of >= 2W leaves and builds its local
//                      product tree; ProductCircuit::compute_layer pairs i with i + len/2, which keeps the low
//                      lg W bits, so every level stays local down to one entry per rank; those W entries are
//                      allgathered and the top lg W levels built on every rank (TreeSh, tree_tops_host)
//   layer sumchecks    batched_prove: local rounds with (e0, e2, e3) summed over the ranks, then a gather
//   hash-layer evals   contiguous shares of each dot product, summed (seg_dots)
//   PolyEvalProofs     L.Z rows split, partial vectors summed; Bullet replicated (poly_eval_prove)
// A circuit set of fewer than 2W leaves (or W not a power of two) stays whole on every rank. Every collective
// carries the rank's status.
struct SparkProver {
  spg_ctx* ctx;
  spg_spark* S;
  FqV ex, ey;
  Tr& t;
  Tape& tape;
  const Shard& sh;
  const size_t B = S->B, N = S->N, BN = B * N, cells = S->cells, hN = N / 2;
  hipStream_t s = ctx->stream;
  Laps lp;
  TreeSh tso, tsm;  // the ops and the memory circuit sets: interleaved shards (W = 1: whole)
  size_t hNl = 0;   // entries of a dot-product circuit's vectors held here
  // workspace: eq(rx), eq(ry) over the cells; the derefs; the dot-product circuits' inputs; the circuits' products;
  // eq(rand_ops), eq(rand_mem)
  Fq *mem_rx = nullptr, *mem_ry = nullptr, *der = nullptr, *dotbuf = nullptr, *dtops = nullptr, *eq_ops = nullptr,
     *eq_mem = nullptr;
  std::vector<Pt> comm_derefs;
  // ProductCircuit::evaluate of the 4B ops circuits (row read, row write, col read, col write: B each), then of the
  // memory circuits (row init, row audit, col init, col audit)
  FqV tops;
  std::vector<Triple> dotp;
  FqV dotp_claims;  // (left_b, right_b) interleaved
  BatchedProofP proof_ops, proof_mem;
  FqV rand_ops, rand_mem;
  FqV ev_der, ev_ops, ev_mem;
  DotProductProofLogP pf_der, pf_ops, pf_mem;

  int run(Writer& w);
  int plan();
  int derefs();
  int hash_and_trees();
  int sharded_tops(int rc);
  int product_layer();
  int hash_layer_evals();
  int open(const char* evals_label, FqV ev, const FqV& rand, const char* combine_label, const char* joint_label,
           ProverGens& g, const Fq* d_poly, DotProductProofLogP* pf);
  int openings();
  void serialize(Writer& w) const;
};

int SparkProver::run(Writer& w) {
  lp.title = "SparseMatPolyEvalProof::prove";
  int rc = plan();
  if (!rc) rc = derefs();
  if (!rc) rc = hash_and_trees();
  if (!rc) rc = product_layer();
  if (!rc) rc = hash_layer_evals();
  if (!rc) rc = openings();
  if (rc) return rc;
  lp.print();
  timer_stop(ctx);
  serialize(w);
  float ms = 0.f;
  hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  ctx->last_us = ms * 1000.0;
  return SPG_OK;
}

// rx / ry padded to one length, the split of the two circuit sets over the ranks, the workspace
int SparkProver::plan() {
  if (ex.size() < ey.size()) ex.insert(ex.begin(), ey.size() - ex.size(), fq_zero());
  if (ey.size() < ex.size()) ey.insert(ey.begin(), ex.size() - ey.size(), fq_zero());
  if (ex.size() > 40 || ((size_t)1 << ex.size()) != cells)
    return set_err(ctx, SPG_E_ARG, "rx / ry do not match the memory size");
  const size_t Wr = (size_t)sh.n;
  const bool pow2 = Wr > 1 && (Wr & (Wr - 1)) == 0;  // interleaving needs W | M (other world sizes: whole trees)
  tso.W = (pow2 && N >= 2 * Wr) ? (int)Wr : 1;
  tsm.W = (pow2 && cells >= 2 * Wr) ? (int)Wr : 1;
  tso.r = tso.W > 1 ? sh.rank : 0;
  tsm.r = tsm.W > 1 ? sh.rank : 0;
  tso.m = N / tso.W;
  tsm.m = cells / tsm.W;
  hNl = hN / tso.W;
  const size_t mo = tso.m, mm = tsm.m;
  t.protocol("Sparse polynomial evaluation proof");
  timer_start(ctx);
  mem_rx = (Fq*)ws_get(ctx, Ws::SparkMemRx, cells * sizeof(Fq) + 64);
  mem_ry = (Fq*)ws_get(ctx, Ws::SparkMemRy, cells * sizeof(Fq) + 64);
  der = (Fq*)ws_get(ctx, Ws::SparkDerefs, S->der_len * sizeof(Fq) + 64);
  tso.loc = (Fq*)ws_get(ctx, Ws::SparkTreeOps, 4 * B * 2 * mo * sizeof(Fq) + 64);
  tsm.loc = (Fq*)ws_get(ctx, Ws::SparkTreeMem, 4 * 2 * mm * sizeof(Fq) + 64);
  tso.top = tso.W > 1 ? (Fq*)ws_get(ctx, Ws::SparkTopOps, 4 * B * 2 * Wr * sizeof(Fq) + 64) : nullptr;
  tsm.top = tsm.W > 1 ? (Fq*)ws_get(ctx, Ws::SparkTopMem, 4 * 2 * Wr * sizeof(Fq) + 64) : nullptr;
  dotbuf = (Fq*)ws_get(ctx, Ws::SparkDotp, 2 * B * 3 * hNl * sizeof(Fq) + 64);
  dtops = (Fq*)ws_get(ctx, Ws::SparkTops, 4 * (B + 1) * sizeof(Fq) + 64);
  eq_ops = (Fq*)ws_get(ctx, Ws::SparkEqOps, N * sizeof(Fq) + 64);
  eq_mem = (Fq*)ws_get(ctx, Ws::SparkEqMem, cells * sizeof(Fq) + 64);
  int rc = 0;
  if (!mem_rx || !mem_ry || !der || !tso.loc || !tsm.loc || (tso.W > 1 && !tso.top) || (tsm.W > 1 && !tsm.top) ||
      !dotbuf || !dtops || !eq_ops || !eq_mem)
    rc = set_err(ctx, SPG_E_NOMEM, "spark workspace");
  if (sh.n > 1) {  // every rank enters the proof's collectives only if every rank has its workspace
    std::vector<uint8_t> none;
    rc = comm_allgather(ctx, sh, rc, nullptr, 0, none);
  }
  return rc;
}

// Derefs (sparse_mlpoly.rs:51-67): comb = row derefs ++ col derefs, zero-padded, and its commitment
int SparkProver::derefs() {
  int rc = eq_tables(ctx, {{ex, mem_rx}, {ey, mem_ry}});
  if (rc) return rc;
  const size_t der_len = S->der_len;
  if (der_len > 2 * BN) SPG_HIP(ctx, hipMemsetAsync(der + 2 * BN, 0, (der_len - 2 * BN) * sizeof(Fq), s));
  {
    KScope ks(ctx, "spark_deref", (4.0 + 32.0 + 32.0) * 2 * BN);
    hipLaunchKernelGGL(k_gather, dim3(nblk(2 * BN)), dim3(256), 0, s, S->d_addr, mem_rx, mem_ry, BN, der);
  }
  SPG_HIP(ctx, hipGetLastError());
  lp.lap("setup+deref");
  rc = commit_dev(ctx, S->g_der, der, lg2(der_len), &comm_derefs, sh);
  lp.lap("derefs_commit");
  if (rc) return rc;
  t.msg("derefs_commitment", "begin_derefs_commitment");
  append_polycomm(t, "comm_poly_row_col_ops_val", comm_derefs);
  t.msg("derefs_commitment", "end_derefs_commitment");
  return 0;
}

// the hash layer's leaves straight into the (local) trees, then the product trees (Layers::new) and their products
int SparkProver::hash_and_trees() {
  const FqV rmc = t.challenges("challenge_r_hash", 2);
  const Fq rh = rmc[0], rh2 = fq_mul(rmc[0], rmc[0]), rms = rmc[1];
  const size_t mo = tso.m, mm = tsm.m;
  {
    KScope ks(ctx, "spark_hash_layer", (8.0 + 32.0 + 64.0) * 2 * B * mo + (4.0 + 32.0 + 64.0) * 2 * mm);
    hipLaunchKernelGGL(k_hash_ops, dim3(nblk(2 * B * mo)), dim3(256), 0, s, S->d_addr, S->d_rts, der, B, (int)lg2(N),
                       (int)lg2(mo), (uint32_t)tso.W, (uint32_t)tso.r, rh, rh2, rms, tso.loc);
    hipLaunchKernelGGL(k_hash_mem, dim3(nblk(2 * mm)), dim3(256), 0, s, S->d_audit, mem_rx, mem_ry, (int)lg2(cells),
                       (int)lg2(mm), (uint32_t)tsm.W, (uint32_t)tsm.r, rh, rh2, rms, tsm.loc);
  }
  int rc = tree_build(ctx, tso.loc, 4 * B, mo, dtops);  // ProductCircuit::new (product_tree.rs:36-58), local trees
  if (!rc) rc = tree_build(ctx, tsm.loc, 4, mm, dtops + 4 * B);
  if (rc) return rc;
  tops.resize(4 * B + 4);
  rc = d2h_fq(ctx, dtops, tops.data(), tops.size());
  if (tso.W > 1 || tsm.W > 1) rc = sharded_tops(rc);
  lp.lap("hash+trees");
  return rc;
}
// sharded sets: the product of a local tree is the rank's entry of the global level with W entries; gather them, build
// the top lg W levels on every rank, and the circuits' claims. rc: this rank's status, carried by the exchange
int SparkProver::sharded_tops(int rc) {
  const size_t Wr = (size_t)sh.n;
  std::vector<uint8_t> all;
  rc = comm_allgather(ctx, sh, rc, tops.data(), tops.size() * sizeof(Fq), all);
  if (rc) return rc;
  const Fq* g = (const Fq*)all.data();
  for (int which = 0; which < 2; which++) {
    const TreeSh& ts = which ? tsm : tso;
    if (ts.W == 1) continue;
    const size_t nc = which ? 4 : 4 * B, base = which ? 4 * B : 0;
    std::vector<Fq> ht(nc * 2 * Wr, fq_zero());
    for (size_t c = 0; c < nc; c++) {
      Fq* v = ht.data() + c * 2 * Wr;
      for (size_t q = 0; q < Wr; q++) v[q] = g[q * tops.size() + base + c];
      tops[base + c] = tree_tops_host(v, Wr);
    }
    SPG_HIP(ctx, hipMemcpyAsync(ts.top, ht.data(), ht.size() * sizeof(Fq), hipMemcpyHostToDevice, s));
  }
  SPG_HIP(ctx, hipStreamSynchronize(s));  // ht is a host temporary
  return 0;
}

// PolyEvalNetworkProof -> ProductLayerProof (sparse_mlpoly.rs:1368-1402, 1118-1263)
int SparkProver::product_layer() {
  t.protocol("Sparse polynomial evaluation proof");
  t.protocol("Sparse polynomial product layer proof");
  const auto part = [&](size_t k) { return FqV(tops.begin() + k * B, tops.begin() + (k + 1) * B); };
  t.scalar("claim_row_eval_init", tops[4 * B]);
  t.scalars("claim_row_eval_read", part(0));
  t.scalars("claim_row_eval_write", part(1));
  t.scalar("claim_row_eval_audit", tops[4 * B + 1]);
  t.scalar("claim_col_eval_init", tops[4 * B + 2]);
  t.scalars("claim_col_eval_read", part(2));
  t.scalars("claim_col_eval_write", part(3));
  t.scalar("claim_col_eval_audit", tops[4 * B + 3]);
  // dot-product circuits (row derefs, col derefs, val) split into halves, interleaved (left_b, right_b);
  // copies (this rank's interleaved shares when the ops set is sharded), since the layer-0 sumcheck folds them
  // while the hash layer evaluates the originals
  for (size_t j = 0; j < 2 * B; j++) {
    Fq* base = dotbuf + j * 3 * hNl;
    dotp.push_back({base, base + hNl, base + 2 * hNl});
  }
  hipLaunchKernelGGL(k_dotp_gather, dim3(nblk(hNl), (unsigned)(6 * B)), dim3(256), 0, s, dotbuf, der, S->d_val, BN, N,
                     hN, hNl, (uint32_t)tso.W, (uint32_t)tso.r);
  SPG_HIP(ctx, hipGetLastError());
  dotp_claims.resize(2 * B);
  int rc = dotp_evaluate(ctx, dotp, hNl, dotp_claims.data());
  if (tso.W > 1) rc = comm_sum_fq(ctx, sh, rc, dotp_claims.data(), 2 * B);
  if (rc) return rc;
  for (size_t b = 0; b < B; b++) {
    t.scalar("claim_eval_dotp_left", dotp_claims[2 * b]);
    t.scalar("claim_eval_dotp_right", dotp_claims[2 * b + 1]);
  }
  lp.lap("dotp_claims");
  rc = batched_prove(ctx, tso, 4 * B, N, FqV(tops.begin(), tops.begin() + 4 * B), dotp, dotp_claims, t, &proof_ops,
                     &rand_ops, sh);
  if (!rc)
    rc = batched_prove(ctx, tsm, 4, cells, FqV(tops.begin() + 4 * B, tops.end()), {}, {}, t, &proof_mem, &rand_mem, sh);
  if (rc) return rc;
  lp.lap("layer_sumchecks");
  return 0;
}

// HashLayerProof (sparse_mlpoly.rs:805-918): the evaluations of the derefs, comb_ops and comb_mem at the layers' points
int SparkProver::hash_layer_evals() {
  t.protocol("Sparse polynomial hash layer proof");
  int rc = eq_tables(ctx, {{rand_ops, eq_ops}, {rand_mem, eq_mem}});
  if (rc) return rc;
  rc = seg_dots_multi(ctx, {{der, N, 2 * B, eq_ops, N, &ev_der}, {S->d_comb_ops, N, 5 * B, eq_ops, N, &ev_ops},
                            {S->d_comb_mem, cells, 2, eq_mem, cells, &ev_mem}}, sh);
  if (rc) return rc;
  lp.lap("hash_evals");
  return 0;
}

// One opening: the evaluations, padded with zeros to a power of two, into the transcript, their n-to-1 reduction, and
// the PolyEvalProof of the joint claim on the polynomial d_poly
int SparkProver::open(const char* evals_label, FqV ev, const FqV& rand, const char* combine_label,
                      const char* joint_label, ProverGens& g, const Fq* d_poly, DotProductProofLogP* pf) {
  ev.resize(npow2(ev.size()), fq_zero());
  t.scalars(evals_label, ev);
  FqV rj;
  Fq ej;
  combine_evals(ev, rand, combine_label, t, &rj, &ej);
  t.scalar(joint_label, ej);
  return poly_eval_prove(ctx, g, d_poly, rj, ej, t, tape, pf, sh);
}
// DerefsEvalProof::prove (sparse_mlpoly.rs:80-146), then the openings of comb_ops and of comb_mem (whose two
// evaluations need no padding)
int SparkProver::openings() {
  t.protocol("Derefs evaluation proof");
  int rc = open("evals_ops_val", ev_der, rand_ops, "challenge_combine_n_to_one", "joint_claim_eval", S->g_der, der, &pf_der);
  if (!rc)
    rc = open("claim_evals_ops", ev_ops, rand_ops, "challenge_combine_n_to_one", "joint_claim_eval_ops", S->g_ops,
              S->d_comb_ops, &pf_ops);
  if (!rc)
    rc = open("claim_evals_mem", ev_mem, rand_mem, "challenge_combine_two_to_one", "joint_claim_eval_mem", S->g_mem,
              S->d_comb_mem, &pf_mem);
  if (rc) return rc;
  lp.lap("poly_eval_proofs");
  return 0;
}

// bincode(SparseMatPolyEvalProof)
void SparkProver::serialize(Writer& w) const {
  const auto part = [&](const FqV& v, size_t k) { return FqV(v.begin() + k * B, v.begin() + (k + 1) * B); };
  w.pts(comm_derefs);
  w.fq(tops[4 * B]);  // ProductLayerProof: row init, read, write, audit; col ..; the dot-product claims
  w.fqs(part(tops, 0));
  w.fqs(part(tops, 1));
  w.fq(tops[4 * B + 1]);
  w.fq(tops[4 * B + 2]);
  w.fqs(part(tops, 2));
  w.fqs(part(tops, 3));
  w.fq(tops[4 * B + 3]);
  FqV dl(B), dr(B);
  for (size_t b = 0; b < B; b++) {
    dl[b] = dotp_claims[2 * b];
    dr[b] = dotp_claims[2 * b + 1];
  }
  w.fqs(dl);
  w.fqs(dr);
  proof_mem.ser(w);
  proof_ops.ser(w);
  w.fqs(part(ev_ops, 0));  // HashLayerProof: row addr, row read_ts, row audit, col ..., val, derefs, proofs
  w.fqs(part(ev_ops, 1));
  w.fq(ev_mem[0]);
  w.fqs(part(ev_ops, 2));
  w.fqs(part(ev_ops, 3));
  w.fq(ev_mem[1]);
  w.fqs(part(ev_ops, 4));
  w.fqs(part(ev_der, 0));
  w.fqs(part(ev_der, 1));
  pf_ops.ser(w);
  pf_mem.ser(w);
  pf_der.ser(w);
}

}  // namespace

// SparseMatPolyEvalProof::prove; appends bincode(proof) to w
int spark_prove_core(spg_ctx* ctx, spg_spark* S, FqV ex, FqV ey, const FqV& evals, Tr& t, Tape& tape, Writer& w,
                     const Shard& sh) {
  if (evals.size() != S->B) return set_err(ctx, SPG_E_ARG, "one evaluation per batched matrix");
  SparkProver p{ctx, S, std::move(ex), std::move(ey), t, tape, sh};
  return p.run(w);
}

}  // namespace spg

static int spg_spark_prove_impl(spg_ctx* ctx, spg_spark* S, const uint64_t* rx, size_t rx_len, const uint64_t* ry,
                               size_t ry_len, const uint64_t* evals_in, size_t n_evals, spg_transcript* transcript,
                               spg_random_tape* tape_h, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
  if (!ctx || !S || !transcript || !tape_h || !proof_len || (!rx && rx_len) || (!ry && ry_len) || !evals_in)
    return SPG_E_ARG;
  FqV ex, ey, evals(n_evals);
  for (size_t i = 0; i < rx_len; i++) ex.push_back(ld_fq(rx + 4 * i));
  for (size_t i = 0; i < ry_len; i++) ey.push_back(ld_fq(ry + 4 * i));
  for (size_t i = 0; i < n_evals; i++) evals[i] = ld_fq(evals_in + 4 * i);
  Writer w;
  int rc = spark_prove_core(ctx, S, ex, ey, evals, transcript->t, tape_h->t, w, ctx_shard(ctx));
  if (rc) return rc;
  *proof_len = w.out.size();
  if (!proof || w.out.size() > proof_cap) return set_err(ctx, SPG_E_ARG, "proof buffer too small");
  memcpy(proof, w.out.data(), w.out.size());
  return SPG_OK;
}

extern "C" int spg_spark_prove(spg_ctx* ctx, spg_spark* S, const uint64_t* rx, size_t rx_len, const uint64_t* ry,
                               size_t ry_len, const uint64_t* evals_in, size_t n_evals, spg_transcript* transcript,
                               spg_random_tape* tape_h, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
  if (!ctx || !transcript) return SPG_E_ARG;
  spg::HostPin pin;
  spg::TrFailScope tfs(ctx, transcript->t);
  return spg::tr_status(ctx, transcript->t, spg_spark_prove_impl(ctx, S, rx, rx_len, ry, ry_len, evals_in, n_evals, transcript, tape_h, proof, proof_cap, proof_len));
}
