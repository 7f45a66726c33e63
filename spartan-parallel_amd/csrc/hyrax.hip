// spg — Hyrax row commitments to and evaluation proofs of dense polynomials held on the device (r1cs.hip, snark.hip,
// polyeval.hip and spark.hip call these through proto.hpp).
//
//   PolyCommitmentGens::new                      src/dense_mlpoly.rs:88-98              gens_view
//   DensePolynomial::commit (no blinds)          :184-256                               commit_dev, commit_rows*
//   PolyEvalProof::prove (no blinds)             :437-490                               poly_eval_prove
//     DensePolynomial::bound                     :258-265                               k_bound_rows, k_bound_sum
#include <algorithm>

#include "hostpoly.hpp"
#include "knobs.hpp"
#include "proto.hpp"

namespace spg {

// ------------------------------------------------------------------------------------ kernels
// DensePolynomial::bound (dense_mlpoly.rs:258-265): out[i] = sum_j L[j] * Z[j * Rs + i], rows split over y
__global__ void __launch_bounds__(256) k_bound_rows(const Fq* __restrict__ Z, const Fq* __restrict__ L, size_t Ls,
                                                    size_t Rs, size_t chunk, Fq* __restrict__ part) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Rs) return;
  size_t j0 = blockIdx.y * chunk, j1 = j0 + chunk < Ls ? j0 + chunk : Ls;
  Fq acc = fq_zero();
  for (size_t j = j0; j < j1; j++) acc = fq_add(acc, fq_mul(L[j], Z[j * Rs + i]));
  part[(size_t)blockIdx.y * Rs + i] = acc;
}
// out[i] = sum_y part[y][i]: a block owns 16 columns and 16 lanes per column split the S partials (S reaches
// thousands when Rs is small, and one lane per column made that a chain of S dependent additions), then an LDS tree
constexpr int kBoundSumCols = 16;
__global__ void __launch_bounds__(256) k_bound_sum(const Fq* __restrict__ part, size_t S, size_t Rs,
                                                   Fq* __restrict__ out) {
  __shared__ Fq sm[256];
  const int t = threadIdx.x, c = t % kBoundSumCols, y0 = t / kBoundSumCols;
  const size_t i = (size_t)blockIdx.x * kBoundSumCols + c;
  constexpr int YL = 256 / kBoundSumCols;
  Fq acc = fq_zero();
  if (i < Rs)
    for (size_t y = y0; y < S; y += YL) acc = fq_add(acc, part[y * Rs + i]);
  sm[t] = acc;
  __syncthreads();
#pragma unroll
  for (int h = YL / 2; h >= 1; h >>= 1) {
    if (y0 < h) sm[t] = fq_add(sm[t], sm[t + kBoundSumCols * h]);
    __syncthreads();
  }
  if (y0 == 0 && i < Rs) out[i] = sm[t];
}

// Hyrax rows up to this many scalars go through the latency MSM path (one block per bucket and row)
static const size_t kSmallRowMax = 256;
static const size_t kHostFinalRows = 64;  // latency-path commits of at most this many rows finish on the host

// PolyCommitmentGens::new(nv, label) as a view of one derived generator stream (dense_mlpoly.rs:88-98)
ProverGens gens_view(spg_gens* dev, size_t nv) {
  ProverGens g;
  g.dev = dev;
  g.host.init(dev->compressed, dev->n + 1);
  size_t n = (size_t)1 << (nv - nv / 2);
  g.n_pc = n;
  g.gens_n.G.resize(n);
  for (size_t i = 0; i < n; i++) g.gens_n.G[i] = i;
  g.gens_n.h = n + 1;
  g.gens_1.G = {n};
  g.gens_1.h = n + 1;
  return g;
}

// Encodings of B device points into host Pt's. Up to SPG_HOST_ENC_MAX (384) points the points come down (128 B each)
// and are encoded on the host pool: one encoding is a ~2.4 us inverse square root on a host core, while
// k_compress_ext gives each point one GPU lane whose ~250 dependent squarings take ~130 us whatever the count.
// Larger batches encode on the device (d_out: 32 B per point of device scratch).
// halved: the device points are P / 2 (msm_comb's halve), encoded as the doubles on the host pool in chunks of one
// field inversion each (hext_double_and_compress_batch: ~25 products per point instead of a ~265-step inverse square
// root on a GPU lane or a host core), at any count
static int encode_points(spg_ctx* ctx, const Ext* d_ext, size_t B, Pt* out, uint8_t* d_out, bool halved = false) {
  const size_t host_max = (size_t)knob::host_enc_max();
  if (halved) {
    Ext* h = (Ext*)enc_stage_get(ctx, B * sizeof(Ext));
    if (!h) return set_err(ctx, SPG_E_NOMEM, "encoding staging");
    const bool tr3 = knob::trace() >= 3;
    const auto t0 = std::chrono::steady_clock::now();
    SPG_HIP(ctx, hipMemcpyAsync(h, d_ext, B * sizeof(Ext), hipMemcpyDeviceToHost, ctx->stream));
    SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const auto t1 = std::chrono::steady_clock::now();
    encode_halved_host(h, B, out);
    if (tr3)
      fprintf(stderr, "[spg] halved encodings of %zu points: device + download %.0f us, host %.0f us\n", B,
              std::chrono::duration<double, std::micro>(t1 - t0).count(),
              std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count());
    return 0;
  }
  if (B <= host_max) {
    Ext* h = (Ext*)enc_stage_get(ctx, B * sizeof(Ext));
    if (!h) return set_err(ctx, SPG_E_NOMEM, "encoding staging");
    SPG_HIP(ctx, hipMemcpyAsync(h, d_ext, B * sizeof(Ext), hipMemcpyDeviceToHost, ctx->stream));
    SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int C = B >= 16 ? (int)std::min<size_t>(B / 2, (size_t)pool().size() + 1) : 1;
    auto enc = [&](int c) {
      for (size_t i = B * c / C; i < B * (c + 1) / C; i++) out[i] = compress(h::hext_from_dev(h[i]));
    };
    if (C == 1)
      enc(0);
    else
      pool().parallel_for(C, enc);
    return 0;
  }
  int rc = compress_ext_device(ctx, d_ext, B, d_out);
  if (rc) return rc;
  SPG_HIP(ctx, hipMemcpyAsync(out, d_out, 32 * B, hipMemcpyDeviceToHost, ctx->stream));
  SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

// L rows of R device scalars on the latency-path generators into device points: the comb tables when they apply
// (>= 64 rows, >= 2^14 scalars in all), else the latency-path bucket kernels
// (*halved: the comb path left P / 2, encode_points' halved form, when `want` -- batches of >= kHalvedMin points
// (proto.hpp); SPG_HALVED_ENC=0 keeps the device / lone encodings everywhere)
static int rows_to_points(spg_ctx* ctx, ProverGens& g, const Fq* d_Z, size_t R, size_t L, Ext* d_ext, bool* halved,
                          bool want) {
  const bool halve = knob::halved_enc() && want;
  *halved = false;
  if (L >= 64 && L * R >= ((size_t)1 << 14)) {
    const int rc = msm_comb(ctx, g.dev, 0, d_Z, R, L, nullptr, nullptr, -1, d_ext, halve);
    if (rc != kCombSkip) {
      *halved = halve;
      return rc;
    }
  }
  return msm_small_device(ctx, g.dev, 0, d_Z, R, L, nullptr, d_ext, nullptr, -1);
}

// L Hyrax rows of R consecutive device scalars each -> L compressed row commitments (host). Rows of up to
// kSmallRowMax scalars take the latency MSM path (one block per bucket and row), longer rows the sorted batch
// pipeline in chunks that keep its sort within 32-bit indices.
int commit_rows(spg_ctx* ctx, ProverGens& g, const Fq* d_Z, size_t R, size_t L, Pt* out) {
  if (R > g.n_pc) return set_err(ctx, SPG_E_ARG, "commit: rows wider than the generators");
  const bool small = R <= kSmallRowMax;
  const size_t chunk = small ? std::min<size_t>(L, 65535)
                             : std::max<size_t>(1, std::min<size_t>(L, ((size_t)1 << 24) / R));
  uint8_t* d_out = (uint8_t*)ws_get(ctx, Ws::Commit, 32 * chunk + 64);
  if (!d_out) return set_err(ctx, SPG_E_NOMEM, "commit out");
  const bool trace2 = knob::trace() >= 2;
  // SPG_HOST_COMMIT_MAX (default 0: off): row batches of at most this many scalars are committed on the host pool against
  // the generators' fixed-base byte tables (HostGens, built once per generator set): the scalars come down (<= 32 KB)
  // and 32 mixed additions per scalar spread over the pool, instead of a device bucket launch, its host finals and a
  // synchronisation (8 scalars: 35-40 us against 44-49 us; 256: 69 against 79 us; 512 scalars already take longer there,
  // 115 against 86 us, profiles/r05_ab_host_commit.txt). Off: a generator's table is built on its first use (11-24 ms
  // for the 8- and 16-generator rows of config 4's first proof), and config 4 measured 4.03 against 3.86 ms with it
  // (ABBA, profiles/r05_ab_host_commit_c4.txt)
  const size_t host_commit_max = (size_t)knob::host_commit_max();
  for (size_t r0 = 0; r0 < L; r0 += chunk) {
    size_t nb = std::min(chunk, L - r0);
    auto t0 = std::chrono::steady_clock::now();
    if (small && nb * R <= host_commit_max) {
      FqV hz(nb * R);
      SPG_HIP(ctx, hipMemcpyAsync(hz.data(), d_Z + r0 * R, nb * R * sizeof(Fq), hipMemcpyDeviceToHost, ctx->stream));
      SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
      std::vector<std::pair<std::vector<size_t>, FqV>> jobs(nb);
      std::vector<size_t> idx(R);
      for (size_t i = 0; i < R; i++) idx[i] = g.gens_n.G[i];
      for (size_t b = 0; b < nb; b++) {
        jobs[b].first = idx;
        jobs[b].second.assign(hz.begin() + b * R, hz.begin() + (b + 1) * R);
      }
      const std::vector<Pt> pts = g.host.commit_many(jobs);
      std::copy(pts.begin(), pts.end(), out + r0);
    } else if (small && nb <= kHostFinalRows) {
      // few rows: the bucket running sums and encodings are cheaper on host cores than the device's
      // one-lane-per-row final + compress (~0.25 ms floor)
      void* d_map = nullptr;
      Ext* mbk = (Ext*)mapped_get(ctx, sizeof(Ext) * nb * 256, &d_map);  // buckets straight into host memory
      Ext* d_bk = mbk ? (Ext*)d_map : (Ext*)ws_get(ctx, Ws::CommitBk, sizeof(Ext) * nb * 256 + 64);
      Ext* bk = mbk ? mbk : (Ext*)pinned_get(ctx, sizeof(Ext) * nb * 256);
      if (!d_bk || !bk) return set_err(ctx, SPG_E_NOMEM, "commit buckets");
      int NB = 0;
      int rc = msm_small_buckets(ctx, g.dev, 0, d_Z + r0 * R, R, nb, nullptr, nullptr, -1, d_bk, &NB);
      if (rc) return rc;
      if (!mbk)
        SPG_HIP(ctx, hipMemcpyAsync(bk, d_bk, sizeof(Ext) * nb * NB, hipMemcpyDeviceToHost, ctx->stream));
      SPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
      bucket_finals(bk, nb, NB, out + r0);
    } else if (small) {
      Ext* d_ext = (Ext*)ws_get(ctx, Ws::CommitExt, sizeof(Ext) * nb + 64);
      if (!d_ext) return set_err(ctx, SPG_E_NOMEM, "commit points");
      bool halved = false;
      int rc = rows_to_points(ctx, g, d_Z + r0 * R, R, nb, d_ext, &halved, nb >= kHalvedMin);
      if (!rc) rc = encode_points(ctx, d_ext, nb, out + r0, d_out, halved);  // synchronous: d_ext, d_out reused next chunk
      if (rc) return rc;
    } else {  // (halved comb points encoded on the host where the comb applies; synchronous)
      const int rc = msm_rows_host_enc(ctx, g.dev, d_Z + r0 * R, R, nb, nullptr, (long)(g.n_pc + 1), (uint8_t*)(out + r0));
      if (rc) return rc;
    }
    if (trace2)
      fprintf(stderr, "[spg] commit rows=%zu R=%zu %s %.0f us\n", nb, R,
              small && nb * R <= host_commit_max ? "host" : (small ? "small" : "batch"),
              std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
  return 0;
}

static bool rows_merged(const RowJob& j) { return j.R <= kSmallRowMax && j.L > kHostFinalRows && j.L <= 65535; }

int commit_rows_many_launch(spg_ctx* ctx, ProverGens& g, const std::vector<RowJob>& jobs, RowsPending* p) {
  p->tot = 0;
  p->hv.clear();
  for (const RowJob& j : jobs) {
    if (j.R > g.n_pc) return set_err(ctx, SPG_E_ARG, "commit: rows wider than the generators");
    if (rows_merged(j)) p->tot += j.L;
  }
  if (!p->tot) return 0;
  p->d_ext = (Ext*)ws_get(ctx, Ws::MultiExt, p->tot * sizeof(Ext) + 64);
  p->d_out = (uint8_t*)ws_get(ctx, Ws::MultiOut, 32 * p->tot + 64);
  if (!p->d_ext || !p->d_out) return set_err(ctx, SPG_E_NOMEM, "commit rows");
  size_t o = 0;
  for (const RowJob& j : jobs) {
    if (!rows_merged(j)) continue;
    bool h = false;
    const int rc = rows_to_points(ctx, g, j.d_Z, j.R, j.L, p->d_ext + o, &h, p->tot >= kHalvedMin);
    if (rc) return rc;
    p->hv.push_back(h);
    o += j.L;
  }
  return 0;
}

int commit_rows_many_finish(spg_ctx* ctx, ProverGens& g, const std::vector<RowJob>& jobs, RowsPending& p) {
  if (p.tot) {  // the encodings of each run of merged jobs with the same form (halved comb points or not)
    std::vector<Pt> rows(p.tot);
    size_t k = 0, a = 0, o = 0;
    for (const RowJob& j : jobs) {
      if (!rows_merged(j)) continue;
      o += j.L;
      k++;
      if (k == p.hv.size() || p.hv[k] != p.hv[k - 1]) {  // the run [a, o) ends here
        const int rc = encode_points(ctx, p.d_ext + a, o - a, rows.data() + a, p.d_out + 32 * a, p.hv[k - 1] != 0);
        if (rc) return rc;
        a = o;
      }
    }
    o = 0;
    for (const RowJob& j : jobs) {
      if (!rows_merged(j)) continue;
      std::copy(rows.begin() + o, rows.begin() + o + j.L, j.out);
      o += j.L;
    }
  }
  for (const RowJob& j : jobs) {
    if (rows_merged(j)) continue;
    int rc = commit_rows(ctx, g, j.d_Z, j.R, j.L, j.out);
    if (rc) return rc;
  }
  return 0;
}

int commit_rows_many(spg_ctx* ctx, ProverGens& g, const std::vector<RowJob>& jobs) {
  RowsPending p;
  const int rc = commit_rows_many_launch(ctx, g, jobs, &p);
  return rc ? rc : commit_rows_many_finish(ctx, g, jobs, p);
}

// Hyrax rows split over the ranks of sh (SURVEY 8e "Hyrax commits: rows per GPU, allgather of the 32-byte
// rows"): rank r commits rows [b(r), b(r+1)) of the balanced split, then every rank receives all L encodings
int commit_rows_sh(spg_ctx* ctx, ProverGens& g, const Fq* d_Z, size_t R, size_t L, Pt* out, const Shard& sh) {
  if (sh.n == 1) return commit_rows(ctx, g, d_Z, R, L, out);
  const size_t r0 = shard_begin(L, sh.n, sh.rank), r1 = shard_begin(L, sh.n, sh.rank + 1);
  const size_t per = (L + sh.n - 1) / sh.n;  // slots per rank in the gather
  std::vector<Pt> mine(per);
  int rc = r1 > r0 ? commit_rows(ctx, g, d_Z + r0 * R, R, r1 - r0, mine.data()) : 0;
  std::vector<uint8_t> all;
  rc = comm_allgather(ctx, sh, rc, mine.data(), per * sizeof(Pt), all);
  if (rc) return rc;
  for (int q = 0; q < sh.n; q++) {
    const size_t b0 = shard_begin(L, sh.n, q), b1 = shard_begin(L, sh.n, q + 1);
    memcpy(out + b0, all.data() + (size_t)q * per * sizeof(Pt), (b1 - b0) * sizeof(Pt));
  }
  return 0;
}

// DensePolynomial::commit without blinds (dense_mlpoly.rs:184-256) of 2^nv device scalars: L = 2^(nv/2)
// rows of R = 2^(nv - nv/2) scalars against the first R generators
int commit_dev(spg_ctx* ctx, ProverGens& g, const Fq* d_Z, size_t nv, std::vector<Pt>* out, const Shard& sh) {
  size_t L = (size_t)1 << (nv / 2), R = (size_t)1 << (nv - nv / 2);
  out->resize(L);
  return commit_rows_sh(ctx, g, d_Z, R, L, out->data(), sh);
}

void append_polycomm(Tr& t, const char* label, const std::vector<Pt>& c) {
  t.msg(label, "poly_commitment_begin");
  for (auto& p : c) t.point("poly_commitment_share", p);
  t.msg(label, "poly_commitment_end");
}

// PolyEvalProof::prove without blinds (dense_mlpoly.rs:437-490) of a device polynomial of 2^|r| scalars.
// Sharded (sh.n > 1): rank r binds its balanced share of the Ls rows, the partial L.Z vectors are summed over the
// ranks, and every rank runs the same (replicated) Bullet rounds.
int poly_eval_prove(spg_ctx* ctx, ProverGens& g, const Fq* d_Z, const FqV& r, const Fq& Zr, Tr& t, Tape& tape,
                    DotProductProofLogP* out, const Shard& sh) {
  t.protocol("polynomial evaluation proof");
  size_t nv = r.size(), ln = nv / 2;
  FqV rl(r.begin(), r.begin() + ln), rr(r.begin() + ln, r.end());
  size_t Ls = (size_t)1 << ln, Rs = (size_t)1 << (nv - ln);
  if (Rs > g.n_pc) return set_err(ctx, SPG_E_ARG, "poly eval: polynomial wider than the generators");
  FqV R = eq_evals_host(rr);
  const size_t j0 = shard_begin(Ls, sh.n, sh.rank), j1 = shard_begin(Ls, sh.n, sh.rank + 1), Lm = j1 - j0;
  FqV LZ(Rs, fq_zero());
  int rc = 0;
  if (Lm) {
    size_t S = std::min<size_t>(Lm, std::max<size_t>(1, 8192 / nblk(Rs)));  // row splits to fill the chip
    size_t chunk = (Lm + S - 1) / S;
    S = (Lm + chunk - 1) / chunk;
    Fq* dL = (Fq*)ws_get(ctx, Ws::BoundL, Ls * sizeof(Fq) + 64);
    Fq* dpart = (Fq*)ws_get(ctx, Ws::BoundPart, S * Rs * sizeof(Fq) + 64);
    Fq* dout = (Fq*)ws_get(ctx, Ws::Bound, Rs * sizeof(Fq) + 64);
    if (!dL || !dpart || !dout) rc = set_err(ctx, SPG_E_NOMEM, "poly_eval_prove");
    if (!rc) rc = eq_table(ctx, rl, dL);
    if (!rc) {
      KScope ks(ctx, "spark_bound", 32.0 * (double)Lm * Rs + 64.0 * S * Rs);
      hipLaunchKernelGGL(k_bound_rows, dim3(nblk(Rs), (unsigned)S), dim3(256), 0, ctx->stream, d_Z + j0 * Rs, dL + j0,
                         Lm, Rs, chunk, dpart);
      hipLaunchKernelGGL(k_bound_sum, dim3((unsigned)((Rs + kBoundSumCols - 1) / kBoundSumCols)), dim3(256), 0,
                         ctx->stream, dpart, S, Rs, dout);
      if (hipGetLastError() != hipSuccess) rc = set_err(ctx, SPG_E_HIP, "poly_eval_prove launch");
    }
    if (!rc) rc = d2h_fq(ctx, dout, LZ.data(), Rs);
  }
  rc = comm_sum_fq(ctx, sh, rc, LZ.data(), Rs);
  if (rc) return rc;
  Pt cy;
  return dotproduct_log_prove(ctx, g, t, tape, LZ, fq_zero(), R, Zr, fq_zero(), out, &cy);
}

}  // namespace spg
