// Microbenchmark: the planned device bound of the dense polynomial commitment seam (csrc/pe_bound.hpp, k_pe_part +
// k_pe_sum) against back-to-back passes of the single-polynomial pair every other prover path uses (k_bound_rows +
// k_bound_sum of csrc/hyrax.hip, restated here with poly_eval_prove's launch shape).
//   points    num_vars = 24, D = 4 distinct left halves over one Z: one tiled pass (kt = 4), D passes with kt = 1 of the
//             same kernels, D passes of the old pair
//   instances 40 polynomials of num_vars = 16, 8 groups: one launch pair against 40 passes of the old pair
// Runs alternate (A B C A B C ..); every variant's output is compared with the old pair's. Times are device times
// between HIP events; GB/s = modelled bytes (Z once per pass, partials written and read) over time.
// hipcc -O3 -std=c++17 --offload-arch=gfx950 -o pe_bound pe_bound.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../spartan-parallel_amd/csrc/pe_bound.hpp"

using namespace spg;

#define CK(x)                                                                      \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);  \
      exit(1);                                                                     \
    }                                                                              \
  } while (0)

// canonical scalars (< 2^252 < q) from the index
__global__ void k_fill(Fq* v, size_t n, uint32_t salt) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Fq a;
  uint32_t x = (uint32_t)i * 2654435761u + salt;
  for (int k = 0; k < 8; k++) {
    x ^= x << 13, x ^= x >> 17, x ^= x << 5;
    a.l[k] = x;
  }
  a.l[7] &= 0x0FFFFFFFu;
  v[i] = a;
}

// csrc/hyrax.hip's pair
__global__ void __launch_bounds__(256) k_bound_rows(const Fq* __restrict__ Z, const Fq* __restrict__ L, size_t Ls,
                                                    size_t Rs, size_t chunk, Fq* __restrict__ part) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Rs) return;
  size_t j0 = blockIdx.y * chunk, j1 = j0 + chunk < Ls ? j0 + chunk : Ls;
  Fq acc = fq_zero();
  for (size_t j = j0; j < j1; j++) acc = fq_add(acc, fq_mul(L[j], Z[j * Rs + i]));
  part[(size_t)blockIdx.y * Rs + i] = acc;
}
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

struct Old {  // one pass of the old pair with poly_eval_prove's split
  const Fq* Z;
  const Fq* L;
  size_t Ls, Rs;
  Fq* out;
};
static double old_bytes(const std::vector<Old>& v) {
  double b = 0;
  for (const Old& o : v) {
    const size_t nb = (o.Rs + 255) / 256, S0 = std::min(o.Ls, std::max<size_t>(1, 8192 / nb));
    const size_t chunk = (o.Ls + S0 - 1) / S0, S = (o.Ls + chunk - 1) / chunk;
    b += 32.0 * o.Ls * o.Rs + 64.0 * S * o.Rs;
  }
  return b;
}
static void run_old(const std::vector<Old>& v, Fq* part) {
  for (const Old& o : v) {
    const size_t nb = (o.Rs + 255) / 256, S0 = std::min(o.Ls, std::max<size_t>(1, 8192 / nb));
    const size_t chunk = (o.Ls + S0 - 1) / S0, S = (o.Ls + chunk - 1) / chunk;
    hipLaunchKernelGGL(k_bound_rows, dim3((unsigned)nb, (unsigned)S), dim3(256), 0, 0, o.Z, o.L, o.Ls, o.Rs, chunk, part);
    hipLaunchKernelGGL(k_bound_sum, dim3((unsigned)((o.Rs + kBoundSumCols - 1) / kBoundSumCols)), dim3(256), 0, 0, part,
                       S, o.Rs, o.out);
  }
}

struct New {  // a planned launch pair
  std::vector<PeJob> jobs;
  std::vector<PeSum> sums;
  PeJob* dj = nullptr;
  PeSum* ds = nullptr;
  unsigned X = 0, Smax = 1, C = 0;
  size_t part_len = 0, out_len = 0;
  double bytes = 0;
};
// jobs of a plan as polyeval.hip's pe_bound builds them; L vectors back to back in bound-term order, Ls entries each
static New make_new(const PePlan& plan, bool points, int kt_max, const std::vector<const Fq*>& Z) {
  New n;
  n.part_len = plan.part_len, n.out_len = plan.out_len;
  auto close = [&](PeJob& j) {
    j.b0 = n.X;
    n.X += (unsigned)((j.Rs + 255) / 256);
    n.Smax = std::max(n.Smax, j.S);
    n.bytes += 32.0 * j.Ls * j.Rs;
    n.jobs.push_back(j);
  };
  size_t offL = 0;
  if (points) {
    const size_t D = plan.groups.size();
    for (size_t p0 = 0; p0 < D; p0 += kt_max) {
      PeJob j;
      memset(&j, 0, sizeof(j));
      const PeGroup& g0 = plan.groups[p0];
      const PeTerm& t0 = plan.terms[g0.first];
      j.Z = Z[0], j.Rs = g0.Rs, j.Ls = (uint32_t)g0.Ls, j.chunk = (uint32_t)t0.chunk, j.S = (uint32_t)t0.S;
      j.kt = (uint32_t)std::min<size_t>(kt_max, D - p0);
      for (uint32_t k = 0; k < j.kt; k++, offL += g0.Ls) j.offL[k] = offL, j.offP[k] = plan.groups[p0 + k].part_off;
      close(j);
    }
  } else {
    for (size_t i = 0; i < plan.terms.size(); i++) {
      const PeTerm& t = plan.terms[i];
      const PeGroup& g = plan.groups[t.group];
      PeJob j;
      memset(&j, 0, sizeof(j));
      j.Z = Z[i], j.Rs = g.Rs, j.Ls = (uint32_t)g.Ls, j.chunk = (uint32_t)t.chunk, j.S = (uint32_t)t.S, j.kt = 1;
      j.offL[0] = offL, j.offP[0] = g.part_off + t.slab * g.Rs;
      offL += g.Ls;
      close(j);
    }
  }
  for (const PeGroup& g : plan.groups) {
    n.sums.push_back(PeSum{g.part_off, g.out_off, g.Rs, (uint32_t)g.S, n.C});
    n.C += (unsigned)((g.Rs + kPeSumCols - 1) / kPeSumCols);
  }
  n.bytes += 64.0 * plan.part_len;
  CK(hipMalloc(&n.dj, n.jobs.size() * sizeof(PeJob)));
  CK(hipMalloc(&n.ds, n.sums.size() * sizeof(PeSum)));
  CK(hipMemcpy(n.dj, n.jobs.data(), n.jobs.size() * sizeof(PeJob), hipMemcpyHostToDevice));
  CK(hipMemcpy(n.ds, n.sums.data(), n.sums.size() * sizeof(PeSum), hipMemcpyHostToDevice));
  return n;
}
static void run_new(const New& n, const Fq* L, Fq* part, Fq* out) {
  hipLaunchKernelGGL(k_pe_part, dim3(n.X, n.Smax), dim3(256), 0, 0, n.dj, (uint32_t)n.jobs.size(), L, part, n.part_len);
  hipLaunchKernelGGL(k_pe_sum, dim3(n.C), dim3(256), 0, 0, n.ds, (uint32_t)n.sums.size(), part, out, n.out_len);
}

template <class F>
static float timed(hipEvent_t e0, hipEvent_t e1, const F& f) {
  CK(hipEventRecord(e0));
  f();
  CK(hipEventRecord(e1));
  CK(hipEventSynchronize(e1));
  CK(hipGetLastError());
  float ms = 0;
  CK(hipEventElapsedTime(&ms, e0, e1));
  return ms;
}
static double median(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}
static bool same(const Fq* a, const Fq* b, size_t n) {
  std::vector<Fq> ha(n), hb(n);
  CK(hipMemcpy(ha.data(), a, n * sizeof(Fq), hipMemcpyDeviceToHost));
  CK(hipMemcpy(hb.data(), b, n * sizeof(Fq), hipMemcpyDeviceToHost));
  return memcmp(ha.data(), hb.data(), n * sizeof(Fq)) == 0;
}
static void report(const char* name, const std::vector<float>& t, double bytes) {
  float lo = *std::min_element(t.begin(), t.end()), hi = *std::max_element(t.begin(), t.end());
  const double m = median(t);
  printf("  %-34s median %8.3f ms (min %.3f, max %.3f)  %7.1f MB modelled  %7.1f GB/s\n", name, m, lo, hi, bytes / 1e6,
         bytes / (m * 1e-3) / 1e9);
}
static Fq small(uint64_t x) { return fq_from_u64(x); }

int main() {
  const int reps = 7;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  {  // ---- points form
    const size_t nv = 24, D = 4, Ls = (size_t)1 << (nv / 2), Rs = (size_t)1 << (nv - nv / 2), N = (size_t)1 << nv;
    Fq *Z, *L, *part, *out_new, *out_k1, *out_old;
    CK(hipMalloc(&Z, N * sizeof(Fq)));
    CK(hipMalloc(&L, D * Ls * sizeof(Fq)));
    hipLaunchKernelGGL(k_fill, dim3((unsigned)(N / 256)), dim3(256), 0, 0, Z, N, 1u);
    hipLaunchKernelGGL(k_fill, dim3((unsigned)(D * Ls / 256)), dim3(256), 0, 0, L, D * Ls, 2u);
    std::vector<Fq> r(D * nv, small(3));
    for (size_t i = 0; i < D; i++) r[i * nv] = small(10 + i);  // D distinct left halves
    const PePlan plan = pe_plan_points(r.data(), D, nv, 1), plan4 = pe_plan_points(r.data(), D, nv, kPeKTMax);
    New tiled = make_new(plan4, true, kPeKTMax, {Z}), k1 = make_new(plan, true, 1, {Z});
    std::vector<Old> old;
    CK(hipMalloc(&part, std::max<size_t>(std::max(plan.part_len, plan4.part_len), 8192 * 256) * sizeof(Fq)));
    CK(hipMalloc(&out_new, D * Rs * sizeof(Fq)));
    CK(hipMalloc(&out_k1, D * Rs * sizeof(Fq)));
    CK(hipMalloc(&out_old, D * Rs * sizeof(Fq)));
    for (size_t k = 0; k < D; k++) old.push_back(Old{Z, L + k * Ls, Ls, Rs, out_old + k * Rs});
    std::vector<float> ta, tb, tc;
    for (int i = 0; i <= reps; i++) {  // the first round warms up
      const float a = timed(e0, e1, [&] { run_new(tiled, L, part, out_new); });
      const float b = timed(e0, e1, [&] { run_new(k1, L, part, out_k1); });
      const float c = timed(e0, e1, [&] { run_old(old, part); });
      if (i) ta.push_back(a), tb.push_back(b), tc.push_back(c);
    }
    printf("points form: num_vars %zu, D = %zu distinct left halves (row ranges: tiled %zu of %zu rows, kt = 1 %zu of %zu)\n",
           nv, D, plan4.terms[0].S, plan4.terms[0].chunk, plan.terms[0].S, plan.terms[0].chunk);
    report("tiled (kt = 4), one launch pair", ta, tiled.bytes);
    report("kt = 1, one launch pair", tb, k1.bytes);
    report("D x (k_bound_rows + k_bound_sum)", tc, old_bytes(old));
    printf("  outputs equal: tiled %d, kt = 1 %d\n", same(out_new, out_old, D * Rs), same(out_k1, out_old, D * Rs));
    for (Fq* p : {Z, L, part, out_new, out_k1, out_old}) CK(hipFree(p));
  }
  {  // ---- instances form
    const size_t nv = 16, n = 40, G = 8, Ls = (size_t)1 << (nv / 2), Rs = (size_t)1 << (nv - nv / 2), N = (size_t)1 << nv;
    Fq *Z, *L, *part, *out_new, *out_old;
    CK(hipMalloc(&Z, n * N * sizeof(Fq)));
    CK(hipMalloc(&L, n * Ls * sizeof(Fq)));
    hipLaunchKernelGGL(k_fill, dim3((unsigned)(n * N / 256)), dim3(256), 0, 0, Z, n * N, 3u);
    hipLaunchKernelGGL(k_fill, dim3((unsigned)(n * Ls / 256)), dim3(256), 0, 0, L, n * Ls, 4u);
    std::vector<Fq> r(n * nv, small(5));
    std::vector<size_t> nvs(n, nv), lens(n, nv);
    for (size_t i = 0; i < n; i++) r[i * nv] = small(100 + i), r[i * nv + nv - 1] = small(7 + i % G);  // G right halves
    const PePlan plan = pe_plan_instances(nvs.data(), r.data(), lens.data(), n);
    std::vector<const Fq*> Zs;
    for (size_t i = 0; i < n; i++) Zs.push_back(Z + i * N);
    New one = make_new(plan, false, 1, Zs);
    CK(hipMalloc(&part, std::max<size_t>(plan.part_len, 8192 * 256) * sizeof(Fq)));
    CK(hipMalloc(&out_new, plan.out_len * sizeof(Fq)));
    CK(hipMalloc(&out_old, n * Rs * sizeof(Fq)));
    std::vector<Old> old;
    for (size_t i = 0; i < n; i++) old.push_back(Old{Zs[i], L + i * Ls, Ls, Rs, out_old + i * Rs});
    std::vector<float> ta, tb;
    for (int i = 0; i <= reps; i++) {
      const float a = timed(e0, e1, [&] { run_new(one, L, part, out_new); });
      const float b = timed(e0, e1, [&] { run_old(old, part); });
      if (i) ta.push_back(a), tb.push_back(b);
    }
    printf("instances form: %zu polynomials of num_vars %zu in %zu groups\n", n, nv, plan.groups.size());
    report("one launch pair", ta, one.bytes);
    report("40 x (k_bound_rows + k_bound_sum)", tb, old_bytes(old));
    // the group sums of the old pair's per-polynomial vectors (the host axpy the planned form has no need of)
    std::vector<Fq> ho(n * Rs), hs(plan.out_len, fq_zero()), hn(plan.out_len);
    CK(hipMemcpy(ho.data(), out_old, n * Rs * sizeof(Fq), hipMemcpyDeviceToHost));
    CK(hipMemcpy(hn.data(), out_new, plan.out_len * sizeof(Fq), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) {
      const size_t o = plan.groups[plan.terms[i].group].out_off;
      for (size_t c = 0; c < Rs; c++) hs[o + c] = fq_add(hs[o + c], ho[i * Rs + c]);
    }
    printf("  outputs equal: %d\n", memcmp(hs.data(), hn.data(), plan.out_len * sizeof(Fq)) == 0);
  }
  return 0;
}
