// Microbenchmark: the univariate form's device bound (csrc/pe_bound.hpp, k_pe_part + k_pe_sum_ragged) on a ragged
// call, 40 polynomials of num_vars 16 and one of num_vars 20 combined into one vector of the widest R_size:
//   A  one launch pair over all 41 (pe_plan_uni)
//   B  the same 41 polynomials as 41 single-polynomial launch pairs (each its own plan), outputs side by side
//   C  the instances form's launch pair (k_pe_part + k_pe_sum) on the 40 polynomials of num_vars 16 in 8 groups: the
//      shape scripts/micro/pe_bound.hip records, the yardstick (the first stage is the same kernel)
// Runs alternate (A B C A B C ..); A's output is compared with the ragged sum of B's on the host. Times are device
// times between HIP events; GB/s = modelled bytes (Z once, partials written and read) over time.
// hipcc -O3 -std=c++17 --offload-arch=gfx950 -o pe_bound_ragged pe_bound_ragged.hip
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

struct Rag {  // a univariate plan's launch pair, as polyeval.hip's pe_bound_ragged builds it
  PeJob* dj = nullptr;
  PeRagSum* ds = nullptr;
  PeRagTerm* dt = nullptr;
  unsigned X = 0, Smax = 1, C = 0, njobs = 0, nsums = 0;
  size_t part_len = 0, out_len = 0;
  double bytes = 0;
};
// Z[i]: polynomial i; offL[i]: first entry of its L table in the shared L buffer
static Rag make_rag(const PeUniPlan& plan, const std::vector<const Fq*>& Z, const std::vector<size_t>& offL) {
  Rag n;
  const size_t N = plan.terms.size();
  std::vector<PeJob> jobs(N);
  std::vector<PeRagTerm> terms(N);
  std::vector<PeRagSum> sums;
  for (size_t i = 0; i < N; i++) {
    const PeUniTerm& t = plan.terms[i];
    PeJob& j = jobs[i];
    memset(&j, 0, sizeof(j));
    j.Z = Z[i], j.Rs = t.Rs, j.Ls = (uint32_t)t.Ls, j.chunk = (uint32_t)t.chunk, j.S = (uint32_t)t.S, j.kt = 1;
    j.offL[0] = offL[i], j.offP[0] = t.part_off, j.b0 = n.X;
    n.X += (unsigned)((t.Rs + 255) / 256);
    n.Smax = std::max(n.Smax, j.S);
    n.bytes += 32.0 * t.Ls * t.Rs;
    terms[i] = PeRagTerm{t.part_off, t.Rs, (uint32_t)t.S};
  }
  sums.push_back(PeRagSum{0, plan.R_size, 0, (uint32_t)N, 0});
  n.C = (unsigned)((plan.R_size + kPeSumCols - 1) / kPeSumCols);
  n.njobs = (unsigned)N, n.nsums = 1, n.part_len = plan.part_len, n.out_len = plan.out_len;
  n.bytes += 64.0 * plan.part_len;
  CK(hipMalloc(&n.dj, N * sizeof(PeJob)));
  CK(hipMalloc(&n.dt, N * sizeof(PeRagTerm)));
  CK(hipMalloc(&n.ds, sizeof(PeRagSum)));
  CK(hipMemcpy(n.dj, jobs.data(), N * sizeof(PeJob), hipMemcpyHostToDevice));
  CK(hipMemcpy(n.dt, terms.data(), N * sizeof(PeRagTerm), hipMemcpyHostToDevice));
  CK(hipMemcpy(n.ds, sums.data(), sizeof(PeRagSum), hipMemcpyHostToDevice));
  return n;
}
static void run_rag(const Rag& n, const Fq* L, Fq* part, Fq* out) {
  hipLaunchKernelGGL(k_pe_part, dim3(n.X, n.Smax), dim3(256), 0, 0, n.dj, n.njobs, L, part, n.part_len);
  hipLaunchKernelGGL(k_pe_sum_ragged, dim3(n.C), dim3(256), 0, 0, n.ds, n.nsums, n.dt, part, n.part_len, out, n.out_len);
}

struct Inst {  // the instances form's pair over a PePlan (every term bound), as scripts/micro/pe_bound.hip
  PeJob* dj = nullptr;
  PeSum* ds = nullptr;
  unsigned X = 0, Smax = 1, C = 0, njobs = 0, nsums = 0;
  size_t part_len = 0, out_len = 0;
  double bytes = 0;
};
static Inst make_inst(const PePlan& plan, const std::vector<const Fq*>& Z, const std::vector<size_t>& offL) {
  Inst n;
  std::vector<PeJob> jobs;
  std::vector<PeSum> sums;
  for (size_t i = 0; i < plan.terms.size(); i++) {
    const PeTerm& t = plan.terms[i];
    const PeGroup& g = plan.groups[t.group];
    PeJob j;
    memset(&j, 0, sizeof(j));
    j.Z = Z[i], j.Rs = g.Rs, j.Ls = (uint32_t)g.Ls, j.chunk = (uint32_t)t.chunk, j.S = (uint32_t)t.S, j.kt = 1;
    j.offL[0] = offL[i], j.offP[0] = g.part_off + t.slab * g.Rs, j.b0 = n.X;
    n.X += (unsigned)((g.Rs + 255) / 256);
    n.Smax = std::max(n.Smax, j.S);
    n.bytes += 32.0 * g.Ls * g.Rs;
    jobs.push_back(j);
  }
  for (const PeGroup& g : plan.groups) {
    sums.push_back(PeSum{g.part_off, g.out_off, g.Rs, (uint32_t)g.S, n.C});
    n.C += (unsigned)((g.Rs + kPeSumCols - 1) / kPeSumCols);
  }
  n.njobs = (unsigned)jobs.size(), n.nsums = (unsigned)sums.size(), n.part_len = plan.part_len, n.out_len = plan.out_len;
  n.bytes += 64.0 * plan.part_len;
  CK(hipMalloc(&n.dj, jobs.size() * sizeof(PeJob)));
  CK(hipMalloc(&n.ds, sums.size() * sizeof(PeSum)));
  CK(hipMemcpy(n.dj, jobs.data(), jobs.size() * sizeof(PeJob), hipMemcpyHostToDevice));
  CK(hipMemcpy(n.ds, sums.data(), sums.size() * sizeof(PeSum), hipMemcpyHostToDevice));
  return n;
}
static void run_inst(const Inst& n, const Fq* L, Fq* part, Fq* out) {
  hipLaunchKernelGGL(k_pe_part, dim3(n.X, n.Smax), dim3(256), 0, 0, n.dj, n.njobs, L, part, n.part_len);
  hipLaunchKernelGGL(k_pe_sum, dim3(n.C), dim3(256), 0, 0, n.ds, n.nsums, part, out, n.out_len);
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
static void report(const char* name, std::vector<float> t, double bytes) {
  std::sort(t.begin(), t.end());
  const double m = t[t.size() / 2];
  printf("  %-44s median %8.3f ms (min %.3f, max %.3f)  %7.1f MB modelled  %7.1f GB/s\n", name, m, t.front(), t.back(),
         bytes / 1e6, bytes / (m * 1e-3) / 1e9);
}

int main() {
  const int reps = 15;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const size_t n = 41, G = 8;
  std::vector<size_t> nvs(40, 16);
  nvs.push_back(20);
  std::vector<size_t> offZ(n), offL(n), Ls(n), Rs(n);
  size_t totZ = 0, totL = 0;
  for (size_t i = 0; i < n; i++) {
    Ls[i] = (size_t)1 << (nvs[i] / 2), Rs[i] = (size_t)1 << (nvs[i] - nvs[i] / 2);
    offZ[i] = totZ, offL[i] = totL;
    totZ += (size_t)1 << nvs[i], totL += Ls[i];
  }
  Fq *Z, *L, *part, *out_one, *out_each, *out_inst;
  CK(hipMalloc(&Z, totZ * sizeof(Fq)));
  CK(hipMalloc(&L, totL * sizeof(Fq)));
  hipLaunchKernelGGL(k_fill, dim3((unsigned)((totZ + 255) / 256)), dim3(256), 0, 0, Z, totZ, 3u);
  hipLaunchKernelGGL(k_fill, dim3((unsigned)((totL + 255) / 256)), dim3(256), 0, 0, L, totL, 4u);
  std::vector<const Fq*> Zs(n);
  for (size_t i = 0; i < n; i++) Zs[i] = Z + offZ[i];

  // A: one call
  const PeUniPlan plan = pe_plan_uni(nvs.data(), n, false);
  const Rag one = make_rag(plan, Zs, offL);
  // B: 41 calls, each polynomial alone
  std::vector<Rag> each;
  std::vector<size_t> each_out(n);
  size_t each_len = 0, part_max = plan.part_len;
  double each_bytes = 0;
  for (size_t i = 0; i < n; i++) {
    const PeUniPlan p1 = pe_plan_uni(&nvs[i], 1, false);
    each.push_back(make_rag(p1, {Zs[i]}, {offL[i]}));
    each_out[i] = each_len;
    each_len += Rs[i];
    part_max = std::max(part_max, p1.part_len);
    each_bytes += each.back().bytes;
  }
  // C: the instances form on the 40 polynomials of num_vars 16, G right halves
  const size_t nv = 16, m = 40;
  std::vector<Fq> r(m * nv, fq_from_u64(5));
  std::vector<size_t> nv40(m, nv), lens(m, nv);
  for (size_t i = 0; i < m; i++) r[i * nv] = fq_from_u64(100 + i), r[i * nv + nv - 1] = fq_from_u64(7 + i % G);
  const PePlan iplan = pe_plan_instances(nv40.data(), r.data(), lens.data(), m);
  const Inst inst = make_inst(iplan, std::vector<const Fq*>(Zs.begin(), Zs.begin() + m),
                              std::vector<size_t>(offL.begin(), offL.begin() + m));
  part_max = std::max(part_max, iplan.part_len);

  CK(hipMalloc(&part, part_max * sizeof(Fq)));
  CK(hipMalloc(&out_one, plan.out_len * sizeof(Fq)));
  CK(hipMalloc(&out_each, each_len * sizeof(Fq)));
  CK(hipMalloc(&out_inst, iplan.out_len * sizeof(Fq)));
  std::vector<float> ta, tb, tc, ta1, ta2, tc1, tc2;
  for (int i = 0; i <= reps; i++) {  // the first round warms up
    const float a = timed(e0, e1, [&] { run_rag(one, L, part, out_one); });
    const float b = timed(e0, e1, [&] {
      for (size_t k = 0; k < n; k++) run_rag(each[k], L, part, out_each + each_out[k]);
    });
    const float c = timed(e0, e1, [&] { run_inst(inst, L, part, out_inst); });
    // the two stages of A and of C alone (the partials of the first are still in place for the second)
    const float a1 = timed(e0, e1, [&] {
      hipLaunchKernelGGL(k_pe_part, dim3(one.X, one.Smax), dim3(256), 0, 0, one.dj, one.njobs, L, part, one.part_len);
    });
    const float a2 = timed(e0, e1, [&] {
      hipLaunchKernelGGL(k_pe_sum_ragged, dim3(one.C), dim3(256), 0, 0, one.ds, one.nsums, one.dt, part, one.part_len,
                         out_one, one.out_len);
    });
    const float c1 = timed(e0, e1, [&] {
      hipLaunchKernelGGL(k_pe_part, dim3(inst.X, inst.Smax), dim3(256), 0, 0, inst.dj, inst.njobs, L, part,
                         inst.part_len);
    });
    const float c2 = timed(e0, e1, [&] {
      hipLaunchKernelGGL(k_pe_sum, dim3(inst.C), dim3(256), 0, 0, inst.ds, inst.nsums, part, out_inst, inst.out_len);
    });
    if (i) {
      ta.push_back(a), tb.push_back(b), tc.push_back(c);
      ta1.push_back(a1), ta2.push_back(a2), tc1.push_back(c1), tc2.push_back(c2);
    }
  }
  printf("univariate form: 40 polynomials of num_vars 16 and one of num_vars 20, R_size %zu\n", plan.R_size);
  printf("  one call: %u column blocks x %u row ranges (num_vars 16: S = %zu of %zu rows; 20: S = %zu of %zu rows), "
         "%u sum blocks over %zu (term, slab) pairs\n",
         one.X, one.Smax, plan.terms[0].S, plan.terms[0].chunk, plan.terms[40].S, plan.terms[40].chunk, one.C,
         40 * plan.terms[0].S + plan.terms[40].S);
  report("A one launch pair, 41 polynomials", ta, one.bytes);
  report("B 41 x (k_pe_part + k_pe_sum_ragged)", tb, each_bytes);
  report("C instances form, 40 x num_vars 16, one pair", tc, inst.bytes);
  report("A stage 1 alone (k_pe_part)", ta1, one.bytes - 32.0 * plan.part_len);
  report("A stage 2 alone (k_pe_sum_ragged)", ta2, 32.0 * plan.part_len);
  report("C stage 1 alone (k_pe_part)", tc1, inst.bytes - 32.0 * iplan.part_len);
  report("C stage 2 alone (k_pe_sum)", tc2, 32.0 * iplan.part_len);
  // A against the ragged sum of B's outputs
  std::vector<Fq> ha(plan.out_len), hb(each_len), hs(plan.out_len, fq_zero());
  CK(hipMemcpy(ha.data(), out_one, plan.out_len * sizeof(Fq), hipMemcpyDeviceToHost));
  CK(hipMemcpy(hb.data(), out_each, each_len * sizeof(Fq), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; i++)
    for (size_t c = 0; c < Rs[i]; c++) hs[c] = fq_add(hs[c], hb[each_out[i] + c]);
  const bool ok = memcmp(hs.data(), ha.data(), plan.out_len * sizeof(Fq)) == 0;
  printf("  outputs equal: %d\n", ok);
  return ok ? 0 : 1;
}
