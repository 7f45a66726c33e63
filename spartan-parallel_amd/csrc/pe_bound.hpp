// spg — the device bound of the dense polynomial commitment seam (polyeval.hip): every L.Z vector of a call in one
// launch pair over descriptors in device memory. A header so that scripts/micro/pe_bound.hip times these very kernels.
//   k_pe_part   job (Z, L'_0 .. L'_{kt-1}): part_k[y][col] = sum_{j in row range y} L'_k[j] Z[j Rs + col]
//   k_pe_sum    out_g[col] = sum of the S_g slabs of group g
//   k_pe_sum_ragged   the univariate form: out_g[col] = sum of the slabs of those terms of group g with Rs_t > col
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "field.hpp"
#include "pe_plan.hpp"

namespace spg {

struct PeJob {  // one pass over Z feeding kt accumulators
  const Fq* Z;
  size_t offL[kPeKTMax];  // first entry of L'_k in the L buffer
  size_t offP[kPeKTMax];  // first scalar of its slabs in the partial buffer
  size_t Rs;
  uint32_t Ls, chunk, S, kt;
  uint32_t b0;         // its column blocks are [b0, next job's b0) of the grid's x range
};
struct PeSum {  // one group: S slabs of Rs scalars at offP -> Rs scalars at o
  size_t offP, o, Rs;
  uint32_t S;
  uint32_t c0;         // its column blocks (kPeSumCols columns each) start here
};

// the last descriptor whose first block is <= b (first blocks ascend, the first is 0)
template <class D, uint32_t D::*first>
__device__ __forceinline__ uint32_t pe_find(const D* __restrict__ d, uint32_t n, uint32_t b) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (d[mid].*first <= b)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(256) k_pe_part(const PeJob* __restrict__ jobs, uint32_t njobs,
                                                 const Fq* __restrict__ L, Fq* __restrict__ part, size_t part_len) {
  const PeJob& d = jobs[pe_find<PeJob, &PeJob::b0>(jobs, njobs, blockIdx.x)];
  const uint32_t y = blockIdx.y;
  if (y >= d.S) return;
  const size_t col = (size_t)(blockIdx.x - d.b0) * 256 + threadIdx.x;
  if (col >= d.Rs) return;
  const uint32_t j0 = y * d.chunk, j1 = min(d.Ls, j0 + d.chunk);
  const int kt = (int)d.kt;
  const Fq* __restrict__ z = d.Z + (size_t)j0 * d.Rs + col;
  Fq acc[kPeKTMax];
#pragma unroll
  for (int k = 0; k < kPeKTMax; k++) acc[k] = fq_zero();
  for (uint32_t j = j0; j < j1; j++, z += d.Rs) {
    const Fq zj = *z;
#pragma unroll
    for (int k = 0; k < kPeKTMax; k++)
      if (k < kt) acc[k] = fq_add(acc[k], fq_mul(L[d.offL[k] + j], zj));
  }
#pragma unroll
  for (int k = 0; k < kPeKTMax; k++)
    if (k < kt) {
      const size_t o = d.offP[k] + (size_t)y * d.Rs + col;
#ifdef SPG_CHECKED
      if (o >= part_len) {
        printf("k_pe_part: slab index %zu past %zu (job b0=%u y=%u k=%d)\n", o, part_len, d.b0, y, k);
        continue;
      }
#endif
      part[o] = acc[k];
    }
}

// a block owns kPeSumCols columns of one group and 256 / kPeSumCols lanes per column split its S slabs, then an LDS
// tree (one lane per column would be a chain of S dependent additions)
constexpr int kPeSumCols = 16;
__global__ void __launch_bounds__(256) k_pe_sum(const PeSum* __restrict__ sums, uint32_t ngroups,
                                                const Fq* __restrict__ part, Fq* __restrict__ out, size_t out_len) {
  __shared__ Fq sm[256];
  constexpr int YL = 256 / kPeSumCols;
  const PeSum& d = sums[pe_find<PeSum, &PeSum::c0>(sums, ngroups, blockIdx.x)];
  const int t = threadIdx.x, y0 = t / kPeSumCols;
  const size_t i = (size_t)(blockIdx.x - d.c0) * kPeSumCols + t % kPeSumCols;
  Fq acc = fq_zero();
  if (i < d.Rs)
    for (size_t y = y0; y < d.S; y += YL) acc = fq_add(acc, part[d.offP + y * d.Rs + i]);
  sm[t] = acc;
  __syncthreads();
#pragma unroll
  for (int h = YL / 2; h >= 1; h >>= 1) {
    if (y0 < h) sm[t] = fq_add(sm[t], sm[t + kPeSumCols * h]);
    __syncthreads();
  }
  if (y0 == 0 && i < d.Rs) {
#ifdef SPG_CHECKED
    if (d.o + i >= out_len) {
      printf("k_pe_sum: output index %zu past %zu\n", d.o + i, out_len);
      return;
    }
#endif
    out[d.o + i] = sm[t];
  }
}

// The univariate form's second stage: a group is a list of terms whose slabs have widths of their own, and output
// column col is the sum of the slabs of those terms whose Rs > col (LZ_comb[k] += c^i LZ_i[k] for k < Rs_i only,
// dense_mlpoly.rs:1109-1112). Built like k_pe_sum: a block owns kPeSumCols columns of one group; the (term, slab)
// pairs of the group, numbered through its terms, go round the 256 / kPeSumCols lanes of a column, so that a group
// of many one-slab terms is split as evenly as one term of many slabs; then the LDS tree.
struct PeRagTerm {  // S slabs of Rs scalars at offP
  size_t offP, Rs;
  uint32_t S;
};
struct PeRagSum {  // one group: terms [t0, t0 + nt) of the term list -> Rs (its widest term's) scalars at o
  size_t o, Rs;
  uint32_t t0, nt;
  uint32_t c0;  // its column blocks (kPeSumCols columns each) start here
};
constexpr uint32_t kPeRagLoads = 4;  // slabs in flight per lane: 4 x 8 VGPRs beside the accumulator
__global__ void __launch_bounds__(256) k_pe_sum_ragged(const PeRagSum* __restrict__ sums, uint32_t ngroups,
                                                       const PeRagTerm* __restrict__ terms,
                                                       const Fq* __restrict__ part, size_t part_len,
                                                       Fq* __restrict__ out, size_t out_len) {
  __shared__ Fq sm[256];
  constexpr uint32_t YL = 256 / kPeSumCols;
  const PeRagSum& d = sums[pe_find<PeRagSum, &PeRagSum::c0>(sums, ngroups, blockIdx.x)];
  const int t = threadIdx.x;
  const uint32_t y0 = (uint32_t)t / kPeSumCols;
  const size_t i = (size_t)(blockIdx.x - d.c0) * kPeSumCols + t % kPeSumCols;
  Fq acc = fq_zero();
  uint32_t pairs = 0;  // (term, slab) pairs of the terms before k: pair p belongs to lane p % YL
  for (uint32_t k = 0; k < d.nt; k++) {
    const PeRagTerm& e = terms[d.t0 + k];
    if (i < e.Rs)
      // kPeRagLoads of a lane's slabs are loaded before any is added: a lane of the one wide group walks all its
      // terms, and a load per addition makes that walk a chain of memory latencies
      for (uint32_t y = (y0 + YL - pairs % YL) % YL; y < e.S; y += kPeRagLoads * YL) {
        Fq v[kPeRagLoads];
#pragma unroll
        for (uint32_t u = 0; u < kPeRagLoads; u++) {
          const uint32_t yu = y + u * YL;
          const size_t p = e.offP + (size_t)yu * e.Rs + i;
          bool in = yu < e.S;
#ifdef SPG_CHECKED
          if (in && p >= part_len) {
            printf("k_pe_sum_ragged: slab index %zu past %zu (term %u y=%u)\n", p, part_len, d.t0 + k, yu);
            in = false;
          }
#endif
          v[u] = in ? part[p] : fq_zero();
        }
#pragma unroll
        for (uint32_t u = 0; u < kPeRagLoads; u++) acc = fq_add(acc, v[u]);
      }
    pairs += e.S;
  }
  sm[t] = acc;
  __syncthreads();
#pragma unroll
  for (int h = YL / 2; h >= 1; h >>= 1) {
    if (y0 < (uint32_t)h) sm[t] = fq_add(sm[t], sm[t + kPeSumCols * h]);
    __syncthreads();
  }
  if (y0 == 0 && i < d.Rs) {
#ifdef SPG_CHECKED
    if (d.o + i >= out_len) {
      printf("k_pe_sum_ragged: output index %zu past %zu\n", d.o + i, out_len);
      return;
    }
#endif
    out[d.o + i] = sm[t];
  }
}

}  // namespace spg
