// spg — the 256-thread block sum and the segment-sum kernel that the dot products of layers.hip (dotp_evaluate) and
// spark.hip (seg_dots_multi) share.
#pragma once
#include <hip/hip_runtime.h>

#include "field.hpp"
#include "lds.hpp"

namespace spg {

__device__ __forceinline__ void block_sum3_sp(Fq& v0, Fq& v1, Fq& v2) {
  __shared__ uint32_t sh[3][soa_words<Fq, 256>()];  // component-major: no bank conflicts
  int t = threadIdx.x;
  for (int d = 128; d >= 1; d >>= 1) {
    if (t >= d && t < 2 * d) {
      soa_put<256>(sh[0], t - d, v0);
      soa_put<256>(sh[1], t - d, v1);
      soa_put<256>(sh[2], t - d, v2);
    }
    __syncthreads();
    if (t < d) {
      v0 = fq_add(v0, soa_get<256, Fq>(sh[0], t));
      v1 = fq_add(v1, soa_get<256, Fq>(sh[1], t));
      v2 = fq_add(v2, soa_get<256, Fq>(sh[2], t));
    }
    __syncthreads();
  }
  // broadcast thread 0's sums
  if (t == 0) {
    soa_put<256>(sh[0], 0, v0);
    soa_put<256>(sh[1], 0, v1);
    soa_put<256>(sh[2], 0, v2);
  }
  __syncthreads();
  v0 = soa_get<256, Fq>(sh[0], 0);
  v1 = soa_get<256, Fq>(sh[1], 0);
  v2 = soa_get<256, Fq>(sh[2], 0);
  __syncthreads();
}
// out[s] = sum of segment s's nb partials. Launched from two files, each of which compiles its own copy (no relocatable
// device code): weak, so that the host stubs link as one
__attribute__((weak)) __global__ void __launch_bounds__(256) k_sum_seg(const Fq* __restrict__ partials, int nb,
                                                                       Fq* __restrict__ out) {
  Fq a = fq_zero(), z = fq_zero(), z2 = fq_zero();
  for (int i = threadIdx.x; i < nb; i += 256) a = fq_add(a, partials[(size_t)blockIdx.x * nb + i]);
  block_sum3_sp(a, z, z2);
  if (threadIdx.x == 0) out[blockIdx.x] = a;
}

}  // namespace spg
