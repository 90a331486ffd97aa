// Reductions over the threads that share a row in the cross-entropy row kernels (ce_soft.hip, ce_hard.hip).
#pragma once
#include "common.h"

// sums / maxima over the G threads that share a row, every thread gets the result.  G == 64: butterflies.  G == 256: the four
// waves' results through LDS, added in wave order; every thread of the workgroup must call (two barriers).
template <int G, int N>
__device__ __forceinline__ void group_sum(float (&v)[N], float* lds) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = wave_sum(v[i]);
  if (G == 64) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                                     // the previous call's readers are done with lds
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < N; ++i) lds[wave * N + i] = v[i];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = (lds[i] + lds[N + i]) + (lds[2 * N + i] + lds[3 * N + i]);
}
template <int G>
__device__ __forceinline__ float group_max(float v, float* lds) {
  v = wave_max(v);
  if (G == 64) return v;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  return fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
}
