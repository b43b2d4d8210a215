// Last step of the per-channel statistics that the convolution epilogues and norm.hip accumulate per block.  The kernel is
// `static __global__`: every unit that includes this header carries a copy, so only the units that launch it
// (conv_bf.hip, conv_up2.hip, firstlayer.hip, norm.hip) include it.
#pragma once
#include "common.h"

namespace kmh_stats {
// partial (N, nblk, C, 2) doubles -> out (N, C, 2): one wave per output element, lanes stride over the partial
// blocks (4 independent loads in flight each), then a fixed-order wave reduction -- deterministic, and a ~64x
// shorter dependency chain than one thread.  Launch: grid (ceil(2C / 4), N), 256 threads.
__global__ __launch_bounds__(256) static void final_kernel(const double* __restrict__ partial, int nblk, int C,
                                                           double* __restrict__ out,
                                                           const int* __restrict__ only_if = nullptr) {
  if (only_if && *only_if == 0) return;        // device-side gate of a fallback path (no host synchronisation)
  const int n = blockIdx.y;
  const int e = blockIdx.x * (256 / kWave) + (threadIdx.x >> 6);
  if (e >= C * 2) return;
  const int lane = threadIdx.x & 63;
  const double* p = partial + (long long)n * nblk * C * 2 + e;
  double s4[4] = {0, 0, 0, 0};
  int b = lane;
  for (; b + 3 * kWave < nblk; b += 4 * kWave) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s4[k] += p[(long long)(b + k * kWave) * C * 2];
  }
  for (; b < nblk; b += kWave) s4[0] += p[(long long)b * C * 2];
  const double s = wave_sum((s4[0] + s4[1]) + (s4[2] + s4[3]));
  if (lane == 0) out[(long long)n * C * 2 + e] = s;
}
}  // namespace kmh_stats
