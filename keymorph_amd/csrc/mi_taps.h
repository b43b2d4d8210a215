// What both joint-histogram units need (mi.hip: two volumes in memory; warp_mi.hip: the first one sampled from a moving volume
// through a matrix on the fly): the Parzen window and the constants of the fixed-point table.  mi.hip states the definition; both
// units must produce the same integer table from the same pair of values, so the window exists once.  (The wave's step into its
// LDS table stays in each kernel's own text: mi_hist_kernel's machine code is as it was.)
#pragma once
#include "common.h"

namespace {
constexpr int kMinBins = 8, kMaxBins = 64;
constexpr int kFrac = 23;                        // fraction bits of one quantised product
constexpr int kSteps = 16;                       // steps of 64 voxels per wave between two flushes
constexpr int kFlushVox = kSteps * kWave;        // voxels per wave between two flushes
constexpr int kMaxBlocks = 2048;                 // workgroups per sample
static_assert((unsigned long long)kFlushVox * 3728271ull < (1ull << 32), "a bin of the LDS table must not overflow");

__device__ __forceinline__ unsigned wave_usum(unsigned v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, kWave);
  return v;
}

struct Taps {
  int k0;
  float w[4], d[4];
};
template <bool DERIV>
__device__ __forceinline__ Taps taps(float x, float lo, float s, int B) {
  Taps r;
  float u = (x - lo) * s + 1.f;
  u = fminf(fmaxf(u, 1.f), (float)(B - 2));                         // NaN -> 1
  int k = (int)floorf(u) - 1;
  k = k < 0 ? 0 : (k > B - 4 ? B - 4 : k);                          // any float addresses inside the table
  r.k0 = k;
  const float t = u - (float)(k + 1), o = 1.f - t, t2 = t * t, t3 = t2 * t;
  constexpr float c6 = 1.f / 6.f;
  r.w[0] = o * o * o * c6;
  r.w[1] = (3.f * t3 - 6.f * t2 + 4.f) * c6;
  r.w[2] = (-3.f * t3 + 3.f * t2 + 3.f * t + 1.f) * c6;
  r.w[3] = t3 * c6;
  if (DERIV) {
    r.d[0] = -0.5f * o * o;
    r.d[1] = 1.5f * t2 - 2.f * t;
    r.d[2] = -1.5f * t2 + t + 0.5f;
    r.d[3] = 0.5f * t2;
  }
  return r;
}
}  // namespace
