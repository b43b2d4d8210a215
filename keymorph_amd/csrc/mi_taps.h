// What both joint-histogram units need (mi.hip: two volumes in memory; warp_mi.hip: the first one sampled from a moving volume
// through a matrix on the fly): a sample's ranges (Range), the Parzen window (taps) and the constants of the fixed-point table, the
// wave's step into its LDS table (hist_add), the workgroup's LDS tables and their flush into the global table with the masked
// kernels' count (zero_tables, flush_tables), and the host side of the format: the workspace's layout (ws_bytes, ws_table) and the
// partition of a sample's voxels into steps and workgroups (hist_steps).  mi.hip states the definition; both units, masked or not,
// must produce the same integer table from the same pair of values, so these exist once.
// One exception, decided by measurement: the unmasked arm of mi.hip's histogram body keeps hist_add's text inline (its masked arm
// calls hist_add: with the text inline that arm measured slower, mi.hip has the figures).  As a call (force-inlined all the
// same) the compiler reschedules mi_hist_kernel (12530 -> 12299 instructions) and it runs slower.  MI355X, medians of 30 calls in
// ms, separate processes in the order inline, call, inline, call (profiles/metric_core_kernel_identity.md):
//   128^3  min/max pass 0.1611 0.1635 0.1622 0.1633   ranges given 0.1522 0.1535 0.1520 0.1526   masked 0.1476 0.1475 0.1478 0.1482
//   256^3  min/max pass 0.6309 0.6313 0.6304 0.6322   ranges given 0.5828 0.5842 0.5822 0.5828   masked 0.4340 0.4357 0.4340 0.4313
// The call's mean exceeds the inline mean by more than the two inline runs differ in four of the six.  warp_mi_hist_kernel's
// machine code is the same with hist_add here or in its own unit.
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

// rng[n] = (lo_a, s_a, lo_b, s_b): a sample's two ranges as mi_scale_kernel writes them
struct Range {
  float lo_a, s_a, lo_b, s_b;
};
__device__ __forceinline__ Range load_range(const float* __restrict__ rng, int n) {
  return {rng[n * 4], rng[n * 4 + 1], rng[n * 4 + 2], rng[n * 4 + 3]};
}

// One step of a wave (mi.hip's histogram body repeats this text, see above): each valid lane's pair (xa, xb) -> 16 quantised
// products added to the wave's own B x B table `mine`.  Every lane of the wave calls it together, and at least one of them is valid.
__device__ __forceinline__ void hist_add(bool valid, float xa, float xb, const Range& r, int B, int lane, unsigned* mine) {
  unsigned q[16];
  int key = -1;
  if (valid) {
    const Taps ta = taps<false>(xa, r.lo_a, r.s_a, B), tb = taps<false>(xb, r.lo_b, r.s_b, B);
    key = ta.k0 * B + tb.k0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) q[i * 4 + k] = (unsigned)__float2int_rn(ta.w[i] * tb.w[k] * (float)(1 << kFrac));
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) q[i] = 0u;
  }
  const int first = __shfl(key, __ffsll((long long)__ballot(valid)) - 1, kWave);
  if (__all(!valid || key == first)) {
    // one window for the whole wave: 64 lanes * rint(2^23 * 4/9) < 2^28 per sum
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const unsigned sum = wave_usum(q[i]);
      if (lane == 0 && sum) atomicAdd(mine + first + (i >> 2) * B + (i & 3), sum);
    }
  } else if (valid) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (q[i]) atomicAdd(mine + key + (i >> 2) * B + (i & 3), q[i]);
  }
}

// The workgroup's WAVES tables of BB bins in LDS, one per wave: cleared by all its WAVES * 64 threads before the first step.
template <int WAVES>
__device__ __forceinline__ void zero_tables(unsigned* tab, int BB) {
  for (int e = threadIdx.x; e < WAVES * BB; e += WAVES * kWave) tab[e] = 0u;
  __syncthreads();
}

// The end of a flush interval, called by the whole workgroup: the WAVES tables are summed in 64 bits and cleared, and the
// non-zero sums are added to the sample's global table `hist` with integer atomics.  MASKED: `counted` is the number of voxels
// the calling wave counted in the interval (wave-uniform); the workgroup adds their sum to *cnt with one integer atomic, and a
// workgroup that counted nothing skips the flush (its tables are still zero).
template <int WAVES, bool MASKED>
__device__ __forceinline__ void flush_tables(unsigned* tab, int BB, unsigned long long* hist, unsigned counted,
                                             unsigned long long* cnt) {
  unsigned total = 1u;
  if constexpr (MASKED) {
    __shared__ unsigned wcnt[WAVES];
    if ((threadIdx.x & (kWave - 1)) == 0) wcnt[threadIdx.x / kWave] = counted;
    __syncthreads();
    total = 0u;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) total += wcnt[w];
  } else {
    __syncthreads();
  }
  if (total) {                                                        // workgroup-uniform
    for (int e = threadIdx.x; e < BB; e += WAVES * kWave) {
      unsigned long long sum = 0ull;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        sum += tab[w * BB + e];
        tab[w * BB + e] = 0u;
      }
      if (sum) atomicAdd(hist + e, sum);
    }
    if (MASKED && threadIdx.x == 0) atomicAdd(cnt, (unsigned long long)total);
  }
  __syncthreads();
}

// The workspace of the histogram entry points: per sample four range keys (kKeyBytes), then the (N, B, B) table of 64-bit sums.
constexpr size_t kKeyBytes = 16;
inline size_t ws_bytes(int N, int bins) { return (size_t)N * kKeyBytes + (size_t)N * bins * bins * sizeof(unsigned long long); }
inline unsigned long long* ws_table(const void* ws, int N) { return (unsigned long long*)((char*)ws + (size_t)N * kKeyBytes); }

// A sample's V voxels are R steps of 64 consecutive voxels; workgroup x of nb owns steps [x * per, + per), `per` a whole number of
// flush intervals (kSteps steps for each of the workgroup's `waves` waves), about two intervals per workgroup, at most kMaxBlocks.
struct HistSteps { long long R, nb, per; };
inline HistSteps hist_steps(long long V, int waves) {
  const int chunk = kSteps * waves;                                  // steps per workgroup between two flushes
  HistSteps p;
  p.R = (V + kWave - 1) / kWave;
  p.nb = (p.R + 2 * chunk - 1) / (2 * chunk);
  if (p.nb > kMaxBlocks) p.nb = kMaxBlocks;
  p.per = (p.R + p.nb - 1) / p.nb;
  p.per = (p.per + chunk - 1) / chunk * chunk;
  p.nb = (p.R + p.per - 1) / p.per;
  return p;
}
}  // namespace
