// Absolute maximum of a tensor -> the {S, 1/S} range scale of the split-operand kernels (common.h: range_scale).  Its two
// kernels are `static __global__`: every unit that includes this header carries a copy, so only the units that launch them
// (headcom.hip, norm.hip) include it.
#pragma once
#include "common.h"

namespace kmh_absmax {
// wave maximum -> one atomic per wave, and only when it would raise the published value: thousands of same-address
// atomics serialise in L2 (~2.5 ns each), a plain load of the current maximum does not
__device__ __forceinline__ void publish(float m, unsigned* acc) {
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) {
    const unsigned bits = __float_as_uint(m);
    if (bits > __hip_atomic_load(acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(acc, bits);
  }
}
__global__ __launch_bounds__(256) static void partial_kernel(const float* __restrict__ x, long long n,
                                                             unsigned* __restrict__ acc) {
  float m = 0.f;
  // scalar head up to the first 16-byte boundary (parameters inside a flat bucket are only 4-byte aligned),
  // float4 body, scalar tail
  long long head = (long long)(((16 - (reinterpret_cast<unsigned long long>(x) & 15)) & 15) >> 2);
  if (head > n) head = n;
  const float* xb = x + head;
  const long long nb = n - head, n4 = nb >> 2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(xb)[i];
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  if (blockIdx.x == 0) {
    for (long long i = threadIdx.x; i < head; i += 256) m = fmaxf(m, fabsf(x[i]));
    for (long long i = (n4 << 2) + threadIdx.x; i < nb; i += 256) m = fmaxf(m, fabsf(xb[i]));
  }
  // non-negative floats order like their bit patterns: an integer max is exact and order independent
  publish(m, acc);
}
__global__ static void final_kernel(float* __restrict__ out2, float min_abs) {
  const float m = fmaxf(__uint_as_float(reinterpret_cast<unsigned*>(out2)[0]), min_abs);
  range_scale(m, out2);
}
// out2[2] = {S, 1/S} for m = max(max|x|, min_abs), m S in [2^14, 2^15) (fmaxf drops a NaN; an infinite m gives S = 1);
// everything on `s`, no host sync
static inline int launch(const float* x, long long n, float min_abs, float* out2, hipStream_t s) {
  hipError_t e = hipMemsetAsync(out2, 0, 2 * sizeof(float), s);
  if (e != hipSuccess) return (int)e;
  long long nb = (n / 4 + 256) / 256;
  if (nb > 2048) nb = 2048;
  partial_kernel<<<(int)nb, 256, 0, s>>>(x, n, reinterpret_cast<unsigned*>(out2));
  final_kernel<<<1, 1, 0, s>>>(out2, min_abs);
  return (int)hipGetLastError();
}
}  // namespace kmh_absmax
