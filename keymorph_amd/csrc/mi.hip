// Mutual information of two volumes through a Parzen-window joint histogram (Mattes et al.), with its gradient.
//
// a, b: (N, V) float32, each sample on its own.  B bins (8 <= B <= 64).  Per sample and image x: lo, hi = its minimum and
// maximum (or the caller's range), s = (B - 3) / (hi - lo), s = 0 if hi == lo.  Bin coordinate u = (x - lo) s + 1, clamped to
// [1, B - 2] (only a caller-given range can be left, beyond rounding; the clamp is not differentiated: the gradient below is
// evaluated at the clamped coordinate).  Window: the cubic B-spline b3 on the four taps k0 .. k0 + 3,
// k0 = min(floor(u) - 1, B - 4), t = u - (k0 + 1) in [0, 1]:
//   w  = ((1 - t)^3, 3 t^3 - 6 t^2 + 4, -3 t^3 + 3 t^2 + 3 t + 1, t^3) / 6
//   w' = (-(1 - t)^2 / 2, 3 t^2 / 2 - 2 t, -3 t^2 / 2 + t + 1 / 2, t^2 / 2)            (sums: 1 and 0)
// h[i][j] = sum_v w_a(v)[i] w_b(v)[j], p = h / V, pa, pb its marginals, MI = sum_{p > 0} p ln(p / (pa pb)),
// G = ln(p / (pa pb)) where p > 0, else 0, and dMI / da_v = (s_a / V) sum_ij G_ij w_a'(v)[i] w_b(v)[j] (b: symmetric).
//
// mi_range_kernel     per-sample minimum and maximum: floats mapped to unsigned keys of the same order, workgroup maximum, one
//                     integer atomic pair per workgroup (exact and independent of the order; csrc/absmax.h's structure, signed).
// mi_hist_kernel      the joint histogram in FIXED POINT.  Every product w_a[i] w_b[j] (<= 4/9) is rounded to a multiple of
//                     2^-23 (kFrac) and added with an unsigned LDS atomic to the wave's own B x B table (four copies per
//                     workgroup).  A wave adds at most kFlushVox = 1024 voxels between two flushes, so a bin holds at most
//                     1024 * rint(2^23 * 4/9) = 3 817 748 480 < 2^32.  A flush sums the four copies in 64 bits and adds the
//                     non-zero entries to the (N, B, B) global table with 64-bit integer atomics.  Integer sums do not depend
//                     on the order: two runs give the same table bit for bit.  Error: every product is off by at most 2^-24, so
//                     |h_ij - exact| <= n_ij 2^-24 with n_ij the number of voxels whose windows cover (i, j) (sum n = 16 V).
//                     Lanes that meet in a bin serialise.  A wave whose 64 voxels all share one window (the background of a
//                     masked volume, and many waves of a smooth image) sums each product over the wave and adds once; otherwise
//                     every lane adds its own.  Measured against the kernel without it: 28 % faster at 256^3, 15 %
//                     with a ball mask; slower at 128^3, where one workgroup per CU does not hide the reductions' latency.
//                     (Giving the lanes of a wave voxels V / 64 apart instead of neighbours measured the same.)
// mi_final_kernel     one workgroup per sample: marginals as exact integer sums, p, ln and the sum in fp64 in a fixed order;
//                     writes MI_n and G.  A sample with s_a = 0 or s_b = 0 (a constant image) gets MI = 0 and G = 0 exactly.
// mi_bwd_kernel       one lane per voxel: recomputes the taps, gathers the 16 entries of G from LDS, writes da and / or db.
// mi_*_masked_kernel  the histogram, finalise and backward kernels over the voxels a byte mask counts, with their number M_n in
//                     V's place.  A voxel is COUNTED iff mask[v] != 0 (mask (N, V) bytes; NULL: every voxel).  Counted voxels add
//                     their products as above, M_n replaces V in p = h / M_n and in the gradient's 1 / V, and a voxel that is
//                     not counted gets gradient 0.  M_n is a 64-bit integer on the device (cnt[n], zeroed by the launcher):
//                     never read by the host.
// Each masked kernel and its unmasked neighbour share their text (mi_hist_body, mi_finalise, mi_voxel_grads): the kernels differ
// in their parameter lists, in where the count comes from and in the mask test, so the definition above stands once.
#include "common.h"
#include "mi_taps.h"      // ranges, the window (taps), the fixed-point format, the LDS tables' flush, the workspace: shared with warp_mi.hip

namespace {
constexpr int TPB = 256;
constexpr int kWaves = TPB / kWave;

// floats -> unsigned keys of the same order (negative: all bits flipped; else the sign bit set)
__device__ __forceinline__ unsigned order_key(float x) {
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ unsigned wave_umax(unsigned v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const unsigned w = (unsigned)__shfl_xor((int)v, o, kWave);
    v = w > v ? w : v;
  }
  return v;
}

// keys[(n * 2 + img) * 2 + {0, 1}] = max key, max ~key (zero-initialised: the minimum is ~(max ~key))
__global__ __launch_bounds__(TPB) void mi_range_kernel(const float* __restrict__ a, const float* __restrict__ b, long long V,
                                                       int skip_a, int skip_b, unsigned* __restrict__ keys) {
  const int n = blockIdx.y, img = blockIdx.z;
  if (img == 0 ? skip_a : skip_b) return;
  const float* x = (img == 0 ? a : b) + (long long)n * V;
  unsigned hi = 0u, lo = 0u;
  for (long long v = (long long)blockIdx.x * TPB + threadIdx.x; v < V; v += (long long)gridDim.x * TPB) {
    const unsigned k = order_key(x[v]);
    hi = k > hi ? k : hi;
    lo = ~k > lo ? ~k : lo;
  }
  __shared__ unsigned part[kWaves][2];
  hi = wave_umax(hi);
  lo = wave_umax(lo);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    part[threadIdx.x / kWave][0] = hi;
    part[threadIdx.x / kWave][1] = lo;
  }
  __syncthreads();
  if (threadIdx.x < 2) {                                              // thread 0: the maximum, thread 1: the minimum
    unsigned m = part[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) m = part[w][threadIdx.x] > m ? part[w][threadIdx.x] : m;
    unsigned* o = keys + ((long long)n * 2 + img) * 2 + threadIdx.x;
    if (m > __hip_atomic_load(o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(o, m);
  }
}

// rng[n] = (lo_a, s_a, lo_b, s_b)
__global__ void mi_scale_kernel(const unsigned* __restrict__ keys, int N, int B, int has_a, float lo_a, float hi_a, int has_b,
                                float lo_b, float hi_b, float* __restrict__ rng) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * N) return;
  const int img = i & 1;
  float lo, hi;
  if (img == 0 ? has_a : has_b) {
    lo = img == 0 ? lo_a : lo_b;
    hi = img == 0 ? hi_a : hi_b;
  } else {
    hi = key_value(keys[i * 2]);
    lo = key_value(~keys[i * 2 + 1]);
  }
  rng[i * 2] = lo;
  rng[i * 2 + 1] = hi > lo ? (float)(B - 3) / (hi - lo) : 0.f;      // NaN compares false: s = 0
}

// The histogram kernels' body.  grid (blocks, N).  The sample's V voxels are R = ceil(V / 64) steps of 64 consecutive voxels, one
// per lane.  Workgroup blockIdx.x owns steps [blockIdx.x * per, + per), kSteps * kWaves of them per flush interval: wave w takes
// steps c + w * kSteps .. + kSteps.  LDS: kWaves tables of B * B.
// MASKED: the interval's mask bytes are loaded first; a lane that is not counted reads voxel 0 (one line for the whole wave)
// instead of its own, a step without a counted lane skips its taps and its adds, and each wave sums its ballots for the
// workgroup's count (flush_tables).
template <bool MASKED>
__device__ __forceinline__ void mi_hist_body(const float* __restrict__ a, const float* __restrict__ b,
                                             const unsigned char* __restrict__ mask, const float* __restrict__ rng, long long V,
                                             long long R, long long per, int B, unsigned long long* __restrict__ hist,
                                             unsigned long long* __restrict__ cnt) {
  extern __shared__ unsigned tab[];
  const int n = blockIdx.y, BB = B * B, lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const Range r = load_range(rng, n);
  const long long beg = per * blockIdx.x;
  long long end = beg + per;
  if (end > R) end = R;
  a += (long long)n * V;
  b += (long long)n * V;
  if (MASKED && mask) mask += (long long)n * V;
  hist += (long long)n * BB;
  if (MASKED) cnt += n;
  zero_tables<kWaves>(tab, BB);
  unsigned* mine = tab + wid * BB;
  for (long long c = beg; c < end; c += kSteps * kWaves) {
    // the interval's 2 * kSteps loads first, all in flight together (an unused slot reads voxel 0)
    float xa[kSteps], xb[kSteps];
    unsigned live = 0u;
    if constexpr (MASKED) {
#pragma unroll
      for (int it = 0; it < kSteps; ++it) {
        const long long j = c + wid * kSteps + it, v = j * kWave + lane;
        const bool in = j < end && v < V;
        const bool counted = in && (mask ? mask[in ? v : 0] != 0 : true);
        live |= (counted ? 1u : 0u) << it;
      }
    }
#pragma unroll
    for (int it = 0; it < kSteps; ++it) {
      const long long j = c + wid * kSteps + it, v = j * kWave + lane;
      const bool valid = MASKED ? (live >> it) & 1u : j < end && v < V;
      if (!MASKED) live |= (valid ? 1u : 0u) << it;
      xa[it] = a[valid ? v : 0];
      xb[it] = b[valid ? v : 0];
    }
    unsigned counted_here = 0u;                                       // wave-uniform
#pragma unroll
    for (int it = 0; it < kSteps; ++it) {
      const bool valid = (live >> it) & 1u;
      if (!__any(valid)) continue;                                    // wave-uniform
      if constexpr (MASKED) {
        counted_here += (unsigned)__popcll(__ballot(valid));
        hist_add(valid, xa[it], xb[it], r, B, lane, mine);
      } else {
        // hist_add's text, kept inline in the unmasked kernel: as a call it is rescheduled and measured slower (mi_taps.h has
        // the figures).  The masked kernel calls it: with this text it measured slower under a mask of ones (MI355X,
        // tools/bench_masked_mi.py, medians of 30 calls in ms, separate processes in the order call, inline, call, inline:
        // 128^3 0.1596 0.1599 0.1597 0.1597, 256^3 0.5768 0.5853 0.5775 0.5856; profiles/mi_dedup_kernel_identity.md).
        unsigned q[16];
        int key = -1;
        if (valid) {
          const Taps ta = taps<false>(xa[it], r.lo_a, r.s_a, B), tb = taps<false>(xb[it], r.lo_b, r.s_b, B);
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
    }
    flush_tables<kWaves, MASKED>(tab, BB, hist, counted_here, cnt);
  }
}

__global__ __launch_bounds__(TPB) void mi_hist_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                      const float* __restrict__ rng, long long V, long long R, long long per,
                                                      int B, unsigned long long* __restrict__ hist) {
  mi_hist_body<false>(a, b, nullptr, rng, V, R, per, B, hist, nullptr);
}
__global__ __launch_bounds__(TPB) void mi_hist_masked_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                             const unsigned char* __restrict__ mask,
                                                             const float* __restrict__ rng, long long V, long long R,
                                                             long long per, int B, unsigned long long* __restrict__ hist,
                                                             unsigned long long* __restrict__ cnt) {
  mi_hist_body<true>(a, b, mask, rng, V, R, per, B, hist, cnt);
}

// The finalise kernels' body: one workgroup per sample, M = the number of voxels its table `hist` counted.  A sample that
// counted nothing or has a constant image (s = 0: independent) gets MI = 0 and G = 0 exactly.
// LDS: B * B doubles (p) + 2 B doubles (pa, pb)
__device__ __forceinline__ void mi_finalise(const unsigned long long* __restrict__ hist, const float* __restrict__ rng, long long M,
                                            int B, float* __restrict__ mi, float* __restrict__ G) {
  extern __shared__ double fin[];
  __shared__ double scratch[kWaves];
  const int n = blockIdx.x, BB = B * B;
  double* pa = fin + BB;
  double* pb = pa + B;
  hist += (long long)n * BB;
  G += (long long)n * BB;
  if (M == 0 || rng[n * 4 + 1] == 0.f || rng[n * 4 + 3] == 0.f) {
    for (int e = threadIdx.x; e < BB; e += TPB) G[e] = 0.f;
    if (threadIdx.x == 0) mi[n] = 0.f;
    return;
  }
  const double unit = 1.0 / ((double)(1 << kFrac) * (double)M);
  for (int e = threadIdx.x; e < BB; e += TPB) fin[e] = (double)hist[e] * unit;
  if (threadIdx.x < 2 * B) {                                          // marginals: integer sums, exact in any order
    const int k = threadIdx.x % B, col = threadIdx.x / B;
    unsigned long long s = 0ull;
    for (int j = 0; j < B; ++j) s += col ? hist[j * B + k] : hist[k * B + j];
    (col ? pb : pa)[k] = (double)s * unit;
  }
  __syncthreads();
  double acc = 0.0;
  for (int e = threadIdx.x; e < BB; e += TPB) {
    const double p = fin[e];
    double g = 0.0;
    if (p > 0.0) {
      g = log(p / (pa[e / B] * pb[e % B]));
      acc += p * g;
    }
    G[e] = (float)g;
  }
  acc = block_sum(acc, scratch);
  if (threadIdx.x == 0) mi[n] = (float)acc;
}

__global__ __launch_bounds__(TPB) void mi_final_kernel(const unsigned long long* __restrict__ hist,
                                                       const float* __restrict__ rng, long long V, int B,
                                                       float* __restrict__ mi, float* __restrict__ G) {
  mi_finalise(hist, rng, V, B, mi, G);                                // the launcher has V >= 1
}
__global__ __launch_bounds__(TPB) void mi_final_masked_kernel(const unsigned long long* __restrict__ hist,
                                                              const float* __restrict__ rng,
                                                              const unsigned long long* __restrict__ cnt, int B,
                                                              float* __restrict__ mi, float* __restrict__ G) {
  mi_finalise(hist, rng, (long long)cnt[blockIdx.x], B, mi, G);
}

// The backward kernels' per-voxel gradient: (ga, gb) = sum_ij G_ij (w_a'[i] w_b[j], w_a[i] w_b'[j]) at the pair (xa, xb), G of the
// sample in LDS (g).  The kernels scale them by gout s / (the number of counted voxels).
__device__ __forceinline__ void mi_voxel_grads(float xa, float xb, const Range& r, int B, const float* g, float& ga, float& gb) {
  const Taps ta = taps<true>(xa, r.lo_a, r.s_a, B), tb = taps<true>(xb, r.lo_b, r.s_b, B);
  const float* row = g + ta.k0 * B + tb.k0;
  ga = 0.f;
  gb = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float rw = 0.f, rd = 0.f;                                        // sum_j G_ij w_b[j], sum_j G_ij w_b'[j]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gij = row[i * B + j];
      rw = fmaf(gij, tb.w[j], rw);
      rd = fmaf(gij, tb.d[j], rd);
    }
    ga = fmaf(ta.d[i], rw, ga);
    gb = fmaf(ta.w[i], rd, gb);
  }
}

// grid (blocks, N), four voxels per lane; LDS: G of the sample (B * B floats)
constexpr int kBwdVpt = 4;
__global__ __launch_bounds__(TPB) void mi_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                     const float* __restrict__ rng, const float* __restrict__ G,
                                                     const float* __restrict__ gout, long long V, int B,
                                                     float* __restrict__ da, float* __restrict__ db) {
  extern __shared__ float g[];
  const int n = blockIdx.y, BB = B * B;
  for (int e = threadIdx.x; e < BB; e += TPB) g[e] = G[(long long)n * BB + e];
  __syncthreads();
  const Range r = load_range(rng, n);
  const float go = gout[n] / (float)V, ca = go * r.s_a, cb = go * r.s_b;
  const long long off = (long long)n * V;
#pragma unroll
  for (int it = 0; it < kBwdVpt; ++it) {
    const long long v = ((long long)blockIdx.x * kBwdVpt + it) * TPB + threadIdx.x;
    if (v >= V) return;
    float ga, gb;
    mi_voxel_grads(a[off + v], b[off + v], r, B, g, ga, gb);
    if (da) da[off + v] = ca * ga;
    if (db) db[off + v] = cb * gb;
  }
}

// mi_bwd_kernel with 1 / M_n for 1 / V; a voxel that is not counted gets 0.  Its own prologue and loop, by measurement: as one
// body with mi_bwd_kernel (mask NULL there) this kernel came out slower.  MI355X, kmh_mi_bwd_masked under a ball mask, medians of
// 30 calls in ms, separate processes in the order two loops, one body, two loops, one body
// (profiles/mi_dedup_kernel_identity.md):  128^3 0.0123 0.0127 0.0123 0.0124   256^3 0.0484 0.0501 0.0477 0.0498
__global__ __launch_bounds__(TPB) void mi_bwd_masked_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            const unsigned char* __restrict__ mask,
                                                            const float* __restrict__ rng, const float* __restrict__ G,
                                                            const float* __restrict__ gout,
                                                            const unsigned long long* __restrict__ cnt, long long V, int B,
                                                            float* __restrict__ da, float* __restrict__ db) {
  extern __shared__ float g[];
  const int n = blockIdx.y, BB = B * B;
  for (int e = threadIdx.x; e < BB; e += TPB) g[e] = G[(long long)n * BB + e];
  __syncthreads();
  const Range r = load_range(rng, n);
  const long long M = (long long)cnt[n];
  const float go = M ? gout[n] / (float)M : 0.f, ca = go * r.s_a, cb = go * r.s_b;
  const long long off = (long long)n * V;
#pragma unroll
  for (int it = 0; it < kBwdVpt; ++it) {
    const long long v = ((long long)blockIdx.x * kBwdVpt + it) * TPB + threadIdx.x;
    if (v >= V) return;
    if (mask && mask[off + v] == 0) {
      if (da) da[off + v] = 0.f;
      if (db) db[off + v] = 0.f;
      continue;
    }
    float ga, gb;
    mi_voxel_grads(a[off + v], b[off + v], r, B, g, ga, gb);
    if (da) da[off + v] = ca * ga;
    if (db) db[off + v] = cb * gb;
  }
}

bool mi_args_ok(const void* a, const void* b, int N, long long V, int B) {
  return a && b && N >= 1 && N <= 65535 && V >= 1 && V <= (1ll << 40) && B >= kMinBins && B <= kMaxBins;
}

// The histogram pass: clears the workspace (keys and table; `cleared`: the range stage already has) and the count, then the
// kernel over hist_steps' partition.  cnt != NULL: the masked kernel.
hipError_t mi_hist_launch(const float* a, const float* b, const unsigned char* mask, const float* rng, int N, long long V,
                          int bins, void* ws, bool cleared, long long* cnt, hipStream_t s) {
  hipError_t e = cleared ? hipSuccess : hipMemsetAsync(ws, 0, ws_bytes(N, bins), s);
  if (e == hipSuccess && cnt) e = hipMemsetAsync(cnt, 0, (size_t)N * sizeof(long long), s);
  if (e != hipSuccess) return e;
  const HistSteps p = hist_steps(V, kWaves);
  const dim3 grid((unsigned)p.nb, (unsigned)N);
  const size_t lds = (size_t)kWaves * bins * bins * sizeof(unsigned);
  if (cnt)
    mi_hist_masked_kernel<<<grid, TPB, lds, s>>>(a, b, mask, rng, V, p.R, p.per, bins, ws_table(ws, N), (unsigned long long*)cnt);
  else
    mi_hist_kernel<<<grid, TPB, lds, s>>>(a, b, rng, V, p.R, p.per, bins, ws_table(ws, N));
  return hipSuccess;
}

// cnt != NULL: p = h / cnt[n], else p = h / V
void mi_final_launch(const void* ws, const float* rng, const long long* cnt, int N, long long V, int bins, float* mi, float* G,
                     hipStream_t s) {
  const size_t lds = (size_t)(bins * bins + 2 * bins) * sizeof(double);
  if (cnt)
    mi_final_masked_kernel<<<N, TPB, lds, s>>>(ws_table(ws, N), rng, (const unsigned long long*)cnt, bins, mi, G);
  else
    mi_final_kernel<<<N, TPB, lds, s>>>(ws_table(ws, N), rng, V, bins, mi, G);
}

// cnt != NULL: the masked kernel, over the voxels `mask` counts
int mi_bwd_launch(const float* a, const float* b, const unsigned char* mask, const float* rng, const float* G, const float* gout,
                  const long long* cnt, int N, long long V, int bins, float* da, float* db, hipStream_t s) {
  if (!da && !db) return 0;
  const long long nb = (V + TPB * kBwdVpt - 1) / (TPB * kBwdVpt);
  if (nb > 0x7fffffffll) return -22;
  const dim3 grid((unsigned)nb, (unsigned)N);
  const size_t lds = (size_t)bins * bins * sizeof(float);
  if (cnt)
    mi_bwd_masked_kernel<<<grid, TPB, lds, s>>>(a, b, mask, rng, G, gout, (const unsigned long long*)cnt, V, bins, da, db);
  else
    mi_bwd_kernel<<<grid, TPB, lds, s>>>(a, b, rng, G, gout, V, bins, da, db);
  return KMH_LAUNCH_CHECK();
}
}  // namespace

/* Workspace of kmh_mi_hist / kmh_mi_final: per sample four range keys and the B x B table of 64-bit sums. */
KMH_API size_t kmh_mi_ws_bytes(int N, int bins) {
  if (N < 0 || bins < 0) return 0;
  return ws_bytes(N, bins);
}

// The range stage: clears the first `clear` bytes of ws (the keys, or the keys and the table behind them), then rng (N, 4) from
// each image's own minimum and maximum or from the caller's range.
static hipError_t mi_range_launch(const float* a, const float* b, int N, long long V, int bins, int has_range_a, float lo_a,
                                  float hi_a, int has_range_b, float lo_b, float hi_b, void* ws, size_t clear, float* rng,
                                  hipStream_t s) {
  hipError_t e = hipMemsetAsync(ws, 0, clear, s);
  if (e != hipSuccess) return e;
  unsigned* keys = (unsigned*)ws;
  if (!has_range_a || !has_range_b) {
    long long nb = (V + TPB * 16 - 1) / (TPB * 16);
    if (nb > 256) nb = 256;
    mi_range_kernel<<<dim3((unsigned)nb, (unsigned)N, 2), TPB, 0, s>>>(a, b, V, has_range_a, has_range_b, keys);
  }
  mi_scale_kernel<<<ceil_div(2 * N, 64), 64, 0, s>>>(keys, N, bins, has_range_a, lo_a, hi_a, has_range_b, lo_b, hi_b, rng);
  return hipSuccess;
}

/* a, b: (N, V) float32 contiguous.  has_range_x != 0: image x uses the range (lo_x, hi_x) instead of its own minimum and maximum.
 * rng: (N, 4) floats out = (lo_a, s_a, lo_b, s_b).  ws: kmh_mi_ws_bytes(N, bins) bytes, holds the joint table for kmh_mi_final. */
KMH_API int kmh_mi_hist(const float* a, const float* b, int N, long long V, int bins, int has_range_a, float lo_a, float hi_a,
                        int has_range_b, float lo_b, float hi_b, void* ws, float* rng, void* stream) {
  if (!mi_args_ok(a, b, N, V, bins) || !ws || !rng) return -22;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = mi_range_launch(a, b, N, V, bins, has_range_a, lo_a, hi_a, has_range_b, lo_b, hi_b, ws, ws_bytes(N, bins), rng, s);
  if (e == hipSuccess) e = mi_hist_launch(a, b, nullptr, rng, N, V, bins, ws, true, nullptr, s);
  if (e != hipSuccess) return (int)e;
  return KMH_LAUNCH_CHECK();
}

/* kmh_mi_hist with the ranges GIVEN on the device: rng (N, 4) in, as kmh_mi_range or kmh_mi_hist wrote it (values outside a range
 * are taken at its ends).  For a caller that scores many warps of one pair without the host ever reading a range. */
KMH_API int kmh_mi_hist_ranges(const float* a, const float* b, const float* rng, int N, long long V, int bins, void* ws,
                               void* stream) {
  if (!mi_args_ok(a, b, N, V, bins) || !ws || !rng) return -22;
  hipError_t e = mi_hist_launch(a, b, nullptr, rng, N, V, bins, ws, false, nullptr, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  return KMH_LAUNCH_CHECK();
}

/* The ranges of kmh_mi_hist without its histogram: rng (N, 4) = (lo_a, s_a, lo_b, s_b), same kernels, same arguments.  ws: 16 N
 * bytes.  For a caller that scores many warps of one pair (csrc/warp_mi.hip): the range of a volume bounds every trilinear,
 * border-padded resampling of it. */
KMH_API int kmh_mi_range(const float* a, const float* b, int N, long long V, int bins, int has_range_a, float lo_a, float hi_a,
                         int has_range_b, float lo_b, float hi_b, void* ws, float* rng, void* stream) {
  if (!mi_args_ok(a, b, N, V, bins) || !ws || !rng) return -22;
  hipError_t e = mi_range_launch(a, b, N, V, bins, has_range_a, lo_a, hi_a, has_range_b, lo_b, hi_b, ws, (size_t)N * kKeyBytes, rng,
                                 (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  return KMH_LAUNCH_CHECK();
}

/* ws, rng as left by kmh_mi_hist for the same N, V, bins.  mi: N floats out.  G: (N, bins, bins) floats out = ln(p / (pa pb))
 * where p > 0, else 0: what kmh_mi_bwd reads. */
KMH_API int kmh_mi_final(const void* ws, const float* rng, int N, long long V, int bins, float* mi, float* G, void* stream) {
  if (!mi_args_ok(ws, rng, N, V, bins) || !mi || !G) return -22;
  mi_final_launch(ws, rng, nullptr, N, V, bins, mi, G, (hipStream_t)stream);
  return KMH_LAUNCH_CHECK();
}

/* da[n, v] = gout[n] dMI_n / da[n, v], db likewise; either may be NULL.  rng, G as written by kmh_mi_hist / kmh_mi_final. */
KMH_API int kmh_mi_bwd(const float* a, const float* b, const float* rng, const float* G, const float* gout, int N, long long V,
                       int bins, float* da, float* db, void* stream) {
  if (!mi_args_ok(a, b, N, V, bins) || !rng || !G || !gout) return -22;
  return mi_bwd_launch(a, b, nullptr, rng, G, gout, nullptr, N, V, bins, da, db, (hipStream_t)stream);
}

/* kmh_mi_hist_ranges over the counted voxels only: mask (N, V) bytes, non-zero = counted, NULL = every voxel.  cnt: N 64-bit
 * integers out, the number of counted voxels per sample (cleared here), which kmh_mi_final_masked and kmh_mi_bwd_masked read. */
KMH_API int kmh_mi_hist_masked(const float* a, const float* b, const unsigned char* mask, const float* rng, int N, long long V,
                               int bins, void* ws, long long* cnt, void* stream) {
  if (!mi_args_ok(a, b, N, V, bins) || !ws || !rng || !cnt) return -22;
  hipError_t e = mi_hist_launch(a, b, mask, rng, N, V, bins, ws, false, cnt, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  return KMH_LAUNCH_CHECK();
}

/* kmh_mi_final with p = h / cnt[n]: for the table of kmh_mi_hist_masked or kmh_warp_mi_hist_masked.  cnt[n] = 0: MI = 0, G = 0. */
KMH_API int kmh_mi_final_masked(const void* ws, const float* rng, const long long* cnt, int N, int bins, float* mi, float* G,
                                void* stream) {
  if (!mi_args_ok(ws, rng, N, 1, bins) || !cnt || !mi || !G) return -22;
  mi_final_launch(ws, rng, cnt, N, 0, bins, mi, G, (hipStream_t)stream);
  return KMH_LAUNCH_CHECK();
}

/* kmh_mi_bwd over the counted voxels, scaled by 1 / cnt[n]; a voxel that is not counted gets 0 in da and db. */
KMH_API int kmh_mi_bwd_masked(const float* a, const float* b, const unsigned char* mask, const float* rng, const float* G,
                              const float* gout, const long long* cnt, int N, long long V, int bins, float* da, float* db,
                              void* stream) {
  if (!mi_args_ok(a, b, N, V, bins) || !rng || !G || !gout || !cnt) return -22;
  return mi_bwd_launch(a, b, mask, rng, G, gout, cnt, N, V, bins, da, db, (hipStream_t)stream);
}
