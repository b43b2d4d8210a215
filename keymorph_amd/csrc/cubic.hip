// Cubic B-spline resampling: the prefilter that turns a volume into B-spline coefficients, and the 64-tap sampler of those
// coefficients with its gradient with respect to the grid.  The interpolant of the image a user keeps (elastix's
// FinalBSplineInterpolationOrder = 3); the fitting loops stay on the trilinear sampler of sampler.hip.
//
// Definition (tests/cubic_ref.py restates it in fp64; scipy.ndimage.spline_filter / map_coordinates with mode="mirror" agree):
//   coefficients  c = prefilter(x), separably along W, H, D:  sum_k c[k] B3(i - k) = x[i] at every integer i, c continued past the
//                 ends by whole-sample mirror (-1 -> 1, n -> n - 2, period 2 (n - 1)); an axis of length 1 is left alone.
//                 Per line, z = sqrt(3) - 2:   c+[0] = sum_{k < 2n-2} z^k x[fold(k)] / (1 - z^(2n-2)),  c+[i] = x[i] + z c+[i-1],
//                 c-[n-1] = z / (z^2 - 1) (c+[n-1] + z c+[n-2]),  c-[i] = z (c-[i+1] - c+[i]),  c = 6 c-.
//   coordinate    unnorm_clip of sampler_taps.h, unchanged: the trilinear sampler's cell, clamp mask and NaN rule.
//   value         i0 = floor(p), t = p - i0 per axis; sum over the taps i0 - 1 .. i0 + 2 of wz wy wx c[fold(.)], fold the mirror
//                 above (everything -> 0 on an axis of length 1), so every tap address lies inside the volume.
//   grid gradient the same sum with the derivative weights on one axis, times the cotangent, summed over the channels, times
//                 unnorm_clip's multiplier (size / 2, or 0 where clamped; all three 0 for a voxel with a NaN coordinate).
// The interpolant overshoots (data in [0, 1] can leave [0, 1]) and is not clamped.  No gradient with respect to the volume.
//
// Prefilter: the recursive form, not a truncated FIR -- two multiply-adds per sample and axis whatever the accuracy asked for,
// where an FIR of the same 2^-24 truncation needs 25 taps.  The recursion's state lives in fp64 registers (one fma per sample),
// so what a pass adds to the data's own rounding is the fp32 store of c+ and of c.
// The initial sum stops after kHorizon = 20 terms: |z|^20 = 3.6e-12, under half an ulp of fp32 (6e-8) by four orders of magnitude;
// a line with 2n - 2 <= 20 takes the full periodic sum with its 1 / (1 - z^(2n-2)).
//   z and y passes: one line per lane, lanes along x (z pass: along the whole H * W plane), every load and store coalesced;
//       16 B per voxel (x in, c+ out, c+ back in and c out), against the floor of 8.
//   x pass: a lane per contiguous line would stride by W; instead a workgroup stages a tile of R consecutive rows (one contiguous
//       span of memory, copied coalesced) in LDS with an ODD pitch, so that the R lanes that run the recursions -- lane r on row
//       r, addresses pitch apart -- hit R different banks; then the tile goes back coalesced: 8 B per voxel.  Rows too long for
//       16 of them to fit the tile (W >= 768) take the line-per-lane kernel with stride 1.
// Lines are independent: no atomics, nothing between workgroups, no waiting loops, every loop bounded by an axis length
// or by kHorizon.
//
// Sampler: the lane-contiguous chunks and LDS-staged grid rows of sampler_taps.h.  The 64 taps are 16 rows (z, y folded) of 4
// consecutive x coefficients: away from the x borders (1 <= x0 <= W - 3) a row is ONE 4-byte-aligned 16-byte buffer load; a voxel
// whose span folds loads its row's four taps one by one at the folded columns instead.  The two arms sit under one branch on
// the lane's own x0, so a wave without a border voxel never executes the folded arm, and both feed the same fma chain:
// x innermost, then y, then z, each an explicit chain -- interior, border and every channel round identically.
// Limits (kmh_* return -22 past them, ops refuses with ValueError before allocating): a channel plane of fewer than 2^29
// voxels (32-bit byte offsets inside a plane's buffer descriptor), N <= 65535 (gridDim.y).
#include "sampler_taps.h"

namespace {

// ------------------------------------------------------------------------------------------------------------- prefilter
constexpr int kHorizon = 20;                       // terms of the causal start: |z|^20 = 3.6e-12 (fp32 resolves 6e-8)
constexpr double kPole = -0.26794919243112270647;  // z = sqrt(3) - 2
constexpr int kBatch = 8;                          // samples whose loads are in flight together

// One line of n >= 2 samples, in place or from a source to a destination: ld(i) reads sample i of the source, cp(i) reads back
// and cs(i, v) stores sample i of the destination (sample i of the source is read before sample i of the destination is written).
template <class LD, class CP, class CS>
__device__ __forceinline__ void prefilter_line(int n, LD ld, CP cp, CS cs) {
  const int period = 2 * n - 2;
  const int kmax = period < kHorizon ? period : kHorizon;
  double zk = 1.0, s = 0.0;
  for (int k = 0; k < kmax; ++k) {                 // bounded by min(2n - 2, kHorizon)
    const int i = k < n ? k : period - k;          // whole-sample mirror
    s = fma(zk, (double)ld(i), s);
    zk *= kPole;
  }
  if (kmax == period) s /= 1.0 - zk;               // the full periodic sum of a short line
  cs(0, (float)s);
  // Both recursions take their samples kBatch at a time: the loads of a batch are issued together, ahead of its chain of fmas
  // and its stores (source and destination may be one array, so the compiler cannot move a load over a store by itself, and a
  // load per dependent step costs a memory round trip per sample).  Sample i is still read before it is written.
  double prev2 = s, prev = s;                      // c+[i-2], c+[i-1]: the fp64 state, not the fp32 values stored
  int i = 1;
  for (; i + kBatch <= n; i += kBatch) {
    float v[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) v[j] = ld(i + j);
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      prev2 = prev;
      prev = fma(kPole, prev, (double)v[j]);
      cs(i + j, (float)prev);
    }
  }
  for (; i < n; ++i) {
    prev2 = prev;
    prev = fma(kPole, prev, (double)ld(i));
    cs(i, (float)prev);
  }
  // anti-causal
  double c = (kPole / (kPole * kPole - 1.0)) * fma(kPole, prev2, prev);
  cs(n - 1, (float)(6.0 * c));
  i = n - 2;
  for (; i - kBatch + 1 >= 0; i -= kBatch) {
    float v[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) v[j] = cp(i - j);
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      c = kPole * (c - (double)v[j]);
      cs(i - j, (float)(6.0 * c));
    }
  }
  for (; i >= 0; --i) {
    c = kPole * (c - (double)cp(i));
    cs(i, (float)(6.0 * c));
  }
}

// line l of nlines: base = (l / inner) * outer + l % inner, samples `stride` apart.  z pass: inner = H W, outer = D H W,
// stride = H W; y pass: inner = W, outer = H W, stride = W; long rows of the x pass: inner = 1, outer = W, stride = 1.
__global__ __launch_bounds__(TPB) void cubic_prefilter_lines_kernel(const float* src, float* dst /* may be src */,
                                                                    long long nlines, long long inner, long long outer,
                                                                    long long stride, int n) {
  const long long l = (long long)blockIdx.x * TPB + threadIdx.x;
  if (l >= nlines) return;
  const long long q = l / inner;
  const long long base = q * outer + (l - q * inner);
  const float* s = src + base;
  float* d = dst + base;
  prefilter_line(
      n, [&](int i) { return s[i * stride]; }, [&](int i) { return d[i * stride]; },
      [&](int i, float v) { d[i * stride] = v; });
}

constexpr int kTileFloats = 12288;                 // 48 KB: three workgroups per CU
constexpr int kTileMinRows = 16;

// x pass: rows [row0, row0 + R) of length W are one contiguous span; tile row r sits at r * pitch, pitch odd
__global__ __launch_bounds__(TPB) void cubic_prefilter_rows_kernel(const float* src, float* dst /* may be src */,
                                                                   long long nrows, int W, int R, int pitch) {
  __shared__ float tile[kTileFloats];
  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * R;
  const int rows = nrows - row0 < R ? (int)(nrows - row0) : R;
  const int cnt = rows * W;                        // <= kTileFloats
  const float* s = src + row0 * W;
  float* d = dst + row0 * W;
  for (int e = tid; e < cnt; e += TPB) {
    const int r = e / W;
    tile[r * pitch + (e - r * W)] = s[e];
  }
  __syncthreads();
  if (tid < rows) {
    float* t = tile + tid * pitch;
    prefilter_line(
        W, [&](int i) { return t[i]; }, [&](int i) { return t[i]; }, [&](int i, float v) { t[i] = v; });
  }
  __syncthreads();
  for (int e = tid; e < cnt; e += TPB) {
    const int r = e / W;
    d[e] = tile[r * pitch + (e - r * W)];
  }
}

// every axis has length 1: the coefficients are the data
__global__ __launch_bounds__(TPB) void cubic_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, long long n) {
  const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// --------------------------------------------------------------------------------------------------------------- sampler
// whole-sample mirror of a tap index in [-1, n + 1] into [0, n - 1] (n = 2 needs the second reflection: 3 -> -1 -> 1)
__device__ __forceinline__ int fold(int i, int n) {
  if (n == 1) return 0;
  i = i < 0 ? -i : i;
  i = i > n - 1 ? 2 * (n - 1) - i : i;
  return i < 0 ? -i : i;
}

// B3 at the four taps i0 - 1 .. i0 + 2 for the fraction t in [0, 1), and its derivative with respect to t
__device__ __forceinline__ void bspline_w(float t, float w[4]) {
  const float a = 1.f - t;
  w[0] = a * a * a * (1.f / 6.f);
  w[1] = fmaf(t * t, fmaf(0.5f, t, -1.f), 2.f / 3.f);
  w[2] = fmaf(a * a, fmaf(0.5f, a, -1.f), 2.f / 3.f);
  w[3] = t * t * t * (1.f / 6.f);
}
__device__ __forceinline__ void bspline_dw(float t, float w[4]) {
  const float a = 1.f - t;
  w[0] = -0.5f * (a * a);
  w[1] = t * fmaf(1.5f, t, -2.f);
  w[2] = -(a * fmaf(1.5f, a, -2.f));
  w[3] = 0.5f * (t * t);
}

typedef unsigned kmh_u4 __attribute__((vector_size(16)));

struct CubicTap {
  unsigned zo[4], yo[4];   // byte offsets of the folded z planes and y rows inside a channel plane
  unsigned xo[4];          // byte offsets of the folded columns; xo[0] is the span's start when !edge
  bool edge;               // the 4-wide x span folds at a border (or W < 4): taps load one by one
  float mx, my, mz;        // d(coordinate)/d(grid) incl. the clamp mask
  float tx, ty, tz;
};

__device__ __forceinline__ CubicTap make_cubic_tap(float gx, float gy, float gz, int D, int H, int W) {
  const Tap t = make_tap(gx, gy, gz, D, H, W);
  CubicTap q;
  q.mx = t.mx; q.my = t.my; q.mz = t.mz;
  q.tx = t.fx; q.ty = t.fy; q.tz = t.fz;
  q.edge = t.x0 < 1 || t.x0 + 2 > W - 1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    q.zo[k] = 4u * (unsigned)(fold(t.z0 - 1 + k, D) * (H * W));
    q.yo[k] = 4u * (unsigned)(fold(t.y0 - 1 + k, H) * W);
    q.xo[k] = 4u * (unsigned)fold(t.x0 - 1 + k, W);
  }
  return q;
}

// the 64 taps of one channel plane, c[4 a + b][k]: plane a, row b, column k.  ONE branch for the 16 rows, so a wave without a
// border voxel issues its 16 wide loads back to back and never executes the folded arm
__device__ __forceinline__ void load_taps(__amdgpu_buffer_rsrc_t r, const CubicTap& q, float c[16][4]) {
  if (q.edge) {
#pragma unroll
    for (int ab = 0; ab < 16; ++ab) {
      const unsigned ro = q.zo[ab >> 2] + q.yo[ab & 3];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        c[ab][k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)(ro + q.xo[k]), 0, 0));
    }
  } else {
#pragma unroll
    for (int ab = 0; ab < 16; ++ab) {
      const kmh_u4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(q.zo[ab >> 2] + q.yo[ab & 3] + q.xo[0]), 0, 0);
      const unsigned u0 = v[0], u1 = v[1], u2 = v[2], u3 = v[3];      // (scalars first: sampler_taps.h, pair_b)
      c[ab][0] = __uint_as_float(u0); c[ab][1] = __uint_as_float(u1);
      c[ab][2] = __uint_as_float(u2); c[ab][3] = __uint_as_float(u3);
    }
  }
}

// THE summation order of every path: x innermost, then y, then z, each one explicit fma chain
__device__ __forceinline__ float chain4(const float c[4], const float w[4]) {
  float o = c[0] * w[0];
  o = fmaf(c[1], w[1], o);
  o = fmaf(c[2], w[2], o);
  o = fmaf(c[3], w[3], o);
  return o;
}

__device__ __forceinline__ float cubic_value(__amdgpu_buffer_rsrc_t r, const CubicTap& q, const float wx[4], const float wy[4],
                                             const float wz[4]) {
  float c[16][4];
  load_taps(r, q, c);
  float pz[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    float py[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) py[b] = chain4(c[4 * a + b], wx);
    pz[a] = chain4(py, wy);
  }
  return chain4(pz, wz);
}

// d(value)/d(ix), d(iy), d(iz): the derivative weights on one axis, the same chains
__device__ __forceinline__ void cubic_grads(__amdgpu_buffer_rsrc_t r, const CubicTap& q, const float wx[4], const float wy[4],
                                            const float wz[4], const float dwx[4], const float dwy[4], const float dwz[4],
                                            float& dx, float& dy, float& dz) {
  float c[16][4];
  load_taps(r, q, c);
  float pv[4], pdx[4], pdy[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    float rv[4], rd[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      rv[b] = chain4(c[4 * a + b], wx);
      rd[b] = chain4(c[4 * a + b], dwx);
    }
    pv[a] = chain4(rv, wy);
    pdx[a] = chain4(rd, wy);
    pdy[a] = chain4(rv, dwy);
  }
  dx = chain4(pdx, wz);
  dy = chain4(pdy, wz);
  dz = chain4(pv, dwz);
}

__global__ __launch_bounds__(TPB) void cubic_sample_fwd_kernel(const float* __restrict__ coef, const float* __restrict__ grid,
                                                               float* __restrict__ out, int C, int D, int H, int W,
                                                               long long ovox) {
  __shared__ __attribute__((aligned(16))) float sg[TPB * PASSES * 3];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
  stage_rows(grid + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
  __syncthreads();
  const long long plane = (long long)D * H * W;
  const unsigned plane_bytes = (unsigned)(plane * 4);
#pragma unroll 1
  for (int j = 0; j < PASSES; ++j) {
    const int l = tid + j * TPB;                     // lane-contiguous: voxel vb + l
    if (l >= cnt) break;                             // (whole waves leave together except in the ragged last pass)
    const CubicTap q = make_cubic_tap(sg[l * 3], sg[l * 3 + 1], sg[l * 3 + 2], D, H, W);
    float wx[4], wy[4], wz[4];
    bspline_w(q.tx, wx); bspline_w(q.ty, wy); bspline_w(q.tz, wz);
    for (int c = 0; c < C; ++c) {
      const __amdgpu_buffer_rsrc_t r = make_rsrc(coef + ((long long)n * C + c) * plane, plane_bytes);
      out[((long long)n * C + c) * ovox + vb + l] = cubic_value(r, q, wx, wy, wz);
    }
  }
}

__global__ __launch_bounds__(TPB) void cubic_sample_bwd_grid_kernel(const float* __restrict__ coef,
                                                                    const float* __restrict__ grid,
                                                                    const float* __restrict__ gout, float* __restrict__ dgrid,
                                                                    int C, int D, int H, int W, long long ovox) {
  __shared__ __attribute__((aligned(16))) float sg[TPB * PASSES * 3];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
  stage_rows(grid + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
  __syncthreads();
  const long long plane = (long long)D * H * W;
  const unsigned plane_bytes = (unsigned)(plane * 4);
  // each lane turns its own rows of sg from grid coordinates into grid gradients
#pragma unroll 1
  for (int j = 0; j < PASSES; ++j) {
    const int l = tid + j * TPB;
    if (l >= cnt) break;
    const CubicTap q = make_cubic_tap(sg[l * 3], sg[l * 3 + 1], sg[l * 3 + 2], D, H, W);
    float wx[4], wy[4], wz[4], dwx[4], dwy[4], dwz[4];
    bspline_w(q.tx, wx); bspline_w(q.ty, wy); bspline_w(q.tz, wz);
    bspline_dw(q.tx, dwx); bspline_dw(q.ty, dwy); bspline_dw(q.tz, dwz);
    float gx = 0.f, gy = 0.f, gz = 0.f;
    for (int c = 0; c < C; ++c) {
      const __amdgpu_buffer_rsrc_t r = make_rsrc(coef + ((long long)n * C + c) * plane, plane_bytes);
      const float go = gout[((long long)n * C + c) * ovox + vb + l];
      float dx, dy, dz;
      cubic_grads(r, q, wx, wy, wz, dwx, dwy, dwz, dx, dy, dz);
      gx = fmaf(dx, go, gx); gy = fmaf(dy, go, gy); gz = fmaf(dz, go, gz);
    }
    grad_row_out(sg, l, gx, gy, gz, q.mx, q.my, q.mz);
  }
  __syncthreads();
  unstage_rows(dgrid + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
}

static bool cubic_shape_ok(int N, int C, int D, int H, int W) {
  return N >= 1 && N <= 65535 && C >= 1 && D >= 1 && H >= 1 && W >= 1 && (long long)D * H * W < (1ll << 29);
}

static int launch_lines(const float* src, float* dst, long long nlines, long long inner, long long outer, long long stride,
                        int n, hipStream_t s) {
  const long long nb = (nlines + TPB - 1) / TPB;
  if (nb >= (1ll << 31)) return -22;
  cubic_prefilter_lines_kernel<<<(unsigned)nb, TPB, 0, s>>>(src, dst, nlines, inner, outer, stride, n);
  return KMH_LAUNCH_CHECK();
}

}  // namespace

KMH_API int kmh_cubic_prefilter(const float* x, float* coef, int N, int C, int D, int H, int W, void* stream) {
  if (!x || !coef || !cubic_shape_ok(N, C, D, H, W)) return -22;
  hipStream_t s = (hipStream_t)stream;
  const long long plane = (long long)D * H * W, total = (long long)N * C * plane;
  if ((total + TPB - 1) / TPB >= (1ll << 31)) return -22;
  const float* src = x;
  int rc = 0;
  if (W >= 2) {
    const long long nrows = total / W;
    const int pitch = W | 1;
    int R = kTileFloats / pitch;
    R = R > TPB ? TPB : R;
    if (R >= kTileMinRows) {
      cubic_prefilter_rows_kernel<<<(unsigned)((nrows + R - 1) / R), TPB, 0, s>>>(src, coef, nrows, W, R, pitch);
      rc = KMH_LAUNCH_CHECK();
    } else {
      rc = launch_lines(src, coef, nrows, 1, W, 1, W, s);
    }
    if (rc) return rc;
    src = coef;
  }
  if (H >= 2) {
    rc = launch_lines(src, coef, total / H, W, (long long)H * W, W, H, s);
    if (rc) return rc;
    src = coef;
  }
  if (D >= 2) {
    rc = launch_lines(src, coef, total / D, (long long)H * W, plane, (long long)H * W, D, s);
    if (rc) return rc;
    src = coef;
  }
  if (src == x) {
    cubic_copy_kernel<<<(unsigned)((total + TPB - 1) / TPB), TPB, 0, s>>>(x, coef, total);
    rc = KMH_LAUNCH_CHECK();
  }
  return rc;
}

KMH_API int kmh_cubic_sample_fwd(const float* coef, const float* grid, float* out, int N, int C, int D, int H, int W, int Do,
                                 int Ho, int Wo, void* stream) {
  if (!coef || !grid || !out || !cubic_shape_ok(N, C, D, H, W) || Do < 1 || Ho < 1 || Wo < 1) return -22;
  const long long ovox = (long long)Do * Ho * Wo;
  if ((ovox + CHUNK - 1) / CHUNK >= (1ll << 31)) return -22;
  const dim3 g((unsigned)((ovox + CHUNK - 1) / CHUNK), N);
  cubic_sample_fwd_kernel<<<g, TPB, 0, (hipStream_t)stream>>>(coef, grid, out, C, D, H, W, ovox);
  return KMH_LAUNCH_CHECK();
}

KMH_API int kmh_cubic_sample_bwd_grid(const float* coef, const float* grid, const float* gout, float* dgrid, int N, int C,
                                      int D, int H, int W, int Do, int Ho, int Wo, void* stream) {
  if (!coef || !grid || !gout || !dgrid || !cubic_shape_ok(N, C, D, H, W) || Do < 1 || Ho < 1 || Wo < 1) return -22;
  const long long ovox = (long long)Do * Ho * Wo;
  if ((ovox + CHUNK - 1) / CHUNK >= (1ll << 31)) return -22;
  const dim3 g((unsigned)((ovox + CHUNK - 1) / CHUNK), N);
  cubic_sample_bwd_grid_kernel<<<g, TPB, 0, (hipStream_t)stream>>>(coef, grid, gout, dgrid, C, D, H, W, ovox);
  return KMH_LAUNCH_CHECK();
}
