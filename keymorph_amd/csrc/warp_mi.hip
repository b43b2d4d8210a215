// Mutual information of a fixed volume and a moving volume warped by a 3 x 4 matrix, and its gradient with respect to the
// matrix, without the sampling grid, the warped volume or their gradients ever being stored.
//
// By definition (per sample):  warp_mi(moving, fixed, mat) = MI(align_img(affine_grid(mat, dims), moving), fixed) with both
// ranges given -- the chain kmh_affine_grid_fwd -> kmh_grid_sample3d_fwd -> kmh_mi_hist -> kmh_mi_final.  Every definition is
// that chain's own: the coordinate is grid_coords.h's (lin, affine_coord_chain: what affine_grid_fwd_kernel writes), the tap, the
// border clamp and the blend are sampler_taps.h's, and the window, the table's constants, the quantised product and the wave's
// step into its table (hist_add), the LDS tables and their flush are mi_taps.h's, which mi.hip uses too.  The joint table is an
// integer sum of the same products, so it is the chain's table bit for bit, and kmh_mi_final turns it into MI and
// G = ln(p / (pa pb)) unchanged.
//
// warp_mi_hist_kernel   mi_hist_kernel's partition (steps of 64 consecutive voxels, one per lane; kSteps steps per wave between
//                       two flushes; per-wave LDS tables; 64-bit global adds) with a = blend8 of the 8 corners of `moving` at
//                       the voxel's coordinate instead of a load.  An affine map sends the 64 neighbouring voxels of a step to
//                       neighbouring source voxels: the coherent case of the lane-contiguous gathers.  kIlp steps' gathers are
//                       in flight together.
// warp_mi_bwd_kernel    one lane per voxel recomputes coordinate, tap, corners and a, then
//                         dMI/da_v = (gout s_a / V) sum_ij G_ij w_a'[i] w_b[j]                          (mi_bwd_kernel)
//                         da_v/d(gx, gy, gz) = blend_grads * (mx, my, mz), 0 for a NaN coordinate        (grad_row_out)
//                         dM[r][k] += d(coordinate r) * (gz, gy, gx, 1)[k]                               (affine_grid_bwd_partial)
//                       fp32 per lane, the workgroup's sum in fp64, one fp64 partial per workgroup and entry.
// warp_mi_final_kernel  the partials of a sample combined in a fixed order (affine_grid_bwd_final's).
// warp_mi_*_masked_kernel  the histogram and backward kernels over the voxels that a fixed mask, a moving mask and the moving
//                       volume's extent count (stated above in_extent).
// The four histogram and backward kernels share their prologue (Range, Sample), the coordinate (voxel_tap) and mi_taps.h's
// step, tables and flush; their loops stay four texts by measurement (the figures stand above the masked histogram kernel and
// above warp_mi_bwd_kernel).
// The number of workgroups per sample depends on the volume's size alone and every sum has a fixed order: a batch reproduces
// its samples run singly and a repeat reproduces itself, bit for bit.  No float atomics.
#include "common.h"
#include "grid_coords.h"
#include "mi_taps.h"
#include "sampler_taps.h"

namespace {
constexpr int kWaves = TPB / kWave;
constexpr int kIlp = 4;                          // steps of a wave whose gathers are in flight together
constexpr int kBwdBlocks = 1024;                 // workgroups per sample of the backward pass, at most
static_assert(kSteps % kIlp == 0, "a flush interval is a whole number of gather groups");

// What every kernel here loads first for its sample n: the matrix, the base grid's steps, and `moving` as a buffer.
struct Sample {
  float M[12];
  float sz, sy, sx;
  unsigned V, plane_bytes;
  __amdgpu_buffer_rsrc_t rm;
};
__device__ __forceinline__ Sample load_sample(const float* __restrict__ moving, const float* __restrict__ mat, int n, int D, int H,
                                              int W) {
  Sample s;
  s.V = (unsigned)D * H * W;
  s.plane_bytes = s.V * 4u;
#pragma unroll
  for (int i = 0; i < 12; ++i) s.M[i] = mat[n * 12 + i];
  s.sz = lin_step(D); s.sy = lin_step(H); s.sx = lin_step(W);
  s.rm = make_rsrc(moving + (long long)n * s.V, s.plane_bytes);
  return s;
}

struct Voxel {
  Tap t;
  float gx, gy, gz;      // the sampling coordinate (x, y, z)
  float pz, py, px;      // the base grid's coordinate
};
// voxel v of the fixed lattice -> where it samples `moving`
__device__ __forceinline__ Voxel voxel_tap(unsigned v, const Sample& s, int D, int H, int W) {
  Voxel r;
  const unsigned row = v / (unsigned)W;
  const int x = (int)(v - row * (unsigned)W), z = (int)(row / (unsigned)H), y = (int)(row - (unsigned)z * (unsigned)H);
  r.pz = lin(z, D, s.sz); r.py = lin(y, H, s.sy); r.px = lin(x, W, s.sx);
  affine_coord_chain(s.M, r.pz, r.py, r.px, r.gx, r.gy, r.gz);
  r.t = make_tap(r.gx, r.gy, r.gz, D, H, W);
  return r;
}

// Which voxels the masked kernels count.  Fixed-lattice voxel v with sampling coordinate g(v) is COUNTED iff fmask[v] != 0 (NULL:
// yes), with `inside` |g(v)_k| <= 1 on all three axes (a NaN is outside), and mmask != 0 at the nearest sampler's voxel for g(v)
// (NULL: yes): the definition's
//   c = fixed_mask & (align_img(grid, moving_mask, "nearest") != 0) & (|grid| <= 1).all(-1).
// M_n = the number of counted voxels (cnt[n], 64-bit on the device) replaces V as in mi.hip's masked kernels; it is piecewise
// constant in the matrix and not differentiated.
// what the coordinate decides, before anything is fetched from `moving` or its mask
__device__ __forceinline__ bool in_extent(const Voxel& p) { return fabsf(p.gx) <= 1.f && fabsf(p.gy) <= 1.f && fabsf(p.gz) <= 1.f; }
// the nearest sampler's voxel (sampler.hip): rintf of the border-clipped coordinate
__device__ __forceinline__ unsigned nearest_index(const Tap& t, int H, int W) {
  const int xn = (int)rintf((float)t.x0 + t.fx), yn = (int)rintf((float)t.y0 + t.fy), zn = (int)rintf((float)t.z0 + t.fz);
  return (unsigned)((zn * H + yn) * W + xn);
}

// grid (blocks, N); R, per as in mi.hip's histogram body.  LDS: kWaves tables of B * B.
__global__ __launch_bounds__(TPB) void warp_mi_hist_kernel(const float* __restrict__ moving, const float* __restrict__ fixed,
                                                           const float* __restrict__ mat, const float* __restrict__ rng,
                                                           int D, int H, int W, int R, int per, int B,
                                                           unsigned long long* __restrict__ hist) {
  extern __shared__ unsigned tab[];
  const int n = blockIdx.y, BB = B * B, lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const Range r = load_range(rng, n);
  const Sample s = load_sample(moving, mat, n, D, H, W);
  const int beg = per * blockIdx.x;
  const int end = beg + per < R ? beg + per : R;
  fixed += (long long)n * s.V;
  hist += (long long)n * BB;
  zero_tables<kWaves>(tab, BB);
  unsigned* mine = tab + wid * BB;
  for (int c = beg; c < end; c += kSteps * kWaves) {
#pragma unroll 1
    for (int it0 = 0; it0 < kSteps; it0 += kIlp) {
      TapB q[kIlp];
      float xb[kIlp], cv[kIlp][8];
      unsigned live = 0u;
#pragma unroll
      for (int u = 0; u < kIlp; ++u) {
        const int j = c + wid * kSteps + it0 + u;
        const unsigned v = (unsigned)j * kWave + lane;                 // j < R <= 2^24: no overflow
        const bool valid = j < end && v < s.V;
        live |= (valid ? 1u : 0u) << u;
        const Voxel p = voxel_tap(valid ? v : 0u, s, D, H, W);
        q[u] = make_tapb(p.t, D, H, W);
        if (!valid) park(q[u], s.plane_bytes);
        xb[u] = fixed[valid ? v : 0u];
      }
#pragma unroll
      for (int u = 0; u < kIlp; ++u) gather8_b(s.rm, q[u], cv[u]);
#pragma unroll
      for (int u = 0; u < kIlp; ++u) {
        const bool valid = (live >> u) & 1u;
        if (!__any(valid)) continue;                                  // wave-uniform
        hist_add(valid, blend8(cv[u], q[u].fx, q[u].fy, q[u].fz), xb[u], r, B, lane, mine);
      }
    }
    flush_tables<kWaves, false>(tab, BB, hist, 0u, nullptr);
  }
}

// warp_mi_hist_kernel over the counted voxels: the group's fixed-mask bytes are loaded first; a lane they or `inside` rule out is
// parked before the gathers and reads no moving-mask byte, and a step without a lane left skips its gathers, its taps and its
// adds.  The moving-mask byte (one per lane still in) travels with the gathers.  Each wave sums its ballots for the workgroup's
// count (flush_tables).
// A kernel of its own text, by measurement: as one body with the kernel above, templated on the mask as mi.hip's pair is, it
// came out slower with both masks given.  MI355X, tools/bench_masked_mi.py, medians of 30 calls in ms, separate processes in the
// order two texts, one body, two texts, one body (profiles/mi_dedup_kernel_identity.md):
//   128^3 ball (both)  0.0698 0.0736 0.0683 0.0714      256^3 ball (both)  0.2287 0.2302 0.2300 0.2314
// The one body's mean exceeds the two texts' by more than their two runs differ.
__global__ __launch_bounds__(TPB) void warp_mi_hist_masked_kernel(const float* __restrict__ moving, const float* __restrict__ fixed,
                                                                  const unsigned char* __restrict__ fmask,
                                                                  const unsigned char* __restrict__ mmask,
                                                                  const float* __restrict__ mat, const float* __restrict__ rng,
                                                                  int D, int H, int W, int R, int per, int B, int inside,
                                                                  unsigned long long* __restrict__ hist,
                                                                  unsigned long long* __restrict__ cnt) {
  extern __shared__ unsigned tab[];
  const int n = blockIdx.y, BB = B * B, lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const Range r = load_range(rng, n);
  const Sample s = load_sample(moving, mat, n, D, H, W);
  const int beg = per * blockIdx.x;
  const int end = beg + per < R ? beg + per : R;
  fixed += (long long)n * s.V;
  if (fmask) fmask += (long long)n * s.V;
  if (mmask) mmask += (long long)n * s.V;
  hist += (long long)n * BB;
  zero_tables<kWaves>(tab, BB);
  unsigned* mine = tab + wid * BB;
  for (int c = beg; c < end; c += kSteps * kWaves) {
    unsigned counted_here = 0u;                                       // wave-uniform
#pragma unroll 1
    for (int it0 = 0; it0 < kSteps; it0 += kIlp) {
      unsigned live = 0u;
#pragma unroll
      for (int u = 0; u < kIlp; ++u) {
        const int j = c + wid * kSteps + it0 + u;
        const unsigned v = (unsigned)j * kWave + lane;                 // j < R <= 2^24: no overflow
        const bool in = j < end && v < s.V;
        const bool keep = in && (fmask ? fmask[in ? v : 0u] != 0 : true);
        live |= (keep ? 1u : 0u) << u;
      }
      TapB q[kIlp];
      float xb[kIlp], cv[kIlp][8];
      unsigned char mm[kIlp];
#pragma unroll
      for (int u = 0; u < kIlp; ++u) {
        const unsigned v = (unsigned)(c + wid * kSteps + it0 + u) * kWave + lane;
        bool keep = (live >> u) & 1u;
        const Voxel p = voxel_tap(keep ? v : 0u, s, D, H, W);
        if (inside && !in_extent(p)) {
          keep = false;
          live &= ~(1u << u);
        }
        q[u] = make_tapb(p.t, D, H, W);
        if (!keep) park(q[u], s.plane_bytes);
        mm[u] = 1;
        if (__any(keep)) {                                            // wave-uniform
          xb[u] = fixed[keep ? v : 0u];
          if (mmask && keep) mm[u] = mmask[nearest_index(p.t, H, W)];
          gather8_b(s.rm, q[u], cv[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < kIlp; ++u) {
        const bool valid = ((live >> u) & 1u) && mm[u] != 0;
        const unsigned long long who = __ballot(valid);
        if (!who) continue;                                           // wave-uniform
        counted_here += (unsigned)__popcll(who);
        hist_add(valid, blend8(cv[u], q[u].fx, q[u].fy, q[u].fz), xb[u], r, B, lane, mine);
      }
    }
    flush_tables<kWaves, true>(tab, BB, hist, counted_here, cnt + n);
  }
}

// grid (blocks, N), grid-stride over the sample's voxels, lane-contiguous.  LDS: G of the sample (B * B floats).
// partial (N, gridDim.x, 12) doubles.
// The per-voxel text below (gather, taps, ga, blend_grads, the NaN gate, the 12 sums) and the epilogue stand in both backward
// kernels by measurement: the time follows the order in which the compiler issues the fixed[v] load and the gathers.  MI355X,
// medians of 30 calls in ms, separate processes in the order two texts, shared, two texts, shared
// (profiles/mi_dedup_kernel_identity.md):
//   a per-voxel helper that takes fixed[v] (tools/bench_masked_mi.py, unmasked)  256^3  0.1784 0.2006 0.1776 0.1993
//   one body for both kernels, masks NULL (tools/bench_warp_mi.py, fused bwd)    128^3  0.0438 0.0442 0.0436 0.0441
//                                         (tools/bench_masked_mi.py, ball both)  256^3  0.1360 0.1361 0.1361 0.1364
// Each shared form's mean exceeds the two texts' by more than their two runs differ.
__global__ __launch_bounds__(TPB) void warp_mi_bwd_kernel(const float* __restrict__ moving, const float* __restrict__ fixed,
                                                          const float* __restrict__ mat, const float* __restrict__ rng,
                                                          const float* __restrict__ G, const float* __restrict__ gout, int D,
                                                          int H, int W, int B, double* __restrict__ partial) {
  extern __shared__ float g[];
  __shared__ double red[kWaves];
  const int n = blockIdx.y, BB = B * B;
  for (int e = threadIdx.x; e < BB; e += TPB) g[e] = G[(long long)n * BB + e];
  __syncthreads();
  const Range r = load_range(rng, n);
  const float ca = gout[n] / (float)((unsigned)D * H * W) * r.s_a;
  const Sample s = load_sample(moving, mat, n, D, H, W);
  fixed += (long long)n * s.V;
  float acc[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) acc[i] = 0.f;
  for (long long v = (long long)blockIdx.x * TPB + threadIdx.x; v < s.V; v += (long long)gridDim.x * TPB) {
    const Voxel p = voxel_tap((unsigned)v, s, D, H, W);
    const TapB q = make_tapb(p.t, D, H, W);
    float cv[8];
    gather8_b(s.rm, q, cv);
    const float xb = fixed[v];
    const Taps ta = taps<true>(blend8(cv, q.fx, q.fy, q.fz), r.lo_a, r.s_a, B), tb = taps<false>(xb, r.lo_b, r.s_b, B);
    const float* row = g + ta.k0 * B + tb.k0;
    float ga = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float rw = 0.f;                                                // sum_j G_ij w_b[j]
#pragma unroll
      for (int j = 0; j < 4; ++j) rw = fmaf(row[i * B + j], tb.w[j], rw);
      ga = fmaf(ta.d[i], rw, ga);
    }
    const float go = ca * ga;                                        // dMI / da_v
    float dx, dy, dz;
    blend_grads(cv, q.fx, q.fy, q.fz, dx, dy, dz);
    const float k = any_nan(p.gx, p.gy, p.gz) ? 0.f : 1.f;
    const float d[3] = {dz * go * p.t.mz * k, dy * go * p.t.my * k, dx * go * p.t.mx * k};      // (z, y, x) rows
    const float b[4] = {p.pz, p.py, p.px, 1.f};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[i * 4 + c] += d[i] * b[c];
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const double sum = block_sum<double>((double)acc[i], red);
    if (threadIdx.x == 0) partial[((long long)n * gridDim.x + blockIdx.x) * 12 + i] = sum;
  }
}

// warp_mi_bwd_kernel over the counted voxels, with 1 / M_n for 1 / V: a lane that is not counted fetches nothing and adds nothing
__global__ __launch_bounds__(TPB) void warp_mi_bwd_masked_kernel(const float* __restrict__ moving, const float* __restrict__ fixed,
                                                                 const unsigned char* __restrict__ fmask,
                                                                 const unsigned char* __restrict__ mmask,
                                                                 const float* __restrict__ mat, const float* __restrict__ rng,
                                                                 const float* __restrict__ G, const float* __restrict__ gout,
                                                                 const unsigned long long* __restrict__ cnt, int D, int H, int W,
                                                                 int B, int inside, double* __restrict__ partial) {
  extern __shared__ float g[];
  __shared__ double red[kWaves];
  const int n = blockIdx.y, BB = B * B;
  for (int e = threadIdx.x; e < BB; e += TPB) g[e] = G[(long long)n * BB + e];
  __syncthreads();
  const Range r = load_range(rng, n);
  const long long Mn = (long long)cnt[n];
  const float ca = Mn ? gout[n] / (float)Mn * r.s_a : 0.f;
  const Sample s = load_sample(moving, mat, n, D, H, W);
  fixed += (long long)n * s.V;
  if (fmask) fmask += (long long)n * s.V;
  if (mmask) mmask += (long long)n * s.V;
  float acc[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) acc[i] = 0.f;
  for (long long v = (long long)blockIdx.x * TPB + threadIdx.x; v < s.V; v += (long long)gridDim.x * TPB) {
    if (fmask && fmask[v] == 0) continue;
    const Voxel p = voxel_tap((unsigned)v, s, D, H, W);
    if (inside && !in_extent(p)) continue;
    if (mmask && mmask[nearest_index(p.t, H, W)] == 0) continue;
    const TapB q = make_tapb(p.t, D, H, W);
    float cv[8];
    gather8_b(s.rm, q, cv);
    const float xb = fixed[v];
    const Taps ta = taps<true>(blend8(cv, q.fx, q.fy, q.fz), r.lo_a, r.s_a, B), tb = taps<false>(xb, r.lo_b, r.s_b, B);
    const float* row = g + ta.k0 * B + tb.k0;
    float ga = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float rw = 0.f;                                                // sum_j G_ij w_b[j]
#pragma unroll
      for (int j = 0; j < 4; ++j) rw = fmaf(row[i * B + j], tb.w[j], rw);
      ga = fmaf(ta.d[i], rw, ga);
    }
    const float go = ca * ga;                                        // dMI / da_v
    float dx, dy, dz;
    blend_grads(cv, q.fx, q.fy, q.fz, dx, dy, dz);
    const float k = any_nan(p.gx, p.gy, p.gz) ? 0.f : 1.f;
    const float d[3] = {dz * go * p.t.mz * k, dy * go * p.t.my * k, dx * go * p.t.mx * k};      // (z, y, x) rows
    const float b[4] = {p.pz, p.py, p.px, 1.f};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[i * 4 + c] += d[i] * b[c];
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const double sum = block_sum<double>((double)acc[i], red);
    if (threadIdx.x == 0) partial[((long long)n * gridDim.x + blockIdx.x) * 12 + i] = sum;
  }
}

// 12 outputs x 16 slices of the per-workgroup partials, combined in a fixed order
__global__ __launch_bounds__(192) void warp_mi_final_kernel(const double* __restrict__ partial, int nblk,
                                                            float* __restrict__ dmat) {
  __shared__ double red[16][12];
  const int n = blockIdx.x;
  const int i = threadIdx.x % 12, sl = threadIdx.x / 12;
  double s = 0;
  for (int b = sl; b < nblk; b += 16) s += partial[((long long)n * nblk + b) * 12 + i];
  red[sl][i] = s;
  __syncthreads();
  if (sl) return;
  s = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) s += red[k][i];
  dmat[n * 12 + i] = (float)s;
}

// buffer loads address a sample of `moving` with 32-bit byte offsets: fewer than 2^30 voxels
bool warp_mi_args_ok(const void* moving, const void* fixed, const void* mat, const void* rng, int N, int D, int H, int W,
                     int B) {
  return moving && fixed && mat && rng && N >= 1 && N <= 65535 && D >= 1 && H >= 1 && W >= 2 && B >= kMinBins &&
         B <= kMaxBins && (long long)D * H * W < (1ll << 30);
}
int bwd_blocks(long long V) {
  long long nb = (V + TPB * 16 - 1) / (TPB * 16);
  return (int)(nb > kBwdBlocks ? kBwdBlocks : nb);
}
size_t table_bytes(int N, int bins) { return (ws_bytes(N, bins) + 255) & ~(size_t)255; }

// The histogram pass: clears the table and the count, then the kernel over hist_steps' partition.  cnt != NULL: the masked kernel.
int warp_mi_hist_launch(const float* moving, const float* fixed, const unsigned char* fmask, const unsigned char* mmask,
                        const float* mat, const float* rng, int N, int D, int H, int W, int bins, int inside, void* ws,
                        long long* cnt, hipStream_t s) {
  hipError_t e = hipMemsetAsync(ws, 0, ws_bytes(N, bins), s);
  if (e == hipSuccess && cnt) e = hipMemsetAsync(cnt, 0, (size_t)N * sizeof(long long), s);
  if (e != hipSuccess) return (int)e;
  const HistSteps p = hist_steps((long long)D * H * W, kWaves);
  const dim3 grid((unsigned)p.nb, (unsigned)N);
  const size_t lds = (size_t)kWaves * bins * bins * sizeof(unsigned);
  if (cnt)
    warp_mi_hist_masked_kernel<<<grid, TPB, lds, s>>>(moving, fixed, fmask, mmask, mat, rng, D, H, W, (int)p.R, (int)p.per, bins,
                                                      inside != 0, ws_table(ws, N), (unsigned long long*)cnt);
  else
    warp_mi_hist_kernel<<<grid, TPB, lds, s>>>(moving, fixed, mat, rng, D, H, W, (int)p.R, (int)p.per, bins, ws_table(ws, N));
  return KMH_LAUNCH_CHECK();
}

// The backward pass: per-workgroup partials behind the table in ws, then their fixed-order sum.  cnt != NULL: the masked kernel.
int warp_mi_bwd_launch(const float* moving, const float* fixed, const unsigned char* fmask, const unsigned char* mmask,
                       const float* mat, const float* rng, const float* G, const float* gout, const long long* cnt, int N, int D,
                       int H, int W, int bins, int inside, void* ws, float* dmat, hipStream_t s) {
  double* partial = (double*)((char*)ws + table_bytes(N, bins));
  const int nb = bwd_blocks((long long)D * H * W);
  const size_t lds = (size_t)bins * bins * sizeof(float);
  if (cnt)
    warp_mi_bwd_masked_kernel<<<dim3(nb, N), TPB, lds, s>>>(moving, fixed, fmask, mmask, mat, rng, G, gout,
                                                            (const unsigned long long*)cnt, D, H, W, bins, inside != 0, partial);
  else
    warp_mi_bwd_kernel<<<dim3(nb, N), TPB, lds, s>>>(moving, fixed, mat, rng, G, gout, D, H, W, bins, partial);
  warp_mi_final_kernel<<<N, 192, 0, s>>>(partial, nb, dmat);
  return KMH_LAUNCH_CHECK();
}
}  // namespace

/* Workspace of kmh_warp_mi_hist / kmh_mi_final / kmh_warp_mi_bwd: the joint table in kmh_mi_hist's layout, then the backward
 * pass's per-workgroup partial sums. */
KMH_API size_t kmh_warp_mi_ws_bytes(int N, int bins, int D, int H, int W) {
  if (N < 0 || bins < 0 || D < 1 || H < 1 || W < 1) return 0;
  return table_bytes(N, bins) + (size_t)N * bwd_blocks((long long)D * H * W) * 12 * sizeof(double);
}

/* moving, fixed: (N, D, H, W) float32 contiguous; mat (N, 3, 4) as kmh_affine_grid_fwd takes it; rng (N, 4) = (lo_a, s_a, lo_b,
 * s_b) with a = the warped moving volume (kmh_mi_range of (moving, fixed)).  Leaves the joint table in ws for kmh_mi_final
 * (same N, bins, V = D H W).  8 <= bins <= 64, W >= 2, fewer than 2^30 voxels per sample. */
KMH_API int kmh_warp_mi_hist(const float* moving, const float* fixed, const float* mat, const float* rng, int N, int D, int H,
                             int W, int bins, void* ws, void* stream) {
  if (!warp_mi_args_ok(moving, fixed, mat, rng, N, D, H, W, bins) || !ws) return -22;
  return warp_mi_hist_launch(moving, fixed, nullptr, nullptr, mat, rng, N, D, H, W, bins, 0, ws, nullptr, (hipStream_t)stream);
}

/* dmat (N, 3, 4) = gout[n] dMI_n / dmat.  G as written by kmh_mi_final for the table of kmh_warp_mi_hist with the same
 * arguments; ws: kmh_warp_mi_ws_bytes(N, bins, D, H, W) bytes (the table in it is not read). */
KMH_API int kmh_warp_mi_bwd(const float* moving, const float* fixed, const float* mat, const float* rng, const float* G,
                            const float* gout, int N, int D, int H, int W, int bins, void* ws, float* dmat, void* stream) {
  if (!warp_mi_args_ok(moving, fixed, mat, rng, N, D, H, W, bins) || !G || !gout || !ws || !dmat) return -22;
  return warp_mi_bwd_launch(moving, fixed, nullptr, nullptr, mat, rng, G, gout, nullptr, N, D, H, W, bins, 0, ws, dmat,
                            (hipStream_t)stream);
}

/* kmh_warp_mi_hist over the counted voxels only (the definition is above in_extent): fixed_mask, moving_mask (N, D, H, W)
 * bytes, non-zero = counted, either may be NULL; inside != 0 drops voxels whose coordinate leaves [-1, 1].  cnt: N 64-bit
 * integers out (cleared here); kmh_mi_final_masked(ws, rng, cnt, ...) follows. */
KMH_API int kmh_warp_mi_hist_masked(const float* moving, const float* fixed, const unsigned char* fixed_mask,
                                    const unsigned char* moving_mask, const float* mat, const float* rng, int N, int D, int H,
                                    int W, int bins, int inside, void* ws, long long* cnt, void* stream) {
  if (!warp_mi_args_ok(moving, fixed, mat, rng, N, D, H, W, bins) || !ws || !cnt) return -22;
  return warp_mi_hist_launch(moving, fixed, fixed_mask, moving_mask, mat, rng, N, D, H, W, bins, inside, ws, cnt,
                             (hipStream_t)stream);
}

/* kmh_warp_mi_bwd over the counted voxels, scaled by 1 / cnt[n] (cnt as kmh_warp_mi_hist_masked left it for the same
 * arguments; it is not differentiated); G from kmh_mi_final_masked. */
KMH_API int kmh_warp_mi_bwd_masked(const float* moving, const float* fixed, const unsigned char* fixed_mask,
                                   const unsigned char* moving_mask, const float* mat, const float* rng, const float* G,
                                   const float* gout, const long long* cnt, int N, int D, int H, int W, int bins, int inside,
                                   void* ws, float* dmat, void* stream) {
  if (!warp_mi_args_ok(moving, fixed, mat, rng, N, D, H, W, bins) || !G || !gout || !cnt || !ws || !dmat) return -22;
  return warp_mi_bwd_launch(moving, fixed, fixed_mask, moving_mask, mat, rng, G, gout, cnt, N, D, H, W, bins, inside, ws, dmat,
                            (hipStream_t)stream);
}

