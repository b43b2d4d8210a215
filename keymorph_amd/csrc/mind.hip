// MIND-SSC, the self-similarity context descriptor (Heinrich et al., MICCAI 2013), as a similarity of two volumes, with its gradient.
//
// a, b: (N, D, H, W) float32, each sample on its own.  Radius r and dilation d in {1, 2, 3}; clamp() is the per-axis clamp into
// the volume (replication).  The six neighbours of a voxel, in this order:
//   0: -d z    1: +d z    2: -d y    3: +d y    4: -d x    5: +d x
// The 12 channels are the unordered pairs (i, j) of distinct, non-opposite neighbours, in this order:
//   c:  0      1      2      3      4      5      6      7      8      9      10     11
//      (0,2)  (0,3)  (0,4)  (0,5)  (1,2)  (1,3)  (1,4)  (1,5)  (2,4)  (2,5)  (3,4)  (3,5)
//   E_c(q) = (I(clamp(q + o_i)) - I(clamp(q + o_j)))^2
//   D_c(p) = (2r+1)^-3 sum over o in [-r, r]^3 of E_c(clamp(p + o))            the box mean over the replicate-padded field
//   m_c = D_c - min_k D_k      (ties: the lowest channel index, in the backward as well)
//   V = min(max(mean_c m_c, lo), hi)      M_c = exp(-m_c / V)      (V == 0, only with lo == 0: M_c = 1, no gradient)
//   out[n] = mean over the voxels and the 12 channels of (M_c(a) - M_c(b))^2                      (>= 0; lower is better)
// lo, hi are constants of the call, bounds (N, 2, 2) = [a or b][lo or hi]; kmh_mind_bounds gives 1e-3 and 1e3 times the sample's
// mean over the voxels of the unclamped mean_c m_c (per-tile partials in a fixed order, added in fp64).
//
// Gradient of out[n] with respect to x (= a; b alike with the roles exchanged), s = gout[n] / (12 voxels):
//   gM_c = 2 s (M_c(x) - M_c(y))
//   gm_k = -gM_k M_k / V + [lo <= mean m <= hi] (1/12) sum_c gM_c M_c m_c / V^2
//   gD_k = gm_k - [k == argmin] sum_c gm_c
//   gE_c(q) = (2r+1)^-3 sum_p wz wy wx gD_c(p):  the transpose of the replicate-padded box, per axis the number of o in [-r, r]
//             with clamp(p + o) == q: 1 inside the truncated window, r - |p - q| + 1 on a face for the padding folded onto it
//   G_i(q) = sum over the channels holding neighbour i of +-2 gE_c(q) (I(clamp(q + o_i)) - I(clamp(q + o_j)))
//   dx(v) = sum_i sum over q with clamp(q + o_i) == v of G_i(q): q = v - o_i, and on a face the d voxels clamped there as well
// Every transpose is a gather; nothing is scattered and there are no floating-point atomics: two runs are bit-identical, the
// tiling depends on (D, H, W) alone, so a batch equals its samples run one by one, and each side is its own sequence of
// launches, so one gradient alone equals the same gradient of a call for both.
//
// A workgroup of 256 owns a 4 x 8 x 32 (z, y, x) tile, one z column of 4 voxels per lane.
//   mind_D          the raw volume with a halo of r + d (replicated) goes to LDS once; then per box plane: the x pass sums 2r+1
//                   squared neighbour differences of every halo row for all 12 channels (four at a time at r = 3, where 12
//                   planes of row sums no longer fit in 64 KB), the y pass sums 2r+1 of those rows, and the plane is added to
//                   the lane's up to 2r+1 output voxels it belongs to: ascending x, then y, then z.
//   mind_fwd_kernel D and M of a, then of b, the squared differences summed per tile; mind_final_kernel adds them in fp64.
//   mind_cot_kernel the backward's first pass: the same walk, writes gD (12 fields, 48 B per voxel).
//   mind_boxT_kernel  the second: planes of gD with a halo of r (zeros outside), the weighted x, y, z passes, G (6 fields, 24 B).
//   mind_shiftT_kernel  the third: the gather of G along the six shifts.
#include "common.h"

namespace {
constexpr int TPB = 256;
constexpr int kTX = 32, kTY = 8, kTZ = 4;
constexpr int kCh = 12, kNb = 6, kMaxR = 3, kMaxDil = 3;
static_assert(kTX * kTY == TPB, "one z column of the tile per lane");
static_assert(kTX + 2 * (kMaxR + kMaxDil) <= kWave, "a halo row is loaded by one wave");

__device__ __forceinline__ constexpr int ch_i(int c) { return c < 4 ? 0 : c < 8 ? 1 : c < 10 ? 2 : 3; }
__device__ __forceinline__ constexpr int ch_j(int c) { return c < 8 ? 2 + (c & 3) : 4 + (c & 1); }
__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// channels whose row sums are held in LDS at a time, and the LDS floats of mind_D
template <int R> constexpr int kGroup = R == 3 ? 4 : kCh;
template <int R> constexpr int kHaloMax = (kTZ + 2 * (R + kMaxDil)) * (kTY + 2 * (R + kMaxDil)) * (kTX + 2 * (R + kMaxDil));
template <int R> constexpr int kLdsD = kHaloMax<R> + kGroup<R> * (kTY + 2 * R) * kTX;
static_assert(kLdsD<1> * 4 + 64 <= 65536 && kLdsD<2> * 4 + 64 <= 65536 && kLdsD<3> * 4 + 64 <= 65536, "LDS");

// tile -> its corner; tiles run x fastest, then y, then z
__device__ __forceinline__ void tile_corner(int t, int H, int W, int& z0, int& y0, int& x0) {
  const int nx = (W + kTX - 1) / kTX, ny = (H + kTY - 1) / kTY;
  x0 = (t % nx) * kTX;
  y0 = (t / nx % ny) * kTY;
  z0 = (t / nx / ny) * kTZ;
}

// Dv[v][c] = D_c at (z0 + v, y0 + ty, x0 + tx) of one sample's volume I; voxels outside the volume get values nobody reads.
template <int R>
__device__ __forceinline__ void mind_D(const float* __restrict__ I, int D, int H, int W, int d, int z0, int y0, int x0,
                                       float* lds, float (&Dv)[kTZ][kCh]) {
  constexpr int G = kGroup<R>, BY = kTY + 2 * R, WIN = 2 * R + 1, ROWS = BY * kTX;
  const int h = R + d, hy = kTY + 2 * h, hx = kTX + 2 * h, hplane = hy * hx;
  float* halo = lds;                                                  // [kTZ + 2h][hy][hx], I(clamp(corner - h + index))
  float* xs = lds + kHaloMax<R>;                                      // [G][BY][kTX]
  const int tid = threadIdx.x, ty = tid / kTX, tx = tid % kTX;
  __syncthreads();                                                    // the previous walk is done with the LDS
  {                                                                   // a wave per halo row (hx <= 44 lanes of it): no divisions
    const int lane = tid % kWave, wid = tid / kWave;
    const int x = clampi(x0 - h + lane, W);
    if (lane < hx)
      for (int ez = 0; ez < kTZ + 2 * h; ++ez) {
        const float* src = I + (size_t)clampi(z0 - h + ez, D) * H * W + x;
        for (int ey = wid; ey < hy; ey += TPB / kWave)
          halo[ez * hplane + ey * hx + lane] = src[(size_t)clampi(y0 - h + ey, H) * W];
      }
  }
  __syncthreads();
#pragma unroll
  for (int v = 0; v < kTZ; ++v)
#pragma unroll
    for (int c = 0; c < kCh; ++c) Dv[v][c] = 0.f;
  const int sz = d * hplane, sy = d * hx;
  for (int pz = 0; pz < kTZ + 2 * R; ++pz) {                          // the box plane clamp(z0 - R + pz)
    const int qz = clampi(z0 - R + pz, D) - (z0 - h);
#pragma unroll
    for (int g = 0; g < kCh / G; ++g) {
      for (int it = tid; it < ROWS; it += TPB) {                      // x pass: row it / 32 of the box halo, output column it % 32
        const int row = it / kTX, col = it % kTX;
        const int qy = clampi(y0 - R + row, H) - (y0 - h);
        const float* base = halo + (qz * hy + qy) * hx;
        float s[G];
#pragma unroll
        for (int c = 0; c < G; ++c) s[c] = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
          const float* p = base + (clampi(x0 - R + col + k, W) - (x0 - h));
          const float nb[kNb] = {p[-sz], p[sz], p[-sy], p[sy], p[-d], p[d]};
#pragma unroll
          for (int c = 0; c < G; ++c) {
            const float diff = nb[ch_i(g * G + c)] - nb[ch_j(g * G + c)];
            s[c] = fmaf(diff, diff, s[c]);
          }
        }
#pragma unroll
        for (int c = 0; c < G; ++c) xs[c * ROWS + it] = s[c];
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < G; ++c) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) s += xs[c * ROWS + (ty + k) * kTX + tx];            // y pass
#pragma unroll
        for (int v = 0; v < kTZ; ++v)
          if (pz >= v && pz <= v + 2 * R) Dv[v][g * G + c] += s;                          // z pass, ascending
      }
      __syncthreads();
    }
  }
  constexpr float inv = 1.f / (float)(WIN * WIN * WIN);
#pragma unroll
  for (int v = 0; v < kTZ; ++v)
#pragma unroll
    for (int c = 0; c < kCh; ++c) Dv[v][c] *= inv;
}

// m (in place of Dc), the unclamped mean, 1 / V (0 for V == 0) and the argmin
__device__ __forceinline__ void mind_m(float (&Dc)[kCh], float lo, float hi, float& meanm, float& invV, int& kmin) {
  float mn = Dc[0];
  kmin = 0;
#pragma unroll
  for (int c = 1; c < kCh; ++c)
    if (Dc[c] < mn) mn = Dc[c], kmin = c;
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < kCh; ++c) {
    Dc[c] -= mn;
    sum += Dc[c];
  }
  meanm = sum * (1.f / kCh);
  const float V = fminf(fmaxf(meanm, lo), hi);
  invV = V > 0.f ? 1.f / V : 0.f;
}

// grid (tiles, N, 2): partial (N, 2, tiles) of the unclamped mean_c m_c of a (z = 0) or b (z = 1)
template <int R>
__global__ __launch_bounds__(TPB) void mind_mean_kernel(const float* __restrict__ a, const float* __restrict__ b, int D, int H,
                                                        int W, int d, float* __restrict__ partial) {
  __shared__ float lds[kLdsD<R>];
  __shared__ float scratch[TPB / kWave];
  const int n = blockIdx.y, img = blockIdx.z;
  const size_t V = (size_t)D * H * W;
  int z0, y0, x0;
  tile_corner(blockIdx.x, H, W, z0, y0, x0);
  float Dv[kTZ][kCh];
  mind_D<R>((img ? b : a) + n * V, D, H, W, d, z0, y0, x0, lds, Dv);
  const int y = y0 + threadIdx.x / kTX, x = x0 + threadIdx.x % kTX;
  float acc = 0.f;
#pragma unroll
  for (int v = 0; v < kTZ; ++v) {
    float meanm, invV;
    int kmin;
    mind_m(Dv[v], 0.f, 0.f, meanm, invV, kmin);
    if (z0 + v < D && y < H && x < W) acc += meanm;
  }
  const float sum = block_sum(acc, scratch);
  if (threadIdx.x == 0) partial[((size_t)n * 2 + img) * gridDim.x + blockIdx.x] = sum;
}

// one workgroup per (sample, image): bounds[n][img] = (1e-3, 1e3) x the mean, in fp64 in a fixed order
__global__ __launch_bounds__(TPB) void mind_bounds_final_kernel(const float* __restrict__ partial, int tiles, long long V,
                                                                float* __restrict__ bounds) {
  __shared__ double scratch[TPB / kWave];
  const int k = blockIdx.x;
  double acc = 0.0;
  for (int t = threadIdx.x; t < tiles; t += TPB) acc += (double)partial[(size_t)k * tiles + t];
  acc = block_sum(acc, scratch);
  if (threadIdx.x == 0) {
    const double mean = acc / (double)V;
    bounds[2 * k] = (float)(1e-3 * mean);
    bounds[2 * k + 1] = (float)(1e3 * mean);
  }
}

// grid (tiles, N): partial (N, tiles) of sum over the tile's voxels and channels of (M_c(a) - M_c(b))^2
template <int R>
__global__ __launch_bounds__(TPB) void mind_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       const float* __restrict__ bounds, int D, int H, int W, int d,
                                                       float* __restrict__ partial) {
  __shared__ float lds[kLdsD<R>];
  __shared__ float scratch[TPB / kWave];
  const int n = blockIdx.y;
  const size_t V = (size_t)D * H * W;
  const float* bd = bounds + 4 * n;
  int z0, y0, x0;
  tile_corner(blockIdx.x, H, W, z0, y0, x0);
  float Ma[kTZ][kCh], Dv[kTZ][kCh];
  mind_D<R>(a + n * V, D, H, W, d, z0, y0, x0, lds, Ma);
#pragma unroll
  for (int v = 0; v < kTZ; ++v) {
    float meanm, invV;
    int kmin;
    mind_m(Ma[v], bd[0], bd[1], meanm, invV, kmin);
#pragma unroll
    for (int c = 0; c < kCh; ++c) Ma[v][c] = expf(-Ma[v][c] * invV);
  }
  mind_D<R>(b + n * V, D, H, W, d, z0, y0, x0, lds, Dv);
  const int y = y0 + threadIdx.x / kTX, x = x0 + threadIdx.x % kTX;
  float acc = 0.f;
#pragma unroll
  for (int v = 0; v < kTZ; ++v) {
    float meanm, invV;
    int kmin;
    mind_m(Dv[v], bd[2], bd[3], meanm, invV, kmin);
    float e = 0.f;
#pragma unroll
    for (int c = 0; c < kCh; ++c) {
      const float diff = Ma[v][c] - expf(-Dv[v][c] * invV);
      e = fmaf(diff, diff, e);
    }
    if (z0 + v < D && y < H && x < W) acc += e;
  }
  const float sum = block_sum(acc, scratch);
  if (threadIdx.x == 0) partial[(size_t)n * gridDim.x + blockIdx.x] = sum;
}

// one workgroup per sample: out[n] = sum of its partials / (12 V), in fp64 in a fixed order
__global__ __launch_bounds__(TPB) void mind_final_kernel(const float* __restrict__ partial, int tiles, long long V,
                                                         float* __restrict__ out) {
  __shared__ double scratch[TPB / kWave];
  const int n = blockIdx.x;
  double acc = 0.0;
  for (int t = threadIdx.x; t < tiles; t += TPB) acc += (double)partial[(size_t)n * tiles + t];
  acc = block_sum(acc, scratch);
  if (threadIdx.x == 0) out[n] = (float)(acc / ((double)kCh * (double)V));
}

// The backward's first pass for the side x (y the other image; bx, by their (lo, hi)): gD, (N, 12, V).
template <int R>
__global__ __launch_bounds__(TPB) void mind_cot_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ bounds, int xside,
                                                       const float* __restrict__ gout, int D, int H, int W, int d,
                                                       float* __restrict__ gD) {
  __shared__ float lds[kLdsD<R>];
  const int n = blockIdx.y;
  const size_t V = (size_t)D * H * W;
  const float* bx = bounds + 4 * n + 2 * xside;
  const float* by = bounds + 4 * n + 2 * (1 - xside);
  int z0, y0, x0;
  tile_corner(blockIdx.x, H, W, z0, y0, x0);
  float My[kTZ][kCh], Dv[kTZ][kCh];
  mind_D<R>(y + n * V, D, H, W, d, z0, y0, x0, lds, My);
#pragma unroll
  for (int v = 0; v < kTZ; ++v) {
    float meanm, invV;
    int kmin;
    mind_m(My[v], by[0], by[1], meanm, invV, kmin);
#pragma unroll
    for (int c = 0; c < kCh; ++c) My[v][c] = expf(-My[v][c] * invV);
  }
  mind_D<R>(x + n * V, D, H, W, d, z0, y0, x0, lds, Dv);
  const float s2 = 2.f * gout[n] / ((float)kCh * (float)V);
  const float lo = bx[0], hi = bx[1];
  const int yy = y0 + threadIdx.x / kTX, xx = x0 + threadIdx.x % kTX;
  float* out = gD + (size_t)n * kCh * V;
#pragma unroll
  for (int v = 0; v < kTZ; ++v) {
    float meanm, invV;
    int kmin;
    mind_m(Dv[v], lo, hi, meanm, invV, kmin);
    float t[kCh], cross = 0.f;                                        // t_c = gM_c M_c; cross = sum_c t_c m_c
#pragma unroll
    for (int c = 0; c < kCh; ++c) {
      const float M = expf(-Dv[v][c] * invV);
      t[c] = s2 * (M - My[v][c]) * M;
      cross = fmaf(t[c], Dv[v][c], cross);
    }
    const float shared = (meanm >= lo && meanm <= hi) ? cross * invV * invV * (1.f / kCh) : 0.f;
    float total = 0.f;
#pragma unroll
    for (int c = 0; c < kCh; ++c) {
      t[c] = fmaf(-t[c], invV, shared);                               // gm_c
      total += t[c];
    }
    if (z0 + v < D && yy < H && xx < W) {
      const size_t i = ((size_t)(z0 + v) * H + yy) * W + xx;
#pragma unroll
      for (int c = 0; c < kCh; ++c) out[c * V + i] = c == kmin ? t[c] - total : t[c];
    }
  }
}

// the number of o in [-r, r] with clamp(p + o) == q, for p inside [0, n)
__device__ __forceinline__ float fold_weight(int p, int q, int r, int n) {
  if (p < 0 || p >= n) return 0.f;
  const int lo = q == 0 ? -r : (q - p > -r ? q - p : -r), hi = q == n - 1 ? r : (q - p < r ? q - p : r);
  return hi >= lo ? (float)(hi - lo + 1) : 0.f;
}

// The second pass: gE = the transposed box of gD, folded with the neighbour differences into G, (N, 6, V).
template <int R>
__global__ __launch_bounds__(TPB) void mind_boxT_kernel(const float* __restrict__ x, const float* __restrict__ gD, int D, int H,
                                                        int W, int d, float* __restrict__ G) {
  constexpr int BY = kTY + 2 * R, PX = kTX + 2 * R, PLANE = BY * PX, ROWS = BY * kTX, WIN = 2 * R + 1;
  __shared__ float raw[kCh * PLANE];                                  // [12][BY][PX], zeros outside the volume
  __shared__ float xs[kCh * ROWS];                                    // [12][BY][kTX]
  const int n = blockIdx.y, tid = threadIdx.x, ty = tid / kTX, tx = tid % kTX;
  const size_t V = (size_t)D * H * W;
  const float* I = x + n * V;
  const float* src = gD + (size_t)n * kCh * V;
  int z0, y0, x0;
  tile_corner(blockIdx.x, H, W, z0, y0, x0);
  float gE[kTZ][kCh];
#pragma unroll
  for (int v = 0; v < kTZ; ++v)
#pragma unroll
    for (int c = 0; c < kCh; ++c) gE[v][c] = 0.f;
  for (int pz = z0 - R; pz < z0 + kTZ + R; ++pz) {
    if (pz < 0 || pz >= D) continue;                                  // workgroup-uniform
    for (int e = tid; e < PLANE; e += TPB) {
      const int py = y0 - R + e / PX, px = x0 - R + e % PX;
      const bool in = py >= 0 && py < H && px >= 0 && px < W;
      const size_t i = in ? ((size_t)pz * H + py) * W + px : 0;
#pragma unroll
      for (int c = 0; c < kCh; ++c) raw[c * PLANE + e] = in ? src[c * V + i] : 0.f;
    }
    __syncthreads();
    for (int it = tid; it < ROWS; it += TPB) {                        // x pass
      const int row = it / kTX, col = it % kTX;
      float w[WIN], s[kCh];
#pragma unroll
      for (int k = 0; k < WIN; ++k) w[k] = fold_weight(x0 + col - R + k, x0 + col, R, W);
#pragma unroll
      for (int c = 0; c < kCh; ++c) {
        s[c] = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) s[c] = fmaf(w[k], raw[c * PLANE + row * PX + col + k], s[c]);
        xs[c * ROWS + it] = s[c];
      }
    }
    __syncthreads();
    float wy[WIN], wz[kTZ];
#pragma unroll
    for (int k = 0; k < WIN; ++k) wy[k] = fold_weight(y0 + ty - R + k, y0 + ty, R, H);
#pragma unroll
    for (int v = 0; v < kTZ; ++v) wz[v] = fold_weight(pz, z0 + v, R, D);
#pragma unroll
    for (int c = 0; c < kCh; ++c) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < WIN; ++k) s = fmaf(wy[k], xs[c * ROWS + (ty + k) * kTX + tx], s);       // y pass
#pragma unroll
      for (int v = 0; v < kTZ; ++v) gE[v][c] = fmaf(wz[v], s, gE[v][c]);                         // z pass, ascending
    }
    __syncthreads();
  }
  constexpr float inv2 = 2.f / (float)(WIN * WIN * WIN);
  const int yy = y0 + ty, xx = x0 + tx;
  float* out = G + (size_t)n * kNb * V;
  if (yy < H && xx < W) {
#pragma unroll
    for (int v = 0; v < kTZ; ++v) {
      const int zz = z0 + v;
      if (zz >= D) continue;
      const size_t i = ((size_t)zz * H + yy) * W + xx;
      const float nb[kNb] = {I[((size_t)clampi(zz - d, D) * H + yy) * W + xx], I[((size_t)clampi(zz + d, D) * H + yy) * W + xx],
                             I[((size_t)zz * H + clampi(yy - d, H)) * W + xx], I[((size_t)zz * H + clampi(yy + d, H)) * W + xx],
                             I[((size_t)zz * H + yy) * W + clampi(xx - d, W)], I[((size_t)zz * H + yy) * W + clampi(xx + d, W)]};
      float g[kNb] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < kCh; ++c) {
        const float t = inv2 * gE[v][c] * (nb[ch_i(c)] - nb[ch_j(c)]);
        g[ch_i(c)] += t;
        g[ch_j(c)] -= t;
      }
#pragma unroll
      for (int k = 0; k < kNb; ++k) out[k * V + i] = g[k];
    }
  }
}

// The third pass: dx(v) = sum_i sum over q with clamp(q + o_i) == v of G_i(q), neighbours and q ascending.
__global__ __launch_bounds__(TPB) void mind_shiftT_kernel(const float* __restrict__ G, int D, int H, int W, int d,
                                                          float* __restrict__ dx) {
  const size_t V = (size_t)D * H * W;
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= V) return;
  const int n = blockIdx.y;
  const int xx = (int)(i % W), yy = (int)(i / W % H), zz = (int)(i / W / H);
  const float* src = G + (size_t)n * kNb * V;
  const int pos[3] = {zz, yy, xx}, len[3] = {D, H, W};
  const size_t stride[3] = {(size_t)H * W, (size_t)W, 1};
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < kNb; ++k) {
    const int ax = k / 2, p = pos[ax], nlen = len[ax];
    int lo, hi;                                                       // q along the axis with clamp(q -+ d) == p
    if (k & 1) {                                                      // +d: q = p - d; on the high face every q >= n - 1 - d
      lo = p == nlen - 1 ? (nlen - 1 - d > 0 ? nlen - 1 - d : 0) : p - d;
      hi = p == nlen - 1 ? nlen - 1 : p - d;
      if (lo < 0) continue;
    } else {                                                          // -d: q = p + d; on the low face every q <= d
      lo = p == 0 ? 0 : p + d;
      hi = p == 0 ? (d < nlen - 1 ? d : nlen - 1) : p + d;
      if (hi > nlen - 1) continue;
    }
    const float* f = src + k * V + (i - (size_t)p * stride[ax]);
    for (int q = lo; q <= hi; ++q) acc += f[(size_t)q * stride[ax]];
  }
  dx[n * V + i] = acc;
}

bool mind_ok(int N, int D, int H, int W, int r, int d) {
  return N >= 1 && N <= 65535 && D >= 1 && H >= 1 && W >= 1 && (long long)D * H * W < (1ll << 31) && r >= 1 && r <= kMaxR &&
         d >= 1 && d <= kMaxDil;
}
long long mind_tiles(int D, int H, int W) { return (long long)ceil_div(D, kTZ) * ceil_div(H, kTY) * ceil_div(W, kTX); }
// the per-tile partials: (N, tiles) of the forward, or (N, 2, tiles) of the bounds
size_t mind_partial_bytes(int N, int D, int H, int W) {
  return ((size_t)2 * N * mind_tiles(D, H, W) * sizeof(float) + 255) / 256 * 256;
}

template <int R>
void mind_bounds_launch(const float* a, const float* b, int N, int D, int H, int W, int d, float* bounds, float* partial,
                        hipStream_t s) {
  const int tiles = (int)mind_tiles(D, H, W);
  mind_mean_kernel<R><<<dim3((unsigned)tiles, (unsigned)N, 2), TPB, 0, s>>>(a, b, D, H, W, d, partial);
  mind_bounds_final_kernel<<<2 * N, TPB, 0, s>>>(partial, tiles, (long long)D * H * W, bounds);
}

template <int R>
void mind_fwd_launch(const float* a, const float* b, const float* bounds, int N, int D, int H, int W, int d, float* out,
                     float* partial, hipStream_t s) {
  const int tiles = (int)mind_tiles(D, H, W);
  mind_fwd_kernel<R><<<dim3((unsigned)tiles, (unsigned)N), TPB, 0, s>>>(a, b, bounds, D, H, W, d, partial);
  mind_final_kernel<<<N, TPB, 0, s>>>(partial, tiles, (long long)D * H * W, out);
}

template <int R>
void mind_bwd_launch(const float* a, const float* b, const float* bounds, const float* gout, int N, int D, int H, int W, int d,
                     float* da, float* db, float* gD, float* G, hipStream_t s) {
  const dim3 grid((unsigned)mind_tiles(D, H, W), (unsigned)N);
  const dim3 flat((unsigned)ceil_div((long long)D * H * W, TPB), (unsigned)N);
  for (int side = 0; side < 2; ++side) {
    float* dx = side ? db : da;
    if (!dx) continue;
    const float* x = side ? b : a;
    mind_cot_kernel<R><<<grid, TPB, 0, s>>>(x, side ? a : b, bounds, side, gout, D, H, W, d, gD);
    mind_boxT_kernel<R><<<grid, TPB, 0, s>>>(x, gD, D, H, W, d, G);
    mind_shiftT_kernel<<<flat, TPB, 0, s>>>(G, D, H, W, d, dx);
  }
}
}  // namespace

#define MIND_RADII(X) X(1) X(2) X(3)

/* Workspace of kmh_mind_bounds, kmh_mind_fwd and kmh_mind_bwd: two floats per tile (4 x 8 x 32 voxels) and sample for the
 * partial sums, and behind them the backward's fields of one side at a time: 12 of gD and 6 of G, 72 bytes per voxel.  0 for
 * arguments the entries refuse. */
KMH_API size_t kmh_mind_ws_bytes(int N, int D, int H, int W, int radius, int dilation) {
  if (!mind_ok(N, D, H, W, radius, dilation)) return 0;
  return mind_partial_bytes(N, D, H, W) + (size_t)(kCh + kNb) * N * D * H * W * sizeof(float);
}

/* bounds (N, 2, 2) = [a or b][lo or hi] = (1e-3, 1e3) x the sample's mean of the unclamped mean_c m_c.  ws: kmh_mind_ws_bytes
 * bytes, of which only the partials are written. */
KMH_API int kmh_mind_bounds(const float* a, const float* b, int N, int D, int H, int W, int radius, int dilation, float* bounds,
                            void* ws, void* stream) {
  if (!mind_ok(N, D, H, W, radius, dilation) || !a || !b || !bounds || !ws) return -22;
  hipStream_t s = (hipStream_t)stream;
  switch (radius) {
#define X(r) case r: mind_bounds_launch<r>(a, b, N, D, H, W, dilation, bounds, (float*)ws, s); break;
    MIND_RADII(X)
#undef X
  }
  return KMH_LAUNCH_CHECK();
}

/* a, b: (N, D, H, W) float32 contiguous, fewer than 2^31 voxels per sample; radius, dilation in 1..3; bounds (N, 2, 2) as
 * kmh_mind_bounds gives them.  out: N floats.  ws: kmh_mind_ws_bytes bytes, of which only the partials are written. */
KMH_API int kmh_mind_fwd(const float* a, const float* b, const float* bounds, int N, int D, int H, int W, int radius,
                         int dilation, float* out, void* ws, void* stream) {
  if (!mind_ok(N, D, H, W, radius, dilation) || !a || !b || !bounds || !out || !ws) return -22;
  hipStream_t s = (hipStream_t)stream;
  switch (radius) {
#define X(r) case r: mind_fwd_launch<r>(a, b, bounds, N, D, H, W, dilation, out, (float*)ws, s); break;
    MIND_RADII(X)
#undef X
  }
  return KMH_LAUNCH_CHECK();
}

/* da[n, v] = gout[n] d out[n] / d a[n, v], db likewise; either may be NULL.  ws: kmh_mind_ws_bytes bytes (everything is
 * recomputed here: nothing of the forward's is read). */
KMH_API int kmh_mind_bwd(const float* a, const float* b, const float* bounds, const float* gout, int N, int D, int H, int W,
                         int radius, int dilation, float* da, float* db, void* ws, void* stream) {
  if (!mind_ok(N, D, H, W, radius, dilation) || !a || !b || !bounds || !gout || !ws) return -22;
  if (!da && !db) return 0;
  hipStream_t s = (hipStream_t)stream;
  float* gD = (float*)((char*)ws + mind_partial_bytes(N, D, H, W));
  float* G = gD + (size_t)kCh * N * D * H * W;
  switch (radius) {
#define X(r) case r: mind_bwd_launch<r>(a, b, bounds, gout, N, D, H, W, dilation, da, db, gD, G, s); break;
    MIND_RADII(X)
#undef X
  }
  return KMH_LAUNCH_CHECK();
}
