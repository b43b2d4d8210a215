// Trilinear / nearest 3-D sampler (ATen grid_sampler_3d semantics: padding_mode=border,
// align_corners=False) forward + backward, and the MSE / Dice reductions that follow it.
// Replaces keymorph/utils.py:14-21 (align_img) and keymorph/loss_ops.py:9-63.
//
// HBM-bound: per output voxel 12 B of grid + 4 B out (+ 8 gathers per channel that hit
// L2 / Infinity Cache because neighbouring voxels sample neighbouring texels).  Each thread
// owns VPT=4 consecutive output voxels so the grid is read as 3 x 16-B loads and the output
// written as one 16-B store per channel.
//
// The source coordinate, the NaN rule, the blend and the chunk helpers are shared with warp_dice.hip: sampler_taps.h.
#include "sampler_taps.h"

namespace {

constexpr int VPT = 4;      // voxels per thread of the plain kernels

// 8 corner values of one channel plane; corners past the far border contribute 0 (weight is 0 there)
__device__ __forceinline__ void gather8(const float* __restrict__ p, const Tap& t, int D, int H, int W,
                                        float v[8]) {
  const int x1 = t.x0 + 1 < W ? t.x0 + 1 : t.x0;
  const int y1 = t.y0 + 1 < H ? t.y0 + 1 : t.y0;
  const int z1 = t.z0 + 1 < D ? t.z0 + 1 : t.z0;
  const float ox = t.x0 + 1 < W ? 1.f : 0.f, oy = t.y0 + 1 < H ? 1.f : 0.f, oz = t.z0 + 1 < D ? 1.f : 0.f;
  const long long r00 = ((long long)t.z0 * H + t.y0) * W, r01 = ((long long)t.z0 * H + y1) * W;
  const long long r10 = ((long long)z1 * H + t.y0) * W, r11 = ((long long)z1 * H + y1) * W;
  v[0] = p[r00 + t.x0];
  v[1] = p[r00 + x1] * ox;
  v[2] = p[r01 + t.x0] * oy;
  v[3] = p[r01 + x1] * (ox * oy);
  v[4] = p[r10 + t.x0] * oz;
  v[5] = p[r10 + x1] * (ox * oz);
  v[6] = p[r11 + t.x0] * (oy * oz);
  v[7] = p[r11 + x1] * (ox * oy * oz);
}

__device__ __forceinline__ void load_grid4(const float* __restrict__ grid, long long v0, long long nvox,
                                           bool full, float g[VPT][3]) {
  // 12 floats = 3 x float4 when the whole quad is in range and the sample base is 16-B aligned
  if (full) {
    const float4* gp = reinterpret_cast<const float4*>(grid + v0 * 3);
    float4 a = gp[0], b = gp[1], c = gp[2];
    g[0][0] = a.x; g[0][1] = a.y; g[0][2] = a.z;
    g[1][0] = a.w; g[1][1] = b.x; g[1][2] = b.y;
    g[2][0] = b.z; g[2][1] = b.w; g[2][2] = c.x;
    g[3][0] = c.y; g[3][1] = c.z; g[3][2] = c.w;
  } else {
#pragma unroll
    for (int i = 0; i < VPT; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) g[i][k] = (v0 + i < nvox) ? grid[(v0 + i) * 3 + k] : 0.f;
  }
}

// ----------------------------------------------------------------------------------------------
template <int MODE, bool FUSE_MSE>
__global__ __launch_bounds__(TPB) void sample_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ grid, float* __restrict__ out,
    const float* __restrict__ fixed, double* __restrict__ partial, int C, int D, int H, int W,
    long long ovox /* Do*Ho*Wo */) {
  const int n = blockIdx.y;
  const long long v0 = ((long long)blockIdx.x * TPB + threadIdx.x) * VPT;
  float acc = 0.f;
  if (v0 < ovox) {
    float g[VPT][3];
    const bool full = (v0 + VPT <= ovox) && ((ovox & 3) == 0);
    load_grid4(grid + (long long)n * ovox * 3, v0, ovox, full, g);
    Tap t[VPT];
#pragma unroll
    for (int i = 0; i < VPT; ++i) t[i] = make_tap(g[i][0], g[i][1], g[i][2], D, H, W);
    const long long plane = (long long)D * H * W;
    for (int c = 0; c < C; ++c) {
      const float* p = x + ((long long)n * C + c) * plane;
      float o[VPT];
#pragma unroll
      for (int i = 0; i < VPT; ++i) {
        if (MODE == 0) {
          float v[8];
          gather8(p, t[i], D, H, W, v);
          o[i] = blend8(v, t[i].fx, t[i].fy, t[i].fz);
        } else {
          // nearest: nearbyint (half to even) of the clipped coordinate
          int xn = (int)rintf((float)t[i].x0 + t[i].fx);
          int yn = (int)rintf((float)t[i].y0 + t[i].fy);
          int zn = (int)rintf((float)t[i].z0 + t[i].fz);
          o[i] = p[((long long)zn * H + yn) * W + xn];
        }
      }
      const long long ob = ((long long)n * C + c) * ovox + v0;
      if (FUSE_MSE) {
        if (full) {
          float4 f = *reinterpret_cast<const float4*>(fixed + ob);
          float d0 = o[0] - f.x, d1 = o[1] - f.y, d2 = o[2] - f.z, d3 = o[3] - f.w;
          acc += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
        } else {
#pragma unroll
          for (int i = 0; i < VPT; ++i)
            if (v0 + i < ovox) { float d = o[i] - fixed[ob + i]; acc += d * d; }
        }
      }
      if (full) {
        *reinterpret_cast<float4*>(out + ob) = make_float4(o[0], o[1], o[2], o[3]);
      } else {
#pragma unroll
        for (int i = 0; i < VPT; ++i)
          if (v0 + i < ovox) out[ob + i] = o[i];
      }
    }
  }
  if (FUSE_MSE) {
    __shared__ double red[TPB / kWave];
    double s = block_sum<double>((double)acc, red);
    if (threadIdx.x == 0) partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(TPB) void sample_bwd_grid_kernel(
    const float* __restrict__ x, const float* __restrict__ grid, const float* __restrict__ gout,
    float* __restrict__ dgrid, int C, int D, int H, int W, long long ovox) {
  const int n = blockIdx.y;
  const long long v0 = ((long long)blockIdx.x * TPB + threadIdx.x) * VPT;
  if (v0 >= ovox) return;
  float g[VPT][3];
  const bool full = (v0 + VPT <= ovox) && ((ovox & 3) == 0);
  load_grid4(grid + (long long)n * ovox * 3, v0, ovox, full, g);
  Tap t[VPT];
  float gx[VPT], gy[VPT], gz[VPT];
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    t[i] = make_tap(g[i][0], g[i][1], g[i][2], D, H, W);
    if (any_nan(g[i][0], g[i][1], g[i][2])) t[i].mx = t[i].my = t[i].mz = 0.f;
    gx[i] = gy[i] = gz[i] = 0.f;
  }
  const long long plane = (long long)D * H * W;
  for (int c = 0; c < C; ++c) {
    const float* p = x + ((long long)n * C + c) * plane;
    const long long ob = ((long long)n * C + c) * ovox + v0;
    float go[VPT];
    if (full) {
      float4 q = *reinterpret_cast<const float4*>(gout + ob);
      go[0] = q.x; go[1] = q.y; go[2] = q.z; go[3] = q.w;
    } else {
#pragma unroll
      for (int i = 0; i < VPT; ++i) go[i] = (v0 + i < ovox) ? gout[ob + i] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      float v[8];
      gather8(p, t[i], D, H, W, v);
      float dx, dy, dz;
      blend_grads(v, t[i].fx, t[i].fy, t[i].fz, dx, dy, dz);
      gx[i] += dx * go[i];
      gy[i] += dy * go[i];
      gz[i] += dz * go[i];
    }
  }
  float* dg = dgrid + ((long long)n * ovox + v0) * 3;
  float r[VPT * 3];
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    r[i * 3 + 0] = gx[i] * t[i].mx;
    r[i * 3 + 1] = gy[i] * t[i].my;
    r[i * 3 + 2] = gz[i] * t[i].mz;
  }
  if (full) {
    float4* d4 = reinterpret_cast<float4*>(dg);
    d4[0] = make_float4(r[0], r[1], r[2], r[3]);
    d4[1] = make_float4(r[4], r[5], r[6], r[7]);
    d4[2] = make_float4(r[8], r[9], r[10], r[11]);
  } else {
#pragma unroll
    for (int i = 0; i < VPT; ++i)
      if (v0 + i < ovox) { dg[i * 3] = r[i * 3]; dg[i * 3 + 1] = r[i * 3 + 1]; dg[i * 3 + 2] = r[i * 3 + 2]; }
  }
}

// ----------------------------------------------------------------------------------------------
// Lane-contiguous variants (sampler_taps.h: PASSES), with the corner rows as element offsets for flat 8-byte loads.
struct Tap32 : CornerRows {
  float oy, oz;             // 0 when the +1 corner is past the far border
};

__device__ __forceinline__ Tap32 make_tap32(const Tap& t, int D, int H, int W) {
  Tap32 q;
  static_cast<CornerRows&>(q) = corner_rows(t, D, H, W);
  q.oy = t.y0 + 1 < H ? 1.f : 0.f; q.oz = t.z0 + 1 < D ? 1.f : 0.f;
  return q;
}
// a lane past the end of its chunk: any valid address (nothing of it is used)
__device__ __forceinline__ void park(Tap32& q) { q.r00 = q.r01 = q.r10 = q.r11 = 0; q.sel = false; }

__device__ __forceinline__ void load_pair(const float* __restrict__ p, bool sel, float& lo, float& hi) {
  float2 r;
  __builtin_memcpy(&r, p, sizeof(float2));      // 4-byte aligned 8-byte load (global_load_dwordx2)
  lo = sel ? r.y : r.x;
  hi = sel ? 0.f : r.y;
}

__device__ __forceinline__ void gather8_pairs(const float* __restrict__ p, const Tap32& q, float v[8]) {
  load_pair(p + q.r00, q.sel, v[0], v[1]);
  load_pair(p + q.r01, q.sel, v[2], v[3]);
  load_pair(p + q.r10, q.sel, v[4], v[5]);
  load_pair(p + q.r11, q.sel, v[6], v[7]);
  v[2] *= q.oy; v[3] *= q.oy; v[4] *= q.oz; v[5] *= q.oz;
  v[6] *= q.oy * q.oz; v[7] *= q.oy * q.oz;
}

// FUSE_GRAD (with FUSE_MSE): the loss is mean((out - fixed)^2), whose cotangent 2 (out - fixed) / count is known right
// here, so the same pass also produces d(loss)/d(grid) -- the rows of the staged grid are overwritten with it and written
// out like the grid came in.  One launch and 36 B per voxel instead of three (warp, MSE backward, grid backward) and 68.
template <int MODE, bool FUSE_MSE, bool FUSE_GRAD = false>
__global__ __launch_bounds__(TPB) void sample_fwd_lc_kernel(
    const float* __restrict__ x, const float* __restrict__ grid, float* __restrict__ out,
    const float* __restrict__ fixed, double* __restrict__ partial, int C, int D, int H, int W, long long ovox,
    float* __restrict__ dgrid = nullptr, float gcoef = 0.f /* 2 / (N C voxels) */) {
  __shared__ __attribute__((aligned(16))) float sg[TPB * PASSES * 3];
  const int n = blockIdx.y, tid = threadIdx.x;
  // (one contiguous chunk range per XCD -- xcd_remap of the block index -- measured slower: DESIGN.md section 8, round 4)
  const long long vb = (long long)blockIdx.x * (TPB * PASSES);
  const int cnt = chunk_count(ovox, vb);
  stage_rows(grid + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
  __syncthreads();
  const long long plane = (long long)D * H * W;
  constexpr int ILP = 2;       // voxels whose 4 pair-gathers are in flight together; 2 keeps the kernel at ~64 VGPRs
  float acc = 0.f;
#pragma unroll 1
  for (int j0 = 0; j0 < PASSES; j0 += ILP) {
    Tap t[ILP];
    Tap32 q[ILP];
    int near[ILP];
#pragma unroll
    for (int u = 0; u < ILP; ++u) {
      const int l = tid + (j0 + u) * TPB;             // lane-contiguous: voxel vb + l
      t[u] = make_tap(sg[l * 3], sg[l * 3 + 1], sg[l * 3 + 2], D, H, W);
      q[u] = make_tap32(t[u], D, H, W);
      if (l >= cnt) park(q[u]);
      near[u] = 0;
      if (MODE != 0 && l < cnt) {
        const int xn = (int)rintf((float)t[u].x0 + t[u].fx), yn = (int)rintf((float)t[u].y0 + t[u].fy),
                  zn = (int)rintf((float)t[u].z0 + t[u].fz);
        near[u] = (zn * H + yn) * W + xn;
      }
    }
    float ggx[ILP], ggy[ILP], ggz[ILP];
#pragma unroll
    for (int u = 0; u < ILP; ++u) ggx[u] = ggy[u] = ggz[u] = 0.f;
    for (int c = 0; c < C; ++c) {
      const float* p = x + ((long long)n * C + c) * plane;
      const long long ob = ((long long)n * C + c) * ovox + vb;
      float o[ILP], fv[ILP];
      if (FUSE_MSE) {
#pragma unroll
        for (int u = 0; u < ILP; ++u) fv[u] = (tid + (j0 + u) * TPB < cnt) ? fixed[ob + tid + (j0 + u) * TPB] : 0.f;
      }
      if (MODE == 0) {
        float v[ILP][8];
#pragma unroll
        for (int u = 0; u < ILP; ++u) gather8_pairs(p, q[u], v[u]);
#pragma unroll
        for (int u = 0; u < ILP; ++u) o[u] = blend8(v[u], t[u].fx, t[u].fy, t[u].fz);
        if (FUSE_GRAD) {
#pragma unroll
          for (int u = 0; u < ILP; ++u) {
            float dx, dy, dz;
            blend_grads(v[u], t[u].fx, t[u].fy, t[u].fz, dx, dy, dz);
            const float go = (tid + (j0 + u) * TPB < cnt) ? (o[u] - fv[u]) * gcoef : 0.f;
            ggx[u] += dx * go; ggy[u] += dy * go; ggz[u] += dz * go;
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < ILP; ++u) o[u] = p[near[u]];
      }
#pragma unroll
      for (int u = 0; u < ILP; ++u) {
        const int l = tid + (j0 + u) * TPB;
        if (l < cnt) {
          if (FUSE_MSE) { const float d = o[u] - fv[u]; acc += d * d; }
          if (out) out[ob + l] = o[u];
        }
      }
    }
    if (FUSE_GRAD) {
#pragma unroll
      for (int u = 0; u < ILP; ++u)
        grad_row_out(sg, tid + (j0 + u) * TPB, ggx[u], ggy[u], ggz[u], t[u].mx, t[u].my, t[u].mz);
    }
  }
  if (FUSE_GRAD) {
    __syncthreads();
    unstage_rows(dgrid + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
  }
  if (FUSE_MSE) {
    __shared__ double red[TPB / kWave];
    double s = block_sum<double>((double)acc, red);
    if (threadIdx.x == 0) partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(TPB) void sample_bwd_grid_lc_kernel(
    const float* __restrict__ x, const float* __restrict__ grid, const float* __restrict__ gout,
    float* __restrict__ dgrid, int C, int D, int H, int W, long long ovox) {
  __shared__ __attribute__((aligned(16))) float sg[TPB * PASSES * 3];
  constexpr int ILP = 2;                   // voxels whose 4 pair-gathers are in flight together (ILP = 1: 151 us, 2: 138 us)
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long vb = (long long)blockIdx.x * (TPB * PASSES);
  const int cnt = chunk_count(ovox, vb);
  stage_rows(grid + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
  __syncthreads();
  const long long plane = (long long)D * H * W;
  // each lane turns its own rows of sg from grid coordinates into grid gradients, ILP rows at a time
#pragma unroll 1
  for (int j0 = 0; j0 < PASSES; j0 += ILP) {
    Tap t[ILP];
    Tap32 q[ILP];
    float gx[ILP], gy[ILP], gz[ILP];
#pragma unroll
    for (int u = 0; u < ILP; ++u) {
      const int l = tid + (j0 + u) * TPB;
      t[u] = make_tap(sg[l * 3], sg[l * 3 + 1], sg[l * 3 + 2], D, H, W);
      q[u] = make_tap32(t[u], D, H, W);
      if (l >= cnt) park(q[u]);
      gx[u] = gy[u] = gz[u] = 0.f;
    }
    for (int c = 0; c < C; ++c) {
      const float* p = x + ((long long)n * C + c) * plane;
      const long long ob = ((long long)n * C + c) * ovox + vb;
      float v[ILP][8], go[ILP];
#pragma unroll
      for (int u = 0; u < ILP; ++u) {
        const int l = tid + (j0 + u) * TPB;
        go[u] = l < cnt ? gout[ob + l] : 0.f;
        gather8_pairs(p, q[u], v[u]);
      }
#pragma unroll
      for (int u = 0; u < ILP; ++u) {
        float dx, dy, dz;
        blend_grads(v[u], t[u].fx, t[u].fy, t[u].fz, dx, dy, dz);
        gx[u] += dx * go[u]; gy[u] += dy * go[u]; gz[u] += dz * go[u];
      }
    }
#pragma unroll
    for (int u = 0; u < ILP; ++u) grad_row_out(sg, tid + (j0 + u) * TPB, gx[u], gy[u], gz[u], t[u].mx, t[u].my, t[u].mz);
  }
  __syncthreads();
  unstage_rows(dgrid + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
}

// Multi-channel bilinear warp (align_img of a one-hot segmentation, keymorph/utils.py:14-21 under
// scripts/pairwise_register_eval.py).  sample_fwd_lc_kernel walks 4-row x 256 chunks of ONE output plane and pays one memory
// round trip per (sub-pass, channel): 1.8 ms at 14 x 256^3 (1.1 TB/s; PMC: L2 hit rate 37 %, FETCH_SIZE 3.4x the algorithmic
// reads).  Here a workgroup owns a compact 16 x 8 x 8 output TILE -- under a rotation about any axis its source box stays
// ~22 x 18 x 17, where a 32 x 8 x 4 tile's does not fit the LDS box below (measured: 1.06 vs 1.73 ms on bench.py's
// three-axis affine grid, 0.94 vs 0.88 ms on a one-axis rotation) -- tiles are walked x-fastest in one contiguous range per
// XCD, and the machinery of the Dice kernels does the rest: persistent blocks, the next tile's grid rows prefetched into
// registers, 32-bit corner offsets, buffer loads, range-checked stores.
// The blend is blend8 on the same corner values (a corner past the far border has weight 0 there and reads 0 here):
// bit-equal to the single-channel kernel (tests/test_ops_gpu.py::test_multichannel_sampler_equals_per_channel).
constexpr int MT_X = 16, MT_Y = 8, MT_Z = 8;
static_assert(MT_X * MT_Y * MT_Z == TPB * PASSES && (MT_X & (MT_X - 1)) == 0 && (MT_Y & (MT_Y - 1)) == 0 && MT_X % 4 == 0,
              "1024-voxel tiles with power-of-two sides");
constexpr int MT_LX = __builtin_ctz(MT_X), MT_LXY = __builtin_ctz(MT_X * MT_Y);
constexpr int MT_Q4 = MT_X * 3 / 4;                  // 16-byte pieces of a tile row of the grid
// tile voxel l = tid + pass * 256  ->  (l & (MT_X-1), (l >> MT_LX) & (MT_Y-1), l >> MT_LXY)
// BOX path: the tile's corners live in a small source box (identity-like grid: 34 x 10 x 5); per channel the workgroup copies
// that box into LDS with coalesced 4-byte loads (prefetched into registers one channel ahead) and the 8 corners of a voxel
// come from four ds_read2_b32 instead of four 64-lane gathers of 4-byte-aligned 8-byte pairs (10 % faster than the global
// gathers of the same tile walk, 0.88 vs 0.97 ms at 14 x 256^3; with loads and stores compiled out the kernel still takes
// 0.41 ms: ~25 instructions per voxel and channel at 3 waves per SIMD are what bounds it, not the memory system).
// A tile whose box does not fit (strong zoom-out / shear: more than MB_PITCH columns or MB_ROWS rows) takes the global gathers.
constexpr int MB_PITCH = MT_X + 8, MB_CAP = 6144;

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(v, m, 64); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(v, m, 64); v = o > v ? o : v; }
  return v;
}

struct BoxGeom { int x0, y0, z0, nx, ny, nrows; };
constexpr int MB_RPS = TPB / MB_PITCH;               // 6 box rows copied per step (240 of the 256 threads)
constexpr int MB_KMAX = 26;                          // steps: up to 156 rows
constexpr int MB_ROWS = MB_CAP / MB_PITCH;           // 153

// one channel loop of a tile through the LDS box; KR = box rows per thread (registers of the one-channel-ahead prefetch).
// rowoff[r]: byte offset (inside a channel plane) of box row r's first float, or >= plane_bytes for rows past the box.
// (16-byte copies -- 7 instead of 26 loads per thread and channel -- measured no faster: the kernel is bound by the ~25
// instructions per voxel and channel of the gather + blend + store, not by the copy.)
template <int KR>
__device__ __forceinline__ void mc_box_channels(const float* __restrict__ x, float* __restrict__ out, int n, int C,
                                                long long plane, long long ovox, unsigned plane_bytes, unsigned out_bytes,
                                                float* box, const unsigned* rowoff, int tid, const BoxGeom& g, int W,
                                                const unsigned (&lo)[PASSES][4], const float (&fr)[PASSES][3],
                                                const unsigned (&oo)[PASSES]) {
  const int r0 = tid / MB_PITCH, ix = tid - r0 * MB_PITCH;
  // idle lanes, columns past the box and the column past the volume's last one read 0 (x0 = W - 1: the pair's second value
  // has weight fx = 0, and the next row's first voxel there could turn 0 * Inf into a NaN the reference does not produce)
  const unsigned colb = (r0 < MB_RPS && ix < g.nx && g.x0 + ix < W) ? 4u * (unsigned)ix : plane_bytes;
  float R[KR];
  auto prefetch = [&](int c) {
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(x + ((long long)n * C + c) * plane, plane_bytes);
#pragma unroll
    for (int k = 0; k < KR; ++k)
      R[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, (int)(rowoff[r0 + k * MB_RPS] + colb), 0, 0));
  };
  prefetch(0);
#pragma unroll 1
  for (int c = 0; c < C; ++c) {
    __syncthreads();                                  // the previous channel's gathers are done
    if (r0 < MB_RPS) {
#pragma unroll
      for (int k = 0; k < KR; ++k) box[tid + k * (MB_RPS * MB_PITCH)] = R[k];
    }
    __syncthreads();
    if (c + 1 < C) prefetch(c + 1);                   // the next channel's box: in flight under this channel's gathers
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(out + ((long long)n * C + c) * ovox, out_bytes);
#pragma unroll
    for (int u = 0; u < PASSES; ++u) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float2 r;
        __builtin_memcpy(&r, box + lo[u][k], sizeof(float2));      // 4-byte aligned pair: ds_read2_b32
        v[2 * k] = r.x; v[2 * k + 1] = r.y;
      }
      const float o = blend8(v, fr[u][0], fr[u][1], fr[u][2]);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o), ro, (int)oo[u], 0, 0);      // dropped past the volume
    }
  }
}

template <int MC_ILP>
__global__ __launch_bounds__(TPB, 3) void sample_fwd_mc_kernel(
    const float* __restrict__ x, const float* __restrict__ grid, float* __restrict__ out, int C, int D, int H, int W,
    int Do, int Ho, int Wo, int ntx, int nty, int ntile, int use_box) {
  __shared__ __attribute__((aligned(16))) float sg[TPB * PASSES * 3];
  __shared__ __attribute__((aligned(16))) float box[MB_KMAX * MB_RPS * MB_PITCH];
  __shared__ unsigned rowoff[MB_KMAX * MB_RPS + MB_RPS];
  __shared__ int sred[TPB / kWave][6];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long plane = (long long)D * H * W, ovox = (long long)Do * Ho * Wo;
  const unsigned plane_bytes = (unsigned)(plane * 4), out_bytes = (unsigned)(ovox * 4);
  const float* gbase = grid + (long long)n * ovox * 3;
  const int lx = tid & (MT_X - 1), ly = (tid >> MT_LX) & (MT_Y - 1), lz = tid >> MT_LXY, dzp = TPB >> MT_LXY;      // pass u: plane lz + u * dzp
  struct TileAt { int tx, ty, tz; };
  auto tile_at = [&](int tile) { return TileAt{tile % ntx, (tile / ntx) % nty, tile / (ntx * nty)}; };      // x-fastest
  // the tile's 32 grid rows (96 floats each) as 768 float4: thread t owns numbers t, t + 256, t + 512
  auto row4 = [&](int tile, int idx) -> float4 {       // (zeros for the rows of a tile that ends past the volume in y or z)
    const auto [tx, ty, tz] = tile_at(tile);
    const int r = idx / MT_Q4, q4 = idx - r * MT_Q4;
    const int z = tz * MT_Z + r / MT_Y, y = ty * MT_Y + (r & (MT_Y - 1));
    const float* p = gbase + (((long long)z * Ho + y) * Wo + tx * MT_X) * 3 + q4 * 4;
    return z < Do && y < Ho ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto tile_fast = [&](int tile) -> bool {       // whole 32-voxel rows, 16-byte aligned: Wo % 4 == 0 and the tile inside in x
    const int tx = tile_at(tile).tx;
    return (Wo & 3) == 0 && tx * MT_X + MT_X <= Wo && ((reinterpret_cast<unsigned long long>(gbase) & 15) == 0);
  };
  auto fetch = [&](int tile, GridRows& g) { g.a = row4(tile, tid); g.b = row4(tile, tid + TPB); g.c = row4(tile, tid + 2 * TPB); };
  const ChunkWalk cw = chunk_walk(blockIdx.x, gridDim.x, ntile);
  int tile = cw.cur;
  GridRows nxt = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  bool nfast = false;
  if (tile < cw.end) {
    nfast = tile_fast(tile);
    if (nfast) fetch(tile, nxt);
  }
#pragma unroll 1
  for (; tile < cw.end; tile += cw.step) {
    const auto [tx, ty, tz] = tile_at(tile);
    const int x0 = tx * MT_X, y0 = ty * MT_Y, z0 = tz * MT_Z;
    __syncthreads();                                  // the previous tile's readers of sg / box are done
    if (nfast) {
      float4* d4 = reinterpret_cast<float4*>(sg);
      d4[tid] = nxt.a; d4[tid + TPB] = nxt.b; d4[tid + 2 * TPB] = nxt.c;
    } else {                                          // edge tile / unaligned rows: element by element, zeros outside
      for (int e = tid; e < TPB * PASSES * 3; e += TPB) {
        const int l = e / 3, k = e - l * 3;
        const int xx = x0 + (l & (MT_X - 1)), yy = y0 + ((l >> MT_LX) & (MT_Y - 1)), zz = z0 + (l >> MT_LXY);
        sg[e] = (xx < Wo && yy < Ho && zz < Do) ? gbase[(((long long)zz * Ho + yy) * Wo + xx) * 3 + k] : 0.f;
      }
    }
    __syncthreads();
    {                                                 // the next tile's rows: in flight under this tile's gathers
      const int t2 = tile + cw.step;
      if (t2 < cw.end) {
        nfast = tile_fast(t2);
        if (nfast) fetch(t2, nxt);
      }
    }
    const bool in_xy = x0 + lx < Wo && y0 + ly < Ho;
    // byte offset of the lane's output voxel of plane z inside a channel plane; a dead lane's store is dropped by the range check
    auto out_off = [&](bool live, int z) -> unsigned {
      return live ? 4u * (unsigned)(((long long)z * Ho + (y0 + ly)) * Wo + (x0 + lx)) : 0xfffffffcu;
    };
    bool boxed = false;
    if (use_box) {
      // corners of the lane's 4 voxels (one per tile plane) and the box that holds every live corner of the tile
      int cx[PASSES], cy[PASSES], cz[PASSES], cy1[PASSES], cz1[PASSES];
      float fr[PASSES][3];
      unsigned oo[PASSES];
      int mn[3] = {1 << 30, 1 << 30, 1 << 30}, mx[3] = {-1, -1, -1};
#pragma unroll
      for (int u = 0; u < PASSES; ++u) {
        const int l = tid + u * TPB, z = z0 + lz + u * dzp;
        const Tap t = make_tap(sg[l * 3], sg[l * 3 + 1], sg[l * 3 + 2], D, H, W);
        const bool live = in_xy && z < Do;
        cx[u] = t.x0; cy[u] = t.y0; cz[u] = t.z0;      // (the pair of x0 = W - 1 takes a zero from past the box's last column)
        const CornerRows cr = corner_rows(t, D, H, W);
        cy1[u] = cr.y1; cz1[u] = cr.z1;
        fr[u][0] = t.fx; fr[u][1] = t.fy; fr[u][2] = t.fz;
        oo[u] = out_off(live, z);
        if (live) {
          mn[0] = cx[u] < mn[0] ? cx[u] : mn[0]; mx[0] = cx[u] + 1 > mx[0] ? cx[u] + 1 : mx[0];
          mn[1] = cy[u] < mn[1] ? cy[u] : mn[1]; mx[1] = cy1[u] > mx[1] ? cy1[u] : mx[1];
          mn[2] = cz[u] < mn[2] ? cz[u] : mn[2]; mx[2] = cz1[u] > mx[2] ? cz1[u] : mx[2];
        } else {            // a dead lane's corners sit on the box origin (filled in below)
          cx[u] = cy[u] = cz[u] = cy1[u] = cz1[u] = -1;
        }
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) { mn[k] = wave_min_i(mn[k]); mx[k] = wave_max_i(mx[k]); }
      if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { sred[tid >> 6][k] = mn[k]; sred[tid >> 6][3 + k] = mx[k]; }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int w = 0; w < TPB / kWave; ++w) {
          mn[k] = sred[w][k] < mn[k] ? sred[w][k] : mn[k];
          mx[k] = sred[w][3 + k] > mx[k] ? sred[w][3 + k] : mx[k];
        }
      }
      BoxGeom g;
      g.x0 = mn[0]; g.y0 = mn[1]; g.z0 = mn[2];
      g.nx = mx[0] - mn[0] + 1; g.ny = mx[1] - mn[1] + 1;
      g.nrows = g.ny * (mx[2] - mn[2] + 1);
      boxed = g.nx <= MB_PITCH && g.nrows <= MB_ROWS;      // uniform
      if (boxed) {
        unsigned lo[PASSES][4];
#pragma unroll
        for (int u = 0; u < PASSES; ++u) {
          const bool dead = cx[u] < 0;
          const int ax = dead ? 0 : cx[u] - g.x0, ay = dead ? 0 : cy[u] - g.y0, ay1 = dead ? 0 : cy1[u] - g.y0;
          const int az = dead ? 0 : cz[u] - g.z0, az1 = dead ? 0 : cz1[u] - g.z0;
          lo[u][0] = (unsigned)((az * g.ny + ay) * MB_PITCH + ax); lo[u][1] = (unsigned)((az * g.ny + ay1) * MB_PITCH + ax);
          lo[u][2] = (unsigned)((az1 * g.ny + ay) * MB_PITCH + ax); lo[u][3] = (unsigned)((az1 * g.ny + ay1) * MB_PITCH + ax);
        }
        // row offsets of the box (rows past it: out of range)
        for (int r = tid; r < MB_KMAX * MB_RPS + MB_RPS; r += TPB) {
          const int iz = (int)(((float)r + 0.5f) / (float)g.ny), iy = r - iz * g.ny;      // exact: r, ny < 2^10
          rowoff[r] = r < g.nrows ? 4u * (unsigned)(((g.z0 + iz) * H + (g.y0 + iy)) * W + g.x0) : plane_bytes;
        }
        __syncthreads();
        if (g.nrows <= 10 * MB_RPS)
          mc_box_channels<10>(x, out, n, C, plane, ovox, plane_bytes, out_bytes, box, rowoff, tid, g, W, lo, fr, oo);
        else if (g.nrows <= 18 * MB_RPS)
          mc_box_channels<18>(x, out, n, C, plane, ovox, plane_bytes, out_bytes, box, rowoff, tid, g, W, lo, fr, oo);
        else
          mc_box_channels<MB_KMAX>(x, out, n, C, plane, ovox, plane_bytes, out_bytes, box, rowoff, tid, g, W, lo, fr, oo);
      }
    }
    if (boxed) continue;
#pragma unroll 1
    for (int j0 = 0; j0 < PASSES; j0 += MC_ILP) {
      TapB q[MC_ILP];
      unsigned oo[MC_ILP];
#pragma unroll
      for (int u = 0; u < MC_ILP; ++u) {
        const int l = tid + (j0 + u) * TPB;
        const int z = z0 + lz + (j0 + u) * dzp;
        q[u] = make_tapb(make_tap(sg[l * 3], sg[l * 3 + 1], sg[l * 3 + 2], D, H, W), D, H, W);
        const bool live = in_xy && z < Do;
        oo[u] = out_off(live, z);
        if (!live) park(q[u], plane_bytes);
      }
#pragma unroll 2
      for (int c = 0; c < C; ++c) {
        const __amdgpu_buffer_rsrc_t rx = make_rsrc(x + ((long long)n * C + c) * plane, plane_bytes);
        const __amdgpu_buffer_rsrc_t ro = make_rsrc(out + ((long long)n * C + c) * ovox, out_bytes);
        float v[MC_ILP][8];
#pragma unroll
        for (int u = 0; u < MC_ILP; ++u) gather8_b(rx, q[u], v[u]);
#pragma unroll
        for (int u = 0; u < MC_ILP; ++u) {
          const float o = blend8(v[u], q[u].fx, q[u].fy, q[u].fz);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o), ro, (int)oo[u], 0, 0);
        }
      }
    }
  }
}

// scatter-add backward wrt the sampled volume (not on the training hot path: the volumes are data;
// used by augmentation-through-images and for completeness of align_img's autograd).
__global__ __launch_bounds__(TPB) void sample_bwd_input_kernel(
    const float* __restrict__ grid, const float* __restrict__ gout, float* __restrict__ dx, int C, int D,
    int H, int W, long long ovox) {
  const int n = blockIdx.y;
  const long long v = (long long)blockIdx.x * TPB + threadIdx.x;
  if (v >= ovox) return;
  const float* gp = grid + ((long long)n * ovox + v) * 3;
  if (any_nan(gp[0], gp[1], gp[2])) return;             // no gradient from a voxel with a NaN coordinate (as ATen)
  Tap t = make_tap(gp[0], gp[1], gp[2], D, H, W);
  const long long plane = (long long)D * H * W;
  const float wx[2] = {1.f - t.fx, t.fx}, wy[2] = {1.f - t.fy, t.fy}, wz[2] = {1.f - t.fz, t.fz};
  for (int c = 0; c < C; ++c) {
    const float go = gout[((long long)n * C + c) * ovox + v];
    float* p = dx + ((long long)n * C + c) * plane;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int xx = t.x0 + (k & 1), yy = t.y0 + ((k >> 1) & 1), zz = t.z0 + (k >> 2);
      if (xx < W && yy < H && zz < D)
        atomicAdd(p + ((long long)zz * H + yy) * W + xx, go * wx[k & 1] * wy[(k >> 1) & 1] * wz[k >> 2]);
    }
  }
}

// a block of the plain kernels takes TPB * VPT voxels, a block of the lane-contiguous ones TPB * PASSES
static_assert(VPT == PASSES, "the plain and the lane-contiguous kernels share one launch grid");
static inline dim3 sample_grid(long long ovox, int N) { return dim3(ceil_div(ovox, (long long)CHUNK), N); }

}  // namespace

KMH_API int kmh_abi_version(void) { return 1; }

KMH_API size_t kmh_reduce_ws_bytes(void) { return (size_t)65536 * sizeof(double) * 3; }

KMH_API int kmh_grid_sample3d_fwd(const float* x, const float* grid, float* out, int N, int C, int D, int H,
                                  int W, int Do, int Ho, int Wo, int mode, void* stream) {
  if (N <= 0 || C <= 0) return -22;
  const long long ovox = (long long)Do * Ho * Wo;
  const dim3 g = sample_grid(ovox, N);
  hipStream_t s = (hipStream_t)stream;
  // C >= 2, bilinear: the persistent tiled multi-channel kernel (KMH_SAMPLER_MC=0: the lc kernel; KMH_SAMPLER_MC_MINC=1: also C = 1)
  static const int mc = env_int("KMH_SAMPLER_MC", 4);
  static const int minc = env_int("KMH_SAMPLER_MC_MINC", 2);
  if (mode == 0 && C >= minc && mc && lane_contiguous_ok(D, H, W) && (long long)D * H * W < (1ll << 30) && ovox < (1ll << 30)) {
    const int ntx = (Wo + MT_X - 1) / MT_X, nty = (Ho + MT_Y - 1) / MT_Y, ntz = (Do + MT_Z - 1) / MT_Z;
    const long long nt = (long long)ntx * nty * ntz;
    if (nt < (1ll << 30)) {
      static const int capa = env_int("KMH_MC_BLOCKS", 2048);   // ~ resident blocks of the chip
      const dim3 gm((unsigned)persistent_blocks(capa, N, nt), N);
      static const int use_box = env_int("KMH_SAMPLER_BOX", 1);
      if (mc == 2) sample_fwd_mc_kernel<2><<<gm, TPB, 0, s>>>(x, grid, out, C, D, H, W, Do, Ho, Wo, ntx, nty, (int)nt, use_box);
      else sample_fwd_mc_kernel<4><<<gm, TPB, 0, s>>>(x, grid, out, C, D, H, W, Do, Ho, Wo, ntx, nty, (int)nt, use_box);
      return KMH_LAUNCH_CHECK();
    }
  }
  if (lane_contiguous_ok(D, H, W)) {
    if (mode == 0)
      sample_fwd_lc_kernel<0, false><<<g, TPB, 0, s>>>(x, grid, out, nullptr, nullptr, C, D, H, W, ovox);
    else
      sample_fwd_lc_kernel<1, false><<<g, TPB, 0, s>>>(x, grid, out, nullptr, nullptr, C, D, H, W, ovox);
  } else if (mode == 0) {
    sample_fwd_kernel<0, false><<<g, TPB, 0, s>>>(x, grid, out, nullptr, nullptr, C, D, H, W, ovox);
  } else {
    sample_fwd_kernel<1, false><<<g, TPB, 0, s>>>(x, grid, out, nullptr, nullptr, C, D, H, W, ovox);
  }
  return KMH_LAUNCH_CHECK();
}

KMH_API int kmh_warp_mse_fwd(const float* x, const float* grid, const float* fixed, float* out,
                             float* out_loss, int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                             void* ws, void* stream) {
  const long long ovox = (long long)Do * Ho * Wo;
  const dim3 g = sample_grid(ovox, N);
  if ((long long)g.x * g.y > 65536 * 3) return -22;
  hipStream_t s = (hipStream_t)stream;
  if (lane_contiguous_ok(D, H, W)) {
    sample_fwd_lc_kernel<0, true><<<g, TPB, 0, s>>>(x, grid, out, fixed, (double*)ws, C, D, H, W, ovox);
  } else {
    sample_fwd_kernel<0, true><<<g, TPB, 0, s>>>(x, grid, out, fixed, (double*)ws, C, D, H, W, ovox);
  }
  return kmh_launch_finalize_mean((const double*)ws, (int)(g.x * g.y), 1.0 / ((double)N * C * (double)ovox), out_loss, s);
}

namespace {
// dgrid *= g[0] unless g[0] == 1 (the usual loss.backward()): the fused pass already wrote d(loss)/d(grid)
__global__ __launch_bounds__(TPB) void scale_unless_one_kernel(float* __restrict__ a, long long n4,
                                                                const float* __restrict__ g) {
  const float s = g[0];
  if (s == 1.f) return;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n4; i += (long long)gridDim.x * TPB) {
    float4 v = reinterpret_cast<float4*>(a)[i];
    v.x *= s; v.y *= s; v.z *= s; v.w *= s;
    reinterpret_cast<float4*>(a)[i] = v;
  }
}
}  // namespace

/* Fused align_img + MSELoss + their backward with respect to the grid, for a loss that IS the mean squared error
 * (keymorph/utils.py:14-21, loss_ops.py:9-13 and autograd of both; caller scripts/train.py:146-176): one pass writes
 * out (or nothing when out == NULL), out_loss[0] and dgrid = d(out_loss)/d(grid).  Returns KMH_EINVAL (-22) when the
 * lane-contiguous kernel does not apply to the shape: the caller then uses the separate entry points. */
KMH_API int kmh_warp_mse_fwd_grad(const float* x, const float* grid, const float* fixed, float* out, float* out_loss,
                                  float* dgrid, int N, int C, int D, int H, int W, int Do, int Ho, int Wo, void* ws,
                                  void* stream) {
  const long long ovox = (long long)Do * Ho * Wo;
  const dim3 g = sample_grid(ovox, N);
  if ((long long)g.x * g.y > 65536 * 3 || !lane_contiguous_ok(D, H, W)) return -22;
  hipStream_t s = (hipStream_t)stream;
  const double cnt = (double)N * C * (double)ovox;
  sample_fwd_lc_kernel<0, true, true><<<g, TPB, 0, s>>>(x, grid, out, fixed, (double*)ws, C, D, H, W, ovox, dgrid,
                                                        (float)(2.0 / cnt));
  return kmh_launch_finalize_mean((const double*)ws, (int)(g.x * g.y), 1.0 / cnt, out_loss, s);
}

/* a (n floats, n % 4 == 0, 16-byte aligned) *= g[0], skipped on the device when g[0] == 1 */
KMH_API int kmh_scale_unless_one(float* a, long long n, const float* g, void* stream) {
  if (n & 3) return -22;
  long long nb = (n / 4 + TPB - 1) / TPB;
  if (nb > 2048) nb = 2048;
  scale_unless_one_kernel<<<(int)nb, TPB, 0, (hipStream_t)stream>>>(a, n / 4, g);
  return KMH_LAUNCH_CHECK();
}

KMH_API int kmh_grid_sample3d_bwd_grid(const float* x, const float* grid, const float* gout, float* dgrid,
                                       int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                                       void* stream) {
  const long long ovox = (long long)Do * Ho * Wo;
  const dim3 g = sample_grid(ovox, N);
  if (lane_contiguous_ok(D, H, W))
    sample_bwd_grid_lc_kernel<<<g, TPB, 0, (hipStream_t)stream>>>(x, grid, gout, dgrid, C, D, H, W, ovox);
  else
    sample_bwd_grid_kernel<<<g, TPB, 0, (hipStream_t)stream>>>(x, grid, gout, dgrid, C, D, H, W, ovox);
  return KMH_LAUNCH_CHECK();
}

KMH_API int kmh_grid_sample3d_bwd_input(const float* grid, const float* gout, float* dx, int N, int C, int D,
                                        int H, int W, int Do, int Ho, int Wo, void* stream) {
  const long long ovox = (long long)Do * Ho * Wo;
  dim3 g(ceil_div(ovox, TPB), N);
  sample_bwd_input_kernel<<<g, TPB, 0, (hipStream_t)stream>>>(grid, gout, dx, C, D, H, W, ovox);
  return KMH_LAUNCH_CHECK();
}
