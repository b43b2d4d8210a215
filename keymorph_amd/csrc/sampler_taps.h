// What more than one of the sampler units needs (sampler.hip: the sampler and the fused warp + MSE, warp_dice.hip: the fused
// warp + Dice, losses.hip: the reductions that sample nothing); anything only one of them uses stays in that file.  Every
// sampler kernel has to round identically, so the coordinate, the blend and its derivative exist once, here.
// Source coordinate (unnorm_clip): ((g + 1) * size - 1) / 2 in fp32 with every operation rounded on its own, as ATen's CPU
// grid_sampler_3d computes it -- the product is kept out of -ffp-contract=fast's fused multiply-add, because one ulp of the
// coordinate moves floor() to the neighbouring cell at lattice points (the grid gradient then takes that cell's difference)
// and flips the clamp mask at the first and last voxel centre.  Then ATen's clip_coordinates_set_grad: <= 0 -> 0 and
// >= size - 1 -> size - 1, both with a zero derivative.
// NaN coordinates: clamped to the far border (size - 1) of their axis, as ATen's forward does; a voxel with a NaN
// coordinate passes no gradient to the grid (all three components 0) nor to the volume, as ATen's backward.  So every
// coordinate that reaches floor() lies in [0, size - 1] and every corner address derived from it is inside the volume.
#pragma once
#include "common.h"
#include <cstdlib>

// mean of np partial sums -> out[0] (losses.hip); the fused warp + MSE launchers of sampler.hip end with it too
int kmh_launch_finalize_mean(const double* partial, int np, double inv_n, float* out, hipStream_t s);

namespace {

constexpr int TPB = 256;    // threads per block
// Lane-contiguous kernels (the ones the launchers use whenever W >= 2 and a channel plane has < 2^31 voxels): a workgroup owns
// a chunk of PASSES * 256 consecutive output voxels, one voxel per lane per pass, so one gather instruction covers 64
// NEIGHBOURING voxels (2-4 cache lines for a smooth grid instead of 8+), the two x-corners of a row come from ONE 8-byte load, all
// in-plane offsets are 32-bit, and the AoS grid / grid-gradient rows go through LDS so their global accesses are 16-byte coalesced.
constexpr int PASSES = 4;   // 256-voxel passes per workgroup
constexpr int CHUNK = TPB * PASSES;

// A/B switches and launch caps are read from the environment once per process (function-local statics at the call sites)
static inline int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}

static bool lane_contiguous_ok(int D, int H, int W) {
  static const bool force_old = getenv("KMH_SAMPLER_OLD") != nullptr;   // A/B switch for tools/bench_sampler.py
  return !force_old && W >= 2 && (long long)D * H * W < (1ll << 31);
}

// blocks per sample row of a PERSISTENT launch: `cap` (~ the resident blocks of the chip) shared by the N rows, a multiple
// of 8 (blockIdx.x % 8 is the XCD, see chunk_walk), at least 8, and no more than there are chunks / tiles to walk
static inline long long persistent_blocks(int cap, int N, long long work) {
  long long nb = (cap / N) & ~7;
  if (nb < 8) nb = 8;
  return nb > work ? work : nb;
}

struct Tap {
  int x0, y0, z0;        // floor corner
  float fx, fy, fz;      // fractional offsets
  float mx, my, mz;      // d(ix)/d(gx) incl. clamp mask (W/2 or 0)
};

__device__ __forceinline__ float unnorm_clip(float g, int size, float& mult) {
  // ((g+1)*size-1)/2 then clip_coordinates_set_grad: borders count as out of bounds for the grad.  The product is rounded
  // on its own, as ATen's CPU kernel rounds it: under -ffp-contract=fast it would be fused into the subtraction (one
  // v_fma_f32, one rounding), and one ulp of the coordinate moves floor() to the neighbouring cell at lattice points and
  // flips the clamp mask at the first and last voxel centre.  The empty asm makes the product opaque, so it stays a
  // v_mul_f32 followed by a v_add_f32 (__fmul_rn and `#pragma clang fp contract(off)` are both contracted anyway).
  float p = (g + 1.f) * (float)size;
  asm volatile("" : "+v"(p));
  const float v = (p - 1.f) * 0.5f;
  const float hi = (float)(size - 1);
  if (v <= 0.f) { mult = 0.f; return 0.f; }
  if (!(v < hi)) { mult = 0.f; return hi; }      // v >= hi, and NaN: the far border (ATen's clip_coordinates)
  mult = 0.5f * (float)size;
  return v;
}

// a voxel with a NaN coordinate passes no gradient at all (ATen's backward finds none of its corners inside the volume).
// Tested where the gradient is written, on the coordinates still in registers or LDS there (not in make_tap: keeping the
// flag live across the channel loop costs the fused warp + MSE + gradient kernel 6 VGPRs and a wave per SIMD).
__device__ __forceinline__ bool any_nan(float gx, float gy, float gz) { return gx != gx || gy != gy || gz != gz; }

__device__ __forceinline__ Tap make_tap(float gx, float gy, float gz, int D, int H, int W) {
  Tap t;
  float ix = unnorm_clip(gx, W, t.mx);
  float iy = unnorm_clip(gy, H, t.my);
  float iz = unnorm_clip(gz, D, t.mz);
  float fx0 = floorf(ix), fy0 = floorf(iy), fz0 = floorf(iz);
  t.x0 = (int)fx0; t.y0 = (int)fy0; t.z0 = (int)fz0;
  t.fx = ix - fx0; t.fy = iy - fy0; t.fz = iz - fz0;
  return t;
}

// the trilinear blend of 8 corner values at the fractions (fx, fy, fz)
__device__ __forceinline__ float blend8(const float v[8], float fx, float fy, float fz) {
  const float ax = 1.f - fx, ay = 1.f - fy, az = 1.f - fz;
  // same association as ATen: value * (wx*wy*wz) summed corner by corner -- as ONE explicit fma chain, so that every
  // instantiation of every sampler kernel rounds identically (left to -ffp-contract=fast the fused and the plain warp
  // differed by 1 ulp in 13 % of the voxels)
  float o = v[0] * (ax * ay * az);
  o = fmaf(v[1], fx * ay * az, o);
  o = fmaf(v[2], ax * fy * az, o);
  o = fmaf(v[3], fx * fy * az, o);
  o = fmaf(v[4], ax * ay * fz, o);
  o = fmaf(v[5], fx * ay * fz, o);
  o = fmaf(v[6], ax * fy * fz, o);
  o = fmaf(v[7], fx * fy * fz, o);
  return o;
}

// d/dix, d/diy, d/diz of the trilinear blend (ATen grid_sampler_3d_backward)
__device__ __forceinline__ void blend_grads(const float w[8], float fx, float fy, float fz, float& dx, float& dy, float& dz) {
  const float ax = 1.f - fx, ay = 1.f - fy, az = 1.f - fz;
  dx = -w[0] * (ay * az) + w[1] * (ay * az) - w[2] * (fy * az) + w[3] * (fy * az)
       - w[4] * (ay * fz) + w[5] * (ay * fz) - w[6] * (fy * fz) + w[7] * (fy * fz);
  dy = -w[0] * (ax * az) - w[1] * (fx * az) + w[2] * (ax * az) + w[3] * (fx * az)
       - w[4] * (ax * fz) - w[5] * (fx * fz) + w[6] * (ax * fz) + w[7] * (fx * fz);
  dz = -w[0] * (ax * ay) - w[1] * (fx * ay) - w[2] * (ax * fy) - w[3] * (fx * fy)
       + w[4] * (ax * ay) + w[5] * (fx * ay) + w[6] * (ax * fy) + w[7] * (fx * fy);
}

// The four x-pairs of a voxel's corners inside one channel plane, in elements (needs a plane of < 2^31 voxels): rows
// (z0, y0), (z0, y1), (z1, y0), (z1, y1) with the +1 corner clamped to the far border (fy = 0 / fz = 0 there), each
// starting at the pair's base column xb.
struct CornerRows {
  int y1, z1;
  int r00, r01, r10, r11;
  bool sel;                 // x0 is the last column: the pair was loaded one to the left
};
__device__ __forceinline__ CornerRows corner_rows(const Tap& t, int D, int H, int W) {
  CornerRows c;
  c.y1 = t.y0 + 1 < H ? t.y0 + 1 : t.y0; c.z1 = t.z0 + 1 < D ? t.z0 + 1 : t.z0;
  c.sel = t.x0 > W - 2;
  const int xb = c.sel ? W - 2 : t.x0;
  c.r00 = (t.z0 * H + t.y0) * W + xb; c.r01 = (t.z0 * H + c.y1) * W + xb;
  c.r10 = (c.z1 * H + t.y0) * W + xb; c.r11 = (c.z1 * H + c.y1) * W + xb;
  return c;
}

// Gathers go through BUFFER loads: the channel plane's base lives in a scalar descriptor that the channel loop advances
// with two scalar adds, the per-voxel part is a 32-bit byte offset computed once per chunk -- no 64-bit VALU address
// arithmetic and no address registers per load (flat loads cost this loop 2 VALU + 2 VGPRs per gather), and lanes past
// the end of a chunk read zeros from the range check instead of needing clamped addresses.
typedef unsigned kmh_u2 __attribute__((vector_size(8)));      // the builtin's own return type (an ext_vector_type
                                                              // of the same size converts by SPLATTING element 0)
struct TapB {
  unsigned o00, o01, o10, o11;   // byte offsets of the four x-pairs inside one channel plane
  bool sel;                      // x0 is the last column: the pair was loaded one to the left
  float fx, fy, fz;
};
__device__ __forceinline__ TapB make_tapb(const Tap& t, int D, int H, int W) {
  TapB q;
  const CornerRows c = corner_rows(t, D, H, W);
  q.sel = c.sel;
  q.o00 = 4u * (unsigned)c.r00; q.o01 = 4u * (unsigned)c.r01;
  q.o10 = 4u * (unsigned)c.r10; q.o11 = 4u * (unsigned)c.r11;
  q.fx = t.fx; q.fy = t.fy; q.fz = t.fz;
  return q;
}
// a lane past the end of its chunk / tile: every corner reads 0 through the range check
__device__ __forceinline__ void park(TapB& q, unsigned plane_bytes) { q.o00 = q.o01 = q.o10 = q.o11 = plane_bytes; }

__device__ __forceinline__ void pair_b(__amdgpu_buffer_rsrc_t r, unsigned off, bool sel, float& lo, float& hi) {
  const kmh_u2 v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0);
  // (scalars first: __builtin_bit_cast applied directly to a vector ELEMENT reads element 0 whatever the index -- hipcc 7.2)
  const unsigned ua = v[0], ub = v[1];
  const float a = __uint_as_float(ua), b = __uint_as_float(ub);
  lo = sel ? b : a;
  hi = sel ? 0.f : b;
}
__device__ __forceinline__ void gather8_b(__amdgpu_buffer_rsrc_t r, const TapB& q, float v[8]) {
  pair_b(r, q.o00, q.sel, v[0], v[1]);
  pair_b(r, q.o01, q.sel, v[2], v[3]);
  pair_b(r, q.o10, q.sel, v[4], v[5]);
  pair_b(r, q.o11, q.sel, v[6], v[7]);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const float* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, (int)bytes, 0x00020000);
}

// A chunk's grid rows (x, y, z per voxel) on their way to LDS and its gradient rows on their way back, 16-byte coalesced.
// chunk_count: voxels of the chunk that starts at voxel vb
__device__ __forceinline__ int chunk_count(long long ovox, long long vb) {
  return ovox - vb < CHUNK ? (int)(ovox - vb) : CHUNK;
}

struct GridRows { float4 a, b, c; };      // PASSES * 3 / 4 = 3 float4 per thread (named members: an array went to scratch)
static_assert(PASSES * 3 / 4 == 3, "GridRows holds three float4 per thread");

// the ONE statement of the fast path: a whole chunk whose rows start on a 16-byte boundary moves as 3 float4 per thread
__device__ __forceinline__ bool rows_fast(const float* p, int cnt) {
  return cnt == CHUNK && ((reinterpret_cast<unsigned long long>(p) & 15) == 0);
}
// global -> registers (fast chunks only: a ragged or unaligned one is copied element by element in commit_rows)
__device__ __forceinline__ void fetch_rows(const float* __restrict__ src, bool fast, GridRows& g, int tid) {
  if (fast) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
    g.a = s4[tid]; g.b = s4[tid + TPB]; g.c = s4[tid + 2 * TPB];
  }
}
// registers (or, not fast, global) -> LDS
__device__ __forceinline__ void commit_rows(const float* __restrict__ src, int cnt, bool fast, const GridRows& g, float* sg,
                                            int tid) {
  if (fast) {
    float4* d4 = reinterpret_cast<float4*>(sg);
    d4[tid] = g.a; d4[tid + TPB] = g.b; d4[tid + 2 * TPB] = g.c;
  } else {
    for (int e = tid; e < cnt * 3; e += TPB) sg[e] = src[e];
  }
}
// global -> LDS in one go, for the kernels that own one chunk per workgroup
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, int cnt, float* sg, int tid) {
  const bool fast = rows_fast(src, cnt);
  GridRows g;
  fetch_rows(src, fast, g, tid);
  commit_rows(src, cnt, fast, g, sg, tid);
}
// LDS -> global
__device__ __forceinline__ void unstage_rows(float* __restrict__ dst, int cnt, const float* sg, int tid) {
  if (rows_fast(dst, cnt)) {
#pragma unroll
    for (int k = 0; k < PASSES * 3 / 4; ++k)
      reinterpret_cast<float4*>(dst)[tid + k * TPB] = reinterpret_cast<const float4*>(sg)[tid + k * TPB];
  } else {
    for (int e = tid; e < cnt * 3; e += TPB) dst[e] = sg[e];
  }
}
// each lane owns its rows of sg: coordinates in, gradient out.  (mx, my, mz): d(ix)/d(gx) incl. the clamp mask
__device__ __forceinline__ void grad_row_out(float* sg, int l, float gx, float gy, float gz, float mx, float my, float mz) {
  const float k = any_nan(sg[l * 3], sg[l * 3 + 1], sg[l * 3 + 2]) ? 0.f : 1.f;
  sg[l * 3] = gx * mx * k; sg[l * 3 + 1] = gy * my * k; sg[l * 3 + 2] = gz * mz * k;
}

// Walk over a sample's chunks for a PERSISTENT launch (gridDim.x a multiple of 8): XCD k (= blockIdx.x % 8: observed
// dispatch order, used for locality only -- any placement is correct) owns ONE contiguous range of chunks and its resident
// blocks sweep it side by side, so that chunks next to each other (a rotated grid makes a 4-row chunk touch ~50 source rows
// that its neighbours touch too) meet in one L2.  Measured: the same speed and the same FETCH_SIZE as the plain strided
// walk at 2 x 14 x 256^3 (the duplicate fetches are not cross-XCD duplicates: DESIGN.md section 8); kept because it is no
// slower and the kernels need a chunk loop for the prefetch of the next chunk's grid rows anyway.
struct ChunkWalk { int cur, end, step; };
__device__ __forceinline__ ChunkWalk chunk_walk(int b, int nb, int nchunk) {
  const int NX = nb < 8 ? nb : 8;            // fewer than 8 blocks: as many ranges as blocks (every range needs an owner)
  const int xcd = b % NX, idx = b / NX;
  const int q = nchunk / NX, r = nchunk % NX;
  ChunkWalk w;
  const int lo = xcd * q + (xcd < r ? xcd : r);
  w.end = lo + q + (xcd < r ? 1 : 0);
  w.step = (nb - xcd + NX - 1) / NX;          // blocks of this launch row that sit on this XCD
  w.cur = lo + idx;
  return w;
}

}  // namespace
