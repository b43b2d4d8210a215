// What the units that treat a grid (n, D, H, W, 3) as a function of space share (fields.hip: compose and invert, svf.hip: the
// scaling-and-squaring steps of a velocity field): the voxel of a linear index and the channels-last gathers -- a grid is gathered
// channels-last, the two x-corners of a row are 24 contiguous bytes (two 12-byte buffer loads), and no (n, 3, D, H, W) copy is made.
#pragma once
#include "sampler_taps.h"

namespace {

struct Vox { int i, j, k; };
__device__ __forceinline__ Vox vox_of(long long v, int H, int W) {
  const int i = (int)(v % W);
  const long long r = v / W;
  return Vox{i, (int)(r % H), (int)(r / H)};
}

// ---- channels-last gathers -----------------------------------------------------------------------------------
typedef unsigned kmh_u3 __attribute__((vector_size(12)));
struct TapG {
  unsigned o00, o01, o10, o11;   // byte offsets of the four x-pairs inside one sample's grid (12 B per voxel)
  bool sel, last;                // last: x0 is the last column (the +1 corner has weight 0 and reads as 0);
};                               // sel: ... and the pair was loaded one voxel to the left (W >= 2)
__device__ __forceinline__ TapG make_tapg(const Tap& t, int D, int H, int W) {
  TapG q;
  const int y1 = t.y0 + 1 < H ? t.y0 + 1 : t.y0, z1 = t.z0 + 1 < D ? t.z0 + 1 : t.z0;
  q.last = t.x0 > W - 2;
  q.sel = q.last && W >= 2;
  const int xb = q.sel ? W - 2 : t.x0;
  q.o00 = 12u * (unsigned)((t.z0 * H + t.y0) * W + xb); q.o01 = 12u * (unsigned)((t.z0 * H + y1) * W + xb);
  q.o10 = 12u * (unsigned)((z1 * H + t.y0) * W + xb); q.o11 = 12u * (unsigned)((z1 * H + y1) * W + xb);
  return q;
}
// a lane with nothing to do: every corner reads 0 through the range check
__device__ __forceinline__ void park(TapG& q, unsigned bytes) { q.o00 = q.o01 = q.o10 = q.o11 = bytes; }

// one row's x-pair: lo[3], hi[3] (xyz of the two corners)
__device__ __forceinline__ void pair_g(__amdgpu_buffer_rsrc_t r, unsigned off, const TapG& q, float lo[3], float hi[3]) {
  const kmh_u3 a = __builtin_amdgcn_raw_buffer_load_b96(r, (int)off, 0, 0);
  const kmh_u3 b = __builtin_amdgcn_raw_buffer_load_b96(r, (int)(off + 12u), 0, 0);
  const unsigned a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2];      // (scalars first: sampler_taps.h)
  const float fa[3] = {__uint_as_float(a0), __uint_as_float(a1), __uint_as_float(a2)};
  const float fb[3] = {__uint_as_float(b0), __uint_as_float(b1), __uint_as_float(b2)};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    lo[c] = q.sel ? fb[c] : fa[c];
    hi[c] = q.last ? 0.f : fb[c];
  }
}
// v[c][corner], corners in blend8's order
__device__ __forceinline__ void gather8_g(__amdgpu_buffer_rsrc_t r, const TapG& q, float v[3][8]) {
  float lo[3], hi[3];
  pair_g(r, q.o00, q, lo, hi);
#pragma unroll
  for (int c = 0; c < 3; ++c) { v[c][0] = lo[c]; v[c][1] = hi[c]; }
  pair_g(r, q.o01, q, lo, hi);
#pragma unroll
  for (int c = 0; c < 3; ++c) { v[c][2] = lo[c]; v[c][3] = hi[c]; }
  pair_g(r, q.o10, q, lo, hi);
#pragma unroll
  for (int c = 0; c < 3; ++c) { v[c][4] = lo[c]; v[c][5] = hi[c]; }
  pair_g(r, q.o11, q, lo, hi);
#pragma unroll
  for (int c = 0; c < 3; ++c) { v[c][6] = lo[c]; v[c][7] = hi[c]; }
}

// a sample's grid of D*H*W voxels fits the 32-bit byte offsets of one buffer descriptor
static bool grid_fits(int D, int H, int W) { return D >= 1 && H >= 1 && W >= 1 && (long long)D * H * W * 3 < (1ll << 30); }

}  // namespace
