// The implicit identity grid and the affine map applied to it, shared by grids.hip (which writes the coordinates out) and
// warp_mi.hip (which samples at them without ever storing them): both have to round identically, because one ulp of a
// coordinate moves floor() to the neighbouring cell at lattice points (sampler_taps.h), so the expressions exist once, here.
// Likewise the voxel-centre lattice (ident) of fields.hip and bspline.hip.
#pragma once
#include "common.h"

namespace {

// torch.linspace(-1, 1, n)[i] in fp32 (symmetric evaluation: start + i*step below the midpoint,
// end - (n-1-i)*step above); an axis of one voxel is its start, -1, as linspace(-1, 1, 1) is
__device__ __forceinline__ float lin(int i, int n, float step) {
  return (i < n / 2 || n == 1) ? (-1.f + step * (float)i) : (1.f - step * (float)(n - 1 - i));
}
__host__ __device__ __forceinline__ float lin_step(int n) { return n > 1 ? 2.f / (float)(n - 1) : 0.f; }

// the voxel-centre lattice (fields.identity_grid) along an axis of size S: (2 i + 1) / S - 1, as ONE rounded division of exact integers
__device__ __forceinline__ float ident(int i, int S) { return (float)(2 * i + 1 - S) / (float)S; }

// rows of M (3 x 4) are (z, y, x) outputs; the result is flipped to the (x, y, z) order grid_sample expects.
// affine_coord is affine_grid_fwd_kernel's statement: under -ffp-contract=fast the compiler turns each row into
//   fma(m2, gx, fma(m0, gz, m1 * gy)) + m3        (one rounded product, two fused multiply-adds, one addition).
// That choice belongs to the call site: in warp_mi.hip the same expression is contracted in another order and the coordinates
// differ in the last bit.  affine_coord_chain spells out the grid kernel's chain for every other user (writing the grid kernel
// itself that way computes the same numbers but reschedules it).  tests/test_warp_mi_gpu.py holds the two together: the joint
// table built through affine_coord_chain equals, bit for bit, the one built from the grid that affine_coord wrote.
__device__ __forceinline__ void affine_coord(const float (&M)[12], float gz, float gy, float gx, float& ox, float& oy,
                                             float& oz) {
  oz = M[0] * gz + M[1] * gy + M[2] * gx + M[3];
  oy = M[4] * gz + M[5] * gy + M[6] * gx + M[7];
  ox = M[8] * gz + M[9] * gy + M[10] * gx + M[11];
}
__device__ __forceinline__ float affine_row_chain(float m0, float m1, float m2, float m3, float gz, float gy, float gx) {
  return fmaf(m2, gx, fmaf(m0, gz, m1 * gy)) + m3;
}
__device__ __forceinline__ void affine_coord_chain(const float (&M)[12], float gz, float gy, float gx, float& ox, float& oy,
                                                   float& oz) {
  oz = affine_row_chain(M[0], M[1], M[2], M[3], gz, gy, gx);
  oy = affine_row_chain(M[4], M[5], M[6], M[7], gz, gy, gx);
  ox = affine_row_chain(M[8], M[9], M[10], M[11], gz, gy, gx);
}

}  // namespace
