// Label maps through a sampling grid by trilinear vote (ops.warp_labels, grid_sample3d(..., "label")): what the reference's
// evaluation computes as argmax_c align_img(grid, one_hot(seg))[c] (scripts/pairwise_register_eval.py:160, 413-425), without
// the one-hot tensor -- one pass, 8 corner labels per voxel, any label ids.
// Definition (tests/labelwarp_ref.py restates it): per output voxel the corners k = 0..7 and the fractions (fx, fy, fz) of
// make_tap (sampler_taps.h: the fp32 source coordinate, the border clamp, NaN -> far border), the +1 corner of an axis clamped
// to the far border where its fraction is exactly 0, and for every label l among the 8 corner labels
//   S_l = blend8([lab_k == l], fx, fy, fz)
// -- the fma chain the sampler runs on channel l of the one-hot volume, so S_l IS that channel's sampled value, bit for bit.
// The output is the label with the largest S_l, the smallest such label on a tie (torch.argmax's first maximum; signed order
// for the signed types); the weight output is that S_l.  A label that is at no corner has S = 0 and at least one S_l is > 0
// (the eight weights sum to about 1), so the labels at the corners are the only candidates.
// Per voxel: 12 B of grid, 8 gathers of one element, one element (+ 4 B of weight) written.  The vote is VALU work in
// registers: no LDS beyond the staged grid rows, no atomics, so runs repeat bit for bit and a batch equals its samples.
#include "sampler_taps.h"

namespace {

// element width in bytes -> the element type, the type the vote compares in, and the gather
template <int B> struct Lab;
template <> struct Lab<1> {
  typedef unsigned char elem; typedef int key;         // uint8 (bool viewed): unsigned order
  static __device__ __forceinline__ key ld(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return (int)((unsigned)__builtin_amdgcn_raw_buffer_load_b8(r, (int)off, 0, 0) & 255u);
  }
};
template <> struct Lab<2> {
  typedef short elem; typedef int key;
  static __device__ __forceinline__ key ld(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return (int)(short)((unsigned)__builtin_amdgcn_raw_buffer_load_b16(r, (int)off, 0, 0) & 65535u);
  }
};
template <> struct Lab<4> {
  typedef int elem; typedef int key;
  static __device__ __forceinline__ key ld(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return (int)__builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0);
  }
};
template <> struct Lab<8> {
  typedef long long elem; typedef long long key;
  static __device__ __forceinline__ key ld(__amdgpu_buffer_rsrc_t r, unsigned off) {
    const kmh_u2 v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0);
    const unsigned lo = v[0], hi = v[1];                 // (scalars first, as pair_b)
    return (long long)(((unsigned long long)hi << 32) | lo);
  }
};

// The 8 corners of a tap as element indices inside one channel plane, in blend8's order (x fastest).  Each corner is loaded on
// its own, so the +1 corner is simply clamped (corner_rows' y1 / z1 rule, for x too): a clamped corner repeats its neighbour's
// label under a weight of exactly 0, and an axis of length 1 needs nothing special.
__device__ __forceinline__ void corner_index(const Tap& t, int D, int H, int W, unsigned idx[8]) {
  const int x1 = t.x0 + 1 < W ? t.x0 + 1 : t.x0, y1 = t.y0 + 1 < H ? t.y0 + 1 : t.y0, z1 = t.z0 + 1 < D ? t.z0 + 1 : t.z0;
  const int r00 = (t.z0 * H + t.y0) * W, r01 = (t.z0 * H + y1) * W, r10 = (z1 * H + t.y0) * W, r11 = (z1 * H + y1) * W;
  idx[0] = r00 + t.x0; idx[1] = r00 + x1; idx[2] = r01 + t.x0; idx[3] = r01 + x1;
  idx[4] = r10 + t.x0; idx[5] = r10 + x1; idx[6] = r11 + t.x0; idx[7] = r11 + x1;
}

// One workgroup owns a chunk of CHUNK consecutive output voxels of one (n, c) plane (blockIdx.y = n * C + c), one voxel per
// lane per pass as in cubic_sample_fwd_kernel; WEIGHT: the winner's S is stored too.
template <int B, bool WEIGHT>
__global__ __launch_bounds__(TPB) void warp_labels_kernel(const void* __restrict__ lab, const float* __restrict__ grid,
                                                          void* __restrict__ out, float* __restrict__ weight, int C, int D,
                                                          int H, int W, long long ovox) {
  typedef typename Lab<B>::key key;
  typedef typename Lab<B>::elem elem;
  __shared__ __attribute__((aligned(16))) float sg[TPB * PASSES * 3];
  const int nc = blockIdx.y, n = nc / C, tid = threadIdx.x;
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
  stage_rows(grid + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
  __syncthreads();
  const long long plane = (long long)D * H * W;                    // < 2^29: plane * B fits 32 bits
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(static_cast<const char*>(lab)) + (long long)nc * plane * B, 0, (int)(unsigned)(plane * B), 0x00020000);
  elem* __restrict__ o = static_cast<elem*>(out) + (long long)nc * ovox + vb;
#pragma unroll 1
  for (int j = 0; j < PASSES; ++j) {
    const int l = tid + j * TPB;                     // lane-contiguous: voxel vb + l
    if (l >= cnt) break;                             // (whole waves leave together except in the ragged last pass)
    const Tap t = make_tap(sg[l * 3], sg[l * 3 + 1], sg[l * 3 + 2], D, H, W);
    unsigned idx[8];
    corner_index(t, D, H, W, idx);
    key L[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) L[k] = Lab<B>::ld(r, idx[k] * (unsigned)B);
    bool same = true;
#pragma unroll
    for (int k = 1; k < 8; ++k) same = same && L[k] == L[0];
    key best = L[0];
    float bs = 0.f;
    if (same) {
      // one label at all 8 corners (nearly every interior voxel of a real map): it wins, and its S is the chain over 8 ones
      if (WEIGHT) {
        const float one[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
        bs = blend8(one, t.fx, t.fy, t.fz);
      }
    } else {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = L[i] == L[0] ? 1.f : 0.f;
      bs = blend8(v, t.fx, t.fy, t.fz);
#pragma unroll
      for (int k = 1; k < 8; ++k) {                  // corners with one label compute one S: a repeat changes nothing
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = L[i] == L[k] ? 1.f : 0.f;
        const float s = blend8(v, t.fx, t.fy, t.fz);
        if (s > bs || (s == bs && L[k] < best)) { bs = s; best = L[k]; }
      }
    }
    o[l] = (elem)best;
    if (WEIGHT) weight[(long long)nc * ovox + vb + l] = bs;
  }
}

template <int B>
int launch_warp_labels(const void* lab, const float* grid, void* out, float* weight, int C, int D, int H, int W, long long ovox,
                       dim3 g, hipStream_t s) {
  if (weight)
    warp_labels_kernel<B, true><<<g, TPB, 0, s>>>(lab, grid, out, weight, C, D, H, W, ovox);
  else
    warp_labels_kernel<B, false><<<g, TPB, 0, s>>>(lab, grid, out, nullptr, C, D, H, W, ovox);
  return KMH_LAUNCH_CHECK();
}

}  // namespace

/* lab (N,C,D,H,W) integer label maps of elem_bytes 1 (unsigned: uint8, bool) or 2 / 4 / 8 (signed), every channel a map of its
 * own; grid (N,Do,Ho,Wo,3) as kmh_grid_sample3d_fwd reads it.  out (N,C,Do,Ho,Wo), same element type: per voxel the label whose
 * one-hot channel the bilinear sampler would give the largest value, the smallest such label on a tie; weight (same shape,
 * float32, or NULL): that value.  -22 for a null pointer, an empty shape, another element type, a channel plane of 2^29 voxels
 * or more, or N * C > 65535. */
KMH_API int kmh_warp_labels(const void* lab, int elem_bytes, int is_signed, const float* grid, void* out, float* weight, int N,
                            int C, int D, int H, int W, int Do, int Ho, int Wo, void* stream) {
  if (!lab || !grid || !out || N < 1 || C < 1 || D < 1 || H < 1 || W < 1 || Do < 1 || Ho < 1 || Wo < 1) return -22;
  if ((long long)D * H * W >= (1ll << 29) || (long long)N * C > 65535) return -22;
  if (is_signed != (elem_bytes == 1 ? 0 : 1)) return -22;
  const long long ovox = (long long)Do * Ho * Wo;
  if ((ovox + CHUNK - 1) / CHUNK >= (1ll << 31)) return -22;
  const dim3 g((unsigned)((ovox + CHUNK - 1) / CHUNK), (unsigned)(N * C));
  hipStream_t s = (hipStream_t)stream;
  switch (elem_bytes) {
    case 1: return launch_warp_labels<1>(lab, grid, out, weight, C, D, H, W, ovox, g, s);
    case 2: return launch_warp_labels<2>(lab, grid, out, weight, C, D, H, W, ovox, g, s);
    case 4: return launch_warp_labels<4>(lab, grid, out, weight, C, D, H, W, ovox, g, s);
    case 8: return launch_warp_labels<8>(lab, grid, out, weight, C, D, H, W, ovox, g, s);
    default: return -22;
  }
}
