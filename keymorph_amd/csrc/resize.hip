// Trilinear resize of (N, C, D, H, W) / (N, D, H, W, C) fp32 volumes with PyTorch's semantics for
// F.interpolate(mode="trilinear", align_corners=False)  (reference: keymorph/model.py:576-588, the brain extractor's x2
// upsampling; notebooks/[B] Brain Extraction.ipynb resizes 256^3 -> 128^3 and back).
//
// The per-axis source coordinates are NOT computed here: the host builds one table per axis with separately rounded fp32
// operations (keymorph_amd/ops.py: _resize_axis_table) -- per output index o the two taps i0[o], i1[o] and the weight
// lam[o] -- so kernel, tests and the fp64 restatement share one definition and no FMA contraction can move a coordinate.
//   forward : y[o] = lerp_z(lerp_y(lerp_x(8 taps))), lerp(a, b, l) = a * (1 - l) + b * l, every operation rounded on its own
//   backward: the exact transpose as a GATHER.  For an input index i along an axis the outputs that reference it (i0 == i or
//             i1 == i) form one contiguous range [lo[i], hi[i]] (the host checks that when it builds the range table); the
//             kernel sums over the box of the three ranges in a fixed order: no float atomics, bitwise repeatable.
// Both kernels are one thread per element and HBM bound: forward 4 B written per output + 4 B per input read once (the eight
// taps of neighbouring outputs hit the same lines), backward the mirror image.  All tensors < 2^31 elements (launcher).
#include "common.h"

namespace {
constexpr int TPB = 256;

struct AxisTab {          // forward table of one axis: 3 * out ints = i0[out], i1[out], lam[out] (float bits)
  const int* t;
  int out;
  __device__ __forceinline__ int i0(int o) const { return t[o]; }
  __device__ __forceinline__ int i1(int o) const { return t[out + o]; }
  __device__ __forceinline__ float lam(int o) const { return __int_as_float(t[2 * out + o]); }
};

__device__ __forceinline__ float lerp_rn(float a, float b, float l) {
  return __fadd_rn(__fmul_rn(a, __fsub_rn(1.f, l)), __fmul_rn(b, l));
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// CL = false: x (NC, D, H, W), one thread per (nc, oz, oy, ox).  CL = true: x (N, D, H, W, C), one thread per (n, oz, oy, ox, c).
// The arithmetic is the same function of the same eight values in both layouts: results are bit-identical.
template <bool CL>
__global__ __launch_bounds__(TPB) void resize_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int total, int C,
                                                         int D, int H, int W, int Do, int Ho, int Wo, AxisTab tz, AxisTab ty,
                                                         AxisTab tx) {
  const int idx = blockIdx.x * TPB + threadIdx.x;
  if (idx >= total) return;
  int r = idx, c = 0;
  if (CL) { c = r % C; r /= C; }
  const int ox = r % Wo; r /= Wo;
  const int oy = r % Ho; r /= Ho;
  const int oz = r % Do; r /= Do;      // r = nc (CL = false) or n (CL = true)
  const int z0 = clampi(tz.i0(oz), D - 1), z1 = clampi(tz.i1(oz), D - 1);
  const int y0 = clampi(ty.i0(oy), H - 1), y1 = clampi(ty.i1(oy), H - 1);
  const int x0 = clampi(tx.i0(ox), W - 1), x1 = clampi(tx.i1(ox), W - 1);
  const float lz = tz.lam(oz), ly = ty.lam(oy), lx = tx.lam(ox);
  const int sx = CL ? C : 1;
  const float* p = x + (CL ? (long long)r * D * H * W * C + c : (long long)r * D * H * W);
  auto at = [&](int z, int yy, int xx) { return p[((long long)(z * H + yy) * W + xx) * sx]; };
  const float a00 = lerp_rn(at(z0, y0, x0), at(z0, y0, x1), lx);
  const float a01 = lerp_rn(at(z0, y1, x0), at(z0, y1, x1), lx);
  const float a10 = lerp_rn(at(z1, y0, x0), at(z1, y0, x1), lx);
  const float a11 = lerp_rn(at(z1, y1, x0), at(z1, y1, x1), lx);
  y[idx] = lerp_rn(lerp_rn(a00, a01, ly), lerp_rn(a10, a11, ly), lz);
}

// weight of input index i in output o along one axis: (i0 == i) * (1 - lam) + (i1 == i) * lam  (both at a clamped border)
__device__ __forceinline__ float axis_w(const AxisTab& t, int o, int i) {
  const float l = t.lam(o);
  float w = 0.f;
  if (t.i0(o) == i) w = __fsub_rn(1.f, l);
  if (t.i1(o) == i) w = __fadd_rn(w, l);
  return w;
}

// gx[i] = sum over oz in [rz.lo, rz.hi], oy, ox (in this order) of wz * wy * wx * gy[o].  r*: 2 * in ints = lo[in], hi[in]
// (lo > hi: no output references the index).  One thread per input element, same index split as the forward.
template <bool CL>
__global__ __launch_bounds__(TPB) void resize_bwd_kernel(const float* __restrict__ gy, float* __restrict__ gx, int total, int C,
                                                         int D, int H, int W, int Do, int Ho, int Wo, AxisTab tz, AxisTab ty,
                                                         AxisTab tx, const int* __restrict__ rz, const int* __restrict__ ry,
                                                         const int* __restrict__ rx) {
  const int idx = blockIdx.x * TPB + threadIdx.x;
  if (idx >= total) return;
  int r = idx, c = 0;
  if (CL) { c = r % C; r /= C; }
  const int ix = r % W; r /= W;
  const int iy = r % H; r /= H;
  const int iz = r % D; r /= D;
  const int zlo = rz[iz] < 0 ? 0 : rz[iz], zhi = rz[D + iz] > Do - 1 ? Do - 1 : rz[D + iz];
  const int ylo = ry[iy] < 0 ? 0 : ry[iy], yhi = ry[H + iy] > Ho - 1 ? Ho - 1 : ry[H + iy];
  const int xlo = rx[ix] < 0 ? 0 : rx[ix], xhi = rx[W + ix] > Wo - 1 ? Wo - 1 : rx[W + ix];
  const int sx = CL ? C : 1;
  const float* p = gy + (CL ? (long long)r * Do * Ho * Wo * C + c : (long long)r * Do * Ho * Wo);
  float acc = 0.f;
  for (int oz = zlo; oz <= zhi; ++oz) {
    const float wz = axis_w(tz, oz, iz);
    for (int oy = ylo; oy <= yhi; ++oy) {
      const float wzy = __fmul_rn(wz, axis_w(ty, oy, iy));
      const float* row = p + (long long)(oz * Ho + oy) * Wo * sx;
      for (int ox = xlo; ox <= xhi; ++ox)
        acc = __fmaf_rn(__fmul_rn(wzy, axis_w(tx, ox, ix)), row[(long long)ox * sx], acc);
    }
  }
  gx[idx] = acc;
}

bool sizes_ok(int N, int C, int D, int H, int W, int Do, int Ho, int Wo) {
  if (N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0) return false;
  const long long lim = 1ll << 31;
  return (long long)N * C * D * H * W < lim && (long long)N * C * Do * Ho * Wo < lim;
}
}  // namespace

/* x -> y resized to (Do, Ho, Wo).  channels_last == 0: (N, C, D, H, W) storage, != 0: (N, D, H, W, C).  tz / ty / tx: device
 * tables of 3 * Do / 3 * Ho / 3 * Wo ints (taps i0, taps i1, weights lam as float bits).  -22: bad sizes or >= 2^31 elements. */
KMH_API int kmh_resize_trilinear3d_fwd(const float* x, float* y, int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                                       const int* tz, const int* ty, const int* tx, int channels_last, void* stream) {
  if (!sizes_ok(N, C, D, H, W, Do, Ho, Wo) || !x || !y || !tz || !ty || !tx) return -22;
  const int total = (int)((long long)N * C * Do * Ho * Wo);
  const AxisTab az{tz, Do}, ay{ty, Ho}, ax{tx, Wo};
  hipStream_t s = (hipStream_t)stream;
  if (channels_last)
    resize_fwd_kernel<true><<<ceil_div(total, TPB), TPB, 0, s>>>(x, y, total, C, D, H, W, Do, Ho, Wo, az, ay, ax);
  else
    resize_fwd_kernel<false><<<ceil_div(total, TPB), TPB, 0, s>>>(x, y, total, C, D, H, W, Do, Ho, Wo, az, ay, ax);
  return KMH_LAUNCH_CHECK();
}

/* gx (the input's shape) = transpose of the forward applied to gy (the output's shape).  rz / ry / rx: device tables of
 * 2 * D / 2 * H / 2 * W ints (first and last output index that references each input index; first > last: none). */
KMH_API int kmh_resize_trilinear3d_bwd(const float* gy, float* gx, int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                                       const int* tz, const int* ty, const int* tx, const int* rz, const int* ry,
                                       const int* rx, int channels_last, void* stream) {
  if (!sizes_ok(N, C, D, H, W, Do, Ho, Wo) || !gy || !gx || !tz || !ty || !tx || !rz || !ry || !rx) return -22;
  const int total = (int)((long long)N * C * D * H * W);
  const AxisTab az{tz, Do}, ay{ty, Ho}, ax{tx, Wo};
  hipStream_t s = (hipStream_t)stream;
  if (channels_last)
    resize_bwd_kernel<true><<<ceil_div(total, TPB), TPB, 0, s>>>(gy, gx, total, C, D, H, W, Do, Ho, Wo, az, ay, ax, rz, ry, rx);
  else
    resize_bwd_kernel<false><<<ceil_div(total, TPB), TPB, 0, s>>>(gy, gx, total, C, D, H, W, Do, Ho, Wo, az, ay, ax, rz, ry, rx);
  return KMH_LAUNCH_CHECK();
}
