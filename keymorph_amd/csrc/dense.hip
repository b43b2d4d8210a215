// Dense displacement fields as a transform model (ops.displacement_grid, displacement_step_scale, displacement_update): what the
// greedy diffeomorphic driver (io.register_greedy) runs per iteration.  DESIGN.md section 8m.
//
// The parameter is PLANAR: disp (N, 3, D, H, W), channels (z, y, x), voxels of its own lattice -- fields.to_displacement's
// convention and the layout ops.gaussian_smooth works on, so the two smoothings of an iteration need no layout change.
//     u[w]    = (disp[2, w] / (W / 2), disp[1, w] / (H / 2), disp[0, w] / (D / 2))       xyz, normalised: kmh_field_from_displacement's
//                                                                                        division, so that mat == NULL is that kernel
//     grid[w] = Ids[w] + u[w]                                  or, with a matrix,
//     grid[w] = affine_grid(mat)[w] + L (s * u[w])             kmh_svf_finish_fwd's rule, expression for expression
// The backward is the per-voxel transpose: one read of dgrid, one planar write, no atomics.
//
// Step scale: out[n] = step / max_w |delta[n, :, w]|_2, 0 where the maximum is 0.  The squared norms are non-negative floats, which
// order like their bit patterns: an integer max is exact and order independent (absmax.h, svf.hip), so runs repeat bit for bit and
// a batch equals its samples.  A squared norm that is not finite does not enter.  The root and the divide are taken once, of the
// maximum.
//
// Update, the greedy composition phi <- phi o (Id + delta'):  delta' = delta * scale[n] (scale read from device memory; NULL: delta)
//     out[n, :, w] = delta'[w] + U_n(Ids[w] + delta'[w] / (S / 2))
// U_n the trilinear, border-clamped interpolant of disp[n] at the sampler's coordinate (make_tap: its clamp and NaN rule; blend8),
// gathered from the three planes as x-pairs.  Every product and sum is rounded on its own in the order written: delta * scale is
// kept out of the add's fused multiply-add.  Bit-identical to  delta' + align_img(fields.from_displacement(delta'), disp).
// Bytes per voxel: grid 12 in + 12 out; step scale 12 in; update 12 (delta) + 12 out + the 24 gathered values, which come from
// cache for a field near the identity.
#include "grid_coords.h"      // ident, lin, affine_coord_chain
#include "sampler_taps.h"
#include "field_taps.h"       // vox_of, grid_fits

namespace {

// ---- grid: forward and transpose ----------------------------------------------------------------------------------------------------
template <bool MAT>
__global__ __launch_bounds__(TPB) void disp_grid_fwd_kernel(const float* __restrict__ disp, const float* __restrict__ mat,
                                                            float* __restrict__ grid, int D, int H, int W) {
  __shared__ __attribute__((aligned(16))) float sg[CHUNK * 3];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long ovox = (long long)D * H * W;
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
  const float hx = 0.5f * (float)W, hy = 0.5f * (float)H, hz = 0.5f * (float)D;
  const float* d = disp + (long long)n * 3 * ovox + vb;
  float M[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) M[i] = MAT ? mat[n * 12 + i] : 0.f;
  const float stz = lin_step(D), sty = lin_step(H), stx = lin_step(W);
  const float sz = (float)D / (float)(D - 1), sy = (float)H / (float)(H - 1), sx = (float)W / (float)(W - 1);      // (MAT: S >= 2)
#pragma unroll
  for (int j = 0; j < PASSES; ++j) {
    const int l = tid + j * TPB;
    if (l < cnt) {
      const Vox p = vox_of(vb + l, H, W);
      if (MAT) {
        const float ux = d[2 * ovox + l] / hx, uy = d[ovox + l] / hy, uz = d[l] / hz;
        float bx, by, bz;
        affine_coord_chain(M, lin(p.k, D, stz), lin(p.j, H, sty), lin(p.i, W, stx), bx, by, bz);
        const float dz = sz * uz, dy = sy * uy, dx = sx * ux;
        sg[l * 3] = bx + fmaf(M[10], dx, fmaf(M[8], dz, M[9] * dy));
        sg[l * 3 + 1] = by + fmaf(M[6], dx, fmaf(M[4], dz, M[5] * dy));
        sg[l * 3 + 2] = bz + fmaf(M[2], dx, fmaf(M[0], dz, M[1] * dy));
      } else {      // field_from_disp_kernel's statement
        sg[l * 3] = d[2 * ovox + l] / hx + ident(p.i, W);
        sg[l * 3 + 1] = d[ovox + l] / hy + ident(p.j, H);
        sg[l * 3 + 2] = d[l] / hz + ident(p.k, D);
      }
    }
  }
  __syncthreads();
  unstage_rows(grid + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
}

// ddisp = (s * (L^T dgrid)) / (S / 2) per axis (mat == NULL: dgrid / (S / 2)), reordered to the planes (z, y, x)
__global__ __launch_bounds__(TPB) void disp_grid_bwd_kernel(const float* __restrict__ dgrid, const float* __restrict__ mat,
                                                            float* __restrict__ ddisp, int D, int H, int W) {
  __shared__ __attribute__((aligned(16))) float sg[CHUNK * 3];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long ovox = (long long)D * H * W;
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
  stage_rows(dgrid + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
  __syncthreads();
  float M[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) M[i] = mat ? mat[n * 12 + i] : 0.f;
  const float hx = 0.5f * (float)W, hy = 0.5f * (float)H, hz = 0.5f * (float)D;
  const float sz = (float)D / (float)(D - 1), sy = (float)H / (float)(H - 1), sx = (float)W / (float)(W - 1);
  float* o = ddisp + (long long)n * 3 * ovox + vb;
#pragma unroll
  for (int j = 0; j < PASSES; ++j) {
    const int l = tid + j * TPB;
    if (l < cnt) {
      float gx = sg[l * 3], gy = sg[l * 3 + 1], gz = sg[l * 3 + 2];
      if (mat) {
        const float ox = sx * fmaf(M[10], gx, fmaf(M[2], gz, M[6] * gy));
        const float oy = sy * fmaf(M[9], gx, fmaf(M[1], gz, M[5] * gy));
        const float oz = sz * fmaf(M[8], gx, fmaf(M[0], gz, M[4] * gy));
        gx = ox; gy = oy; gz = oz;
      }
      o[l] = gz / hz; o[ovox + l] = gy / hy; o[2 * ovox + l] = gx / hx;
    }
  }
}

// ---- step scale -------------------------------------------------------------------------------------------------------------------
// acc[n] (zero on entry): the bits of the largest finite squared norm of sample n
__global__ __launch_bounds__(TPB) void disp_norm_max_kernel(const float* __restrict__ delta, unsigned* __restrict__ acc,
                                                            long long ovox) {
  const int n = blockIdx.y, tid = threadIdx.x;
  const float* dn = delta + (long long)n * 3 * ovox;
  float m = 0.f;
  // a workgroup walks every gridDim.x-th chunk (at most nchunk of them), so that a few thousand waves publish, not one per 256 voxels
  for (long long vb = (long long)blockIdx.x * CHUNK; vb < ovox; vb += (long long)gridDim.x * CHUNK) {
    const int cnt = chunk_count(ovox, vb);
    const float* d = dn + vb;
#pragma unroll
    for (int j = 0; j < PASSES; ++j) {
      const int l = tid + j * TPB;
      if (l < cnt) {
        const float z = d[l], y = d[ovox + l], x = d[2 * ovox + l];
        const float n2 = z * z + y * y + x * x;
        m = fmaxf(m, n2 <= 3.4028234e38f ? n2 : 0.f);      // (a NaN compares false)
      }
    }
  }
  m = wave_max(m);
  if ((tid & (kWave - 1)) == 0) {      // one atomic per wave, and only when it would raise the published value (absmax.h)
    const unsigned bits = __float_as_uint(m);
    if (bits > __hip_atomic_load(acc + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(acc + n, bits);
  }
}

// in place: the bits of the largest squared norm -> step / its root, 0 for a zero field
__global__ void disp_step_final_kernel(float* out, float step, int N) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < N) {
    const float m = sqrtf(__uint_as_float(reinterpret_cast<const unsigned*>(out)[n]));
    out[n] = m > 0.f ? step / m : 0.f;
  }
}

// ---- update -----------------------------------------------------------------------------------------------------------------------
// PAIRS (W >= 2): the sampler's own x-pairs, sampler_taps.h's TapB / gather8_b on each of the three planes.  W == 1 is what that
// layout excludes (lane_contiguous_ok): a row is one voxel, x0 = 0 and fx = 0, and an 8-byte load of the last voxel would straddle the
// plane's end -- so the same TapB carries the four ROW offsets, each corner is one 4-byte load and the +1 corner in x reads as 0.
template <bool PAIRS>
__device__ __forceinline__ TapB make_tap_rows(const Tap& t, int D, int H, int W) {
  if (PAIRS) return make_tapb(t, D, H, W);
  TapB q;
  const int y1 = t.y0 + 1 < H ? t.y0 + 1 : t.y0, z1 = t.z0 + 1 < D ? t.z0 + 1 : t.z0;
  q.sel = false;
  q.o00 = 4u * (unsigned)(t.z0 * H + t.y0); q.o01 = 4u * (unsigned)(t.z0 * H + y1);
  q.o10 = 4u * (unsigned)(z1 * H + t.y0); q.o11 = 4u * (unsigned)(z1 * H + y1);
  q.fx = t.fx; q.fy = t.fy; q.fz = t.fz;
  return q;
}
template <bool PAIRS>
__device__ __forceinline__ void gather8_rows(__amdgpu_buffer_rsrc_t r, const TapB& q, float v[8]) {
  if (PAIRS) {
    gather8_b(r, q, v);
    return;
  }
  v[0] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)q.o00, 0, 0));
  v[2] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)q.o01, 0, 0));
  v[4] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)q.o10, 0, 0));
  v[6] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)q.o11, 0, 0));
  v[1] = v[3] = v[5] = v[7] = 0.f;
}

template <bool PAIRS>
__global__ __launch_bounds__(TPB) void disp_update_kernel(const float* __restrict__ disp, const float* __restrict__ delta,
                                                          const float* __restrict__ scale, float* __restrict__ out, int D, int H,
                                                          int W) {
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long ovox = (long long)D * H * W;
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
  const float hx = 0.5f * (float)W, hy = 0.5f * (float)H, hz = 0.5f * (float)D;
  const float s = scale ? scale[n] : 1.f;
  const float* dl = delta + (long long)n * 3 * ovox + vb;
  float* o = out + (long long)n * 3 * ovox + vb;
  const unsigned bytes = 4u * (unsigned)ovox;      // one plane (grid_fits: < 2^31)
  const float* base = disp + (long long)n * 3 * ovox;
  const __amdgpu_buffer_rsrc_t rz = make_rsrc(base, bytes), ry = make_rsrc(base + ovox, bytes), rx = make_rsrc(base + 2 * ovox, bytes);
  constexpr int ILP = 2;       // voxels whose 12 gathers are in flight together
#pragma unroll 1
  for (int j0 = 0; j0 < PASSES; j0 += ILP) {
    Tap t[ILP];
    TapB q[ILP];
    float dz[ILP], dy[ILP], dx[ILP];
#pragma unroll
    for (int k = 0; k < ILP; ++k) {
      const int l = tid + (j0 + k) * TPB;
      const bool live = l < cnt;
      dz[k] = (live ? dl[l] : 0.f) * s; dy[k] = (live ? dl[ovox + l] : 0.f) * s; dx[k] = (live ? dl[2 * ovox + l] : 0.f) * s;
      // The products are rounded here.  This is the one asm statement of the unit, which otherwise holds no inline assembly: it is
      // EMPTY, emits no instruction, and only makes the three values opaque so that -ffp-contract=fast cannot fuse a product into
      // the add below -- unnorm_clip's device (sampler_taps.h records that __fmul_rn and the contract pragma are fused anyway).
      asm volatile("" : "+v"(dz[k]), "+v"(dy[k]), "+v"(dx[k]));
      const Vox p = vox_of(vb + (live ? l : 0), H, W);
      t[k] = make_tap(dx[k] / hx + ident(p.i, W), dy[k] / hy + ident(p.j, H), dz[k] / hz + ident(p.k, D), D, H, W);
      q[k] = make_tap_rows<PAIRS>(t[k], D, H, W);
      if (!live) park(q[k], bytes);
    }
    float v[ILP][3][8];
#pragma unroll
    for (int k = 0; k < ILP; ++k) {
      gather8_rows<PAIRS>(rz, q[k], v[k][0]);
      gather8_rows<PAIRS>(ry, q[k], v[k][1]);
      gather8_rows<PAIRS>(rx, q[k], v[k][2]);
    }
#pragma unroll
    for (int k = 0; k < ILP; ++k) {
      const int l = tid + (j0 + k) * TPB;
      if (l < cnt) {
        o[l] = dz[k] + blend8(v[k][0], t[k].fx, t[k].fy, t[k].fz);
        o[ovox + l] = dy[k] + blend8(v[k][1], t[k].fx, t[k].fy, t[k].fz);
        o[2 * ovox + l] = dx[k] + blend8(v[k][2], t[k].fx, t[k].fy, t[k].fz);
      }
    }
  }
}

static bool dense_args_ok(int N, int D, int H, int W) { return N >= 1 && N <= 65535 && grid_fits(D, H, W); }
static inline dim3 dense_launch(long long ovox, int N) { return dim3(ceil_div(ovox, (long long)CHUNK), N); }

}  // namespace

/* grid (N, D, H, W, 3) of the planar voxel displacement disp (N, 3, D, H, W): Ids + u (mat NULL, bit-identical to
   kmh_field_from_displacement), else kmh_affine_grid_fwd's grid + L (s * u).  With a matrix every axis needs two voxels. */
KMH_API int kmh_disp_grid_fwd(const float* disp, const float* mat, float* grid, int N, int D, int H, int W, void* stream) {
  if (!dense_args_ok(N, D, H, W) || !disp || !grid || grid == disp || (mat && (D < 2 || H < 2 || W < 2))) return -22;
  const dim3 g = dense_launch((long long)D * H * W, N);
  if (mat)
    disp_grid_fwd_kernel<true><<<g, TPB, 0, (hipStream_t)stream>>>(disp, mat, grid, D, H, W);
  else
    disp_grid_fwd_kernel<false><<<g, TPB, 0, (hipStream_t)stream>>>(disp, nullptr, grid, D, H, W);
  return KMH_LAUNCH_CHECK();
}

/* The transpose of kmh_disp_grid_fwd in disp: ddisp (N, 3, D, H, W) from dgrid (N, D, H, W, 3). */
KMH_API int kmh_disp_grid_bwd(const float* dgrid, const float* mat, float* ddisp, int N, int D, int H, int W, void* stream) {
  if (!dense_args_ok(N, D, H, W) || !dgrid || !ddisp || ddisp == dgrid || (mat && (D < 2 || H < 2 || W < 2))) return -22;
  disp_grid_bwd_kernel<<<dense_launch((long long)D * H * W, N), TPB, 0, (hipStream_t)stream>>>(dgrid, mat, ddisp, D, H, W);
  return KMH_LAUNCH_CHECK();
}

/* out (N) = step / the largest finite |delta[n, :, w]|_2, 0 for a field without one; out doubles as the accumulator of the maximum. */
KMH_API int kmh_disp_step_scale(const float* delta, float step, float* out, int N, int D, int H, int W, void* stream) {
  if (!dense_args_ok(N, D, H, W) || !delta || !out) return -22;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(out, 0, (size_t)N * sizeof(float), s);
  if (e != hipSuccess) return (int)e;
  const long long ovox = (long long)D * H * W;
  const int nchunk = ceil_div(ovox, (long long)CHUNK), cap = 2048 / N > 8 ? 2048 / N : 8;      // ~2048 workgroups in all
  disp_norm_max_kernel<<<dim3(nchunk < cap ? nchunk : cap, N), TPB, 0, s>>>(delta, reinterpret_cast<unsigned*>(out), ovox);
  disp_step_final_kernel<<<ceil_div(N, 256), 256, 0, s>>>(out, step, N);
  return KMH_LAUNCH_CHECK();
}

/* out = delta' + U(Ids + delta' / (S / 2)), delta' = delta * scale[n] (scale (N) on the device, or NULL: delta), U the border-clamped
   trilinear interpolant of disp; all fields (N, 3, D, H, W).  out must not be disp. */
KMH_API int kmh_disp_update(const float* disp, const float* delta, const float* scale, float* out, int N, int D, int H, int W,
                            void* stream) {
  if (!dense_args_ok(N, D, H, W) || !disp || !delta || !out || out == disp) return -22;
  const dim3 g = dense_launch((long long)D * H * W, N);
  if (W >= 2)
    disp_update_kernel<true><<<g, TPB, 0, (hipStream_t)stream>>>(disp, delta, scale, out, D, H, W);
  else
    disp_update_kernel<false><<<g, TPB, 0, (hipStream_t)stream>>>(disp, delta, scale, out, D, H, W);
  return KMH_LAUNCH_CHECK();
}
