// Diffeomorphic grids: the exponential of a stationary velocity field by scaling and squaring (ops.svf_grid), forward and
// backward.  DESIGN.md section 8g.
//
// Definition.  A displacement u (N, D, H, W, 3) -- xyz, normalised, on the voxel-centre lattice Ids of fields.hip -- is, as a
// function of space, its own trilinear interpolant U with border clamping: the sampler's coordinate, clamp mask, NaN rule and
// blend (sampler_taps.h), gathered channels-last (field_taps.h).  From u_0 = the B-spline of ctrl 2^-K (kmh_bspline_disp_fwd)
//     u_{k+1}[w] = u_k[w] + U_k(Ids[w] + u_k[w])          K times (kmh_svf_compose with first == NULL)
//     grid[w]    = Ids[w] + u_K[w]                         or, with a matrix,
//     grid[w]    = affine_grid(mat)[w] + L (s * u_K[w])    L = mat[:, :3], s = S / (S - 1) per axis   (kmh_svf_finish_fwd)
// The DISPLACEMENT is squared, not the grid: a grid that leaves the lattice hull is clamped flat by the sampler's border rule,
// a displacement is extended by its border value.  Every add is a plain fp32 add of two stored values, so a step is
// bit-identical to  u + align_img(identity_grid + u, u).
//
// Backward of a step (kmh_svf_square_bwd), the exact transpose: with g the cotangent of u_{k+1} and p = Ids + u_k,
//     du_k[w] = g[w] + J_U(p[w])^T g[w]                    (the gather half: a direct write per voxel; J carries the clamp mask, a
//                                                           NaN coordinate passes nothing)
//             + sum over the voxels w' whose cell has w as a corner of  weight(w', w) g[w']        (the scatter half).
// The scatter half is summed in 64-BIT FIXED POINT with integer atomics, so the sum does not depend on the order of arrival: runs
// are bit-identical and a batch equals its samples.  Format: per sample n, A_n = the largest finite |g| of the sample (an integer
// max on float bits, published by the kernel that wrote g), A_n < 2^ea; V <= 2^ev voxels; a contribution c = weight * g (exact
// in double: 24 x 24 bits) is added as llrint(c 2^(61 - ea - ev)).  |c| <= A_n and at most V contributions meet in one voxel, so
// |sum| <= 2^61: no overflow.  Error: each contribution is rounded to a multiple of q = 2^(ea + ev - 61) <= 2 A_n 2^(ev - 61), i.e.
// by at most A_n 2^(ev - 61) <= A_n 2^-32 (ev <= 29: grid_fits); the integer sum is exact, and the total -- gather half plus
// scatter half, added in double -- is rounded to fp32 once.  A non-finite contribution cannot be represented: it sets a flag bit of
// its channel in the voxel's word of a fourth plane instead (an atomic OR), and the finalise kernel writes NaN there; the scale ignores
// non-finite values, so a NaN poisons the corners it is scattered to and nothing else.
// Bytes per voxel and step: forward 12 in + 12 out + the gathers; backward 32 (clearing the accumulators) + 36 (u, g in, gather
// half out) + 24 eight-byte atomics + 32 + 12 + 12 (finalise).
#include "grid_coords.h"      // ident, lin, affine_coord_chain
#include "sampler_taps.h"
#include "field_taps.h"

namespace {

// ---- forward: out[w] = add[w] + U(first[w]) ---------------------------------------------------------------------------------------
// GIVEN false: first = Ids + u and add = u, the squaring step (one staging).  field_compose_kernel's chunk walk.
template <bool GIVEN>
__global__ __launch_bounds__(TPB) void svf_compose_kernel(const float* __restrict__ u, const float* __restrict__ first,
                                                          const float* __restrict__ add, float* __restrict__ out, int D, int H,
                                                          int W) {
  __shared__ __attribute__((aligned(16))) float sg[CHUNK * 3];
  __shared__ __attribute__((aligned(16))) float sa[GIVEN ? CHUNK * 3 : 4];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long ovox = (long long)D * H * W;
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
  const long long row = ((long long)n * ovox + vb) * 3;
  stage_rows((GIVEN ? first : u) + row, cnt, sg, tid);
  if (GIVEN) stage_rows(add + row, cnt, sa, tid);
  __syncthreads();
  const unsigned bytes = 12u * (unsigned)ovox;
  const __amdgpu_buffer_rsrc_t r = make_rsrc(u + (long long)n * ovox * 3, bytes);
  constexpr int ILP = 2;       // voxels whose 8 gathers are in flight together
#pragma unroll 1
  for (int j0 = 0; j0 < PASSES; j0 += ILP) {
    Tap t[ILP];
    TapG q[ILP];
#pragma unroll
    for (int k = 0; k < ILP; ++k) {
      const int l = tid + (j0 + k) * TPB;
      float px = sg[l * 3], py = sg[l * 3 + 1], pz = sg[l * 3 + 2];
      if (!GIVEN) {
        const Vox p = vox_of(vb + l, H, W);
        px = ident(p.i, W) + px; py = ident(p.j, H) + py; pz = ident(p.k, D) + pz;
      }
      t[k] = make_tap(px, py, pz, D, H, W);
      q[k] = make_tapg(t[k], D, H, W);
      if (l >= cnt) park(q[k], bytes);
    }
    float v[ILP][3][8];
#pragma unroll
    for (int k = 0; k < ILP; ++k) gather8_g(r, q[k], v[k]);
#pragma unroll
    for (int k = 0; k < ILP; ++k) {
      const int l = tid + (j0 + k) * TPB;       // each lane owns its rows of sg
#pragma unroll
      for (int c = 0; c < 3; ++c) sg[l * 3 + c] = (GIVEN ? sa[l * 3 + c] : sg[l * 3 + c]) + blend8(v[k][c], t[k].fx, t[k].fy, t[k].fz);
    }
  }
  __syncthreads();
  unstage_rows(out + row, cnt, sg, tid);
}

// ---- the per-sample scale of the fixed-point sums ---------------------------------------------------------------------------------
// the largest FINITE magnitude (a NaN or an Inf is flagged where it lands, it does not set the scale)
__device__ __forceinline__ float finite_abs(float x) {
  const float a = fabsf(x);
  return a <= 3.4028234e38f ? a : 0.f;
}
// non-negative floats order like their bit patterns: an integer max is exact and order independent (absmax.h)
__device__ __forceinline__ void publish_max(float m, unsigned* acc) {
  m = wave_max(m);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    const unsigned bits = __float_as_uint(m);
    if (bits > __hip_atomic_load(acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(acc, bits);
  }
}
// the exponent e of the scale 2^e: A < 2^ea, at most 2^ev contributions per voxel, |sum| 2^e <= 2^61
__device__ __forceinline__ int scale_exp(unsigned amax_bits, int ev) {
  const float A = __uint_as_float(amax_bits);
  if (!(A > 0.f)) return 0;
  int ea;
  frexpf(A, &ea);
  return 61 - ea - ev;
}

// ---- backward of a squaring step: the gather half and the scatter -----------------------------------------------------------------
// acc (N, 4, V) 64-bit words, zero on entry: planes 0..2 the fixed-point sums of the three channels, plane 3 the non-finite flags.
// Planar, so that the 64 lanes of an atomic instruction -- neighbouring voxels, whose corners are neighbours for a map near the
// identity -- add to 512 contiguous bytes (voxel-major words, 8 bytes in every 32, ran the 256^3 step at 0.3 TB/s of added bytes).
__global__ __launch_bounds__(TPB) void svf_square_bwd_kernel(const float* __restrict__ u, const float* g, float* half,
                                                             unsigned long long* __restrict__ acc,
                                                             const unsigned* __restrict__ amax, int ev, int D, int H, int W) {
  __shared__ __attribute__((aligned(16))) float su[CHUNK * 3];
  __shared__ __attribute__((aligned(16))) float sg[CHUNK * 3];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long ovox = (long long)D * H * W;
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
  const long long row = ((long long)n * ovox + vb) * 3;
  stage_rows(u + row, cnt, su, tid);
  stage_rows(g + row, cnt, sg, tid);
  __syncthreads();
  const unsigned bytes = 12u * (unsigned)ovox;
  const __amdgpu_buffer_rsrc_t r = make_rsrc(u + (long long)n * ovox * 3, bytes);
  const double S = ldexp(1.0, scale_exp(amax[n], ev));
  unsigned long long* a = acc + (long long)n * ovox * 4;
#pragma unroll 1
  for (int j = 0; j < PASSES; ++j) {
    const int l = tid + j * TPB;
    const Vox p = vox_of(vb + l, H, W);
    const float px = ident(p.i, W) + su[l * 3], py = ident(p.j, H) + su[l * 3 + 1], pz = ident(p.k, D) + su[l * 3 + 2];
    const Tap t = make_tap(px, py, pz, D, H, W);
    TapG q = make_tapg(t, D, H, W);
    if (l >= cnt) park(q, bytes);
    float v[3][8];
    gather8_g(r, q, v);
    const float gc[3] = {sg[l * 3], sg[l * 3 + 1], sg[l * 3 + 2]};
    const bool nan_p = any_nan(px, py, pz);
    // the gather half: g + J^T g, J[c][a] = d U_c / d p_a
    float jx = 0.f, jy = 0.f, jz = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float dx, dy, dz;
      blend_grads(v[c], t.fx, t.fy, t.fz, dx, dy, dz);
      jx = fmaf(dx, gc[c], jx); jy = fmaf(dy, gc[c], jy); jz = fmaf(dz, gc[c], jz);
    }
    sg[l * 3] = gc[0] + (nan_p ? 0.f : jx * t.mx); sg[l * 3 + 1] = gc[1] + (nan_p ? 0.f : jy * t.my);
    sg[l * 3 + 2] = gc[2] + (nan_p ? 0.f : jz * t.mz);
    // the scatter half: weight * g onto the corners that lie inside the volume (a corner past the far border has weight 0)
    if (l < cnt && !nan_p) {
      const float wx[2] = {1.f - t.fx, t.fx}, wy[2] = {1.f - t.fy, t.fy}, wz[2] = {1.f - t.fz, t.fz};
      const bool fin[3] = {fabsf(gc[0]) <= 3.4028234e38f, fabsf(gc[1]) <= 3.4028234e38f, fabsf(gc[2]) <= 3.4028234e38f};
      const unsigned long long flags = (fin[0] ? 0ull : 1ull) | (fin[1] ? 0ull : 2ull) | (fin[2] ? 0ull : 4ull);
#pragma unroll
      for (int cz = 0; cz < 2; ++cz)
#pragma unroll
        for (int cy = 0; cy < 2; ++cy)
#pragma unroll
          for (int cx = 0; cx < 2; ++cx) {
            const int x = t.x0 + cx, y = t.y0 + cy, z = t.z0 + cz;
            if (x < W && y < H && z < D) {      // (x0, y0, z0 are inside: make_tap)
              const float w = wx[cx] * wy[cy] * wz[cz];      // the weight as blend8 forms it
              unsigned long long* d = a + ((long long)(z * H + y) * W + x);
#pragma unroll
              for (int c = 0; c < 3; ++c)
                if (fin[c]) {
                  const long long qv = __double2ll_rn((double)w * (double)gc[c] * S);
                  if (qv != 0) atomicAdd(d + c * ovox, (unsigned long long)qv);
                }
              if (flags) atomicOr(d + 3 * ovox, flags);
            }
          }
    }
  }
  __syncthreads();
  unstage_rows(half + row, cnt, sg, tid);
}

// out = half + acc / scale (may be written over half), and the largest finite |out| of the sample for the next step
__global__ __launch_bounds__(TPB) void svf_square_bwd_final_kernel(const float* half, const unsigned long long* __restrict__ acc,
                                                                   float* out, const unsigned* __restrict__ amax,
                                                                   unsigned* __restrict__ amax_out, int ev, long long ovox) {
  __shared__ __attribute__((aligned(16))) float sg[CHUNK * 3];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
  const long long row = ((long long)n * ovox + vb) * 3;
  stage_rows(half + row, cnt, sg, tid);
  __syncthreads();
  const double inv = ldexp(1.0, -scale_exp(amax[n], ev));
  const unsigned long long* a = acc + (long long)n * ovox * 4 + vb;
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < PASSES; ++j) {
    const int l = tid + j * TPB;
    if (l < cnt) {
      const long long s[3] = {(long long)a[l], (long long)a[ovox + l], (long long)a[2 * ovox + l]};
      const unsigned long long flags = a[3 * ovox + l];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float o = (float)((double)sg[l * 3 + c] + (double)s[c] * inv);
        if ((flags >> c) & 1ull) o = __uint_as_float(0x7fc00000u);
        sg[l * 3 + c] = o;
        m = fmaxf(m, finite_abs(o));
      }
    }
  }
  if (amax_out) publish_max(m, amax_out + n);
  __syncthreads();
  unstage_rows(out + row, cnt, sg, tid);
}

// ---- finish: the grid of a displacement, and its transpose ------------------------------------------------------------------------
// mat == NULL: Ids + u.  Else the matrix applied to the deformed point: kmh_affine_grid_fwd's base (bspline.hip's statement of it)
// plus L (s * u) -- the small displacement is multiplied before it meets an O(1) coordinate, and a zero u leaves the base's bits.
__global__ __launch_bounds__(TPB) void svf_finish_fwd_kernel(const float* u, const float* __restrict__ mat, float* out, int D, int H,
                                                             int W) {
  __shared__ __attribute__((aligned(16))) float sg[CHUNK * 3];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long ovox = (long long)D * H * W;
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
  const long long row = ((long long)n * ovox + vb) * 3;
  stage_rows(u + row, cnt, sg, tid);
  __syncthreads();
  float M[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) M[i] = mat ? mat[n * 12 + i] : 0.f;
  const float stz = lin_step(D), sty = lin_step(H), stx = lin_step(W);
  const float sz = (float)D / (float)(D - 1), sy = (float)H / (float)(H - 1), sx = (float)W / (float)(W - 1);      // (mat: S >= 2)
#pragma unroll
  for (int j = 0; j < PASSES; ++j) {
    const int l = tid + j * TPB;
    const Vox p = vox_of(vb + l, H, W);
    const float ux = sg[l * 3], uy = sg[l * 3 + 1], uz = sg[l * 3 + 2];
    if (mat) {
      float bx, by, bz;
      affine_coord_chain(M, lin(p.k, D, stz), lin(p.j, H, sty), lin(p.i, W, stx), bx, by, bz);
      const float dz = sz * uz, dy = sy * uy, dx = sx * ux;
      sg[l * 3] = bx + fmaf(M[10], dx, fmaf(M[8], dz, M[9] * dy));
      sg[l * 3 + 1] = by + fmaf(M[6], dx, fmaf(M[4], dz, M[5] * dy));
      sg[l * 3 + 2] = bz + fmaf(M[2], dx, fmaf(M[0], dz, M[1] * dy));
    } else {
      sg[l * 3] = ident(p.i, W) + ux; sg[l * 3 + 1] = ident(p.j, H) + uy; sg[l * 3 + 2] = ident(p.k, D) + uz;
    }
  }
  __syncthreads();
  unstage_rows(out + row, cnt, sg, tid);
}

// du = s * (L^T dgrid) (mat == NULL: dgrid itself), and the largest finite |du| of the sample for the first squaring step
__global__ __launch_bounds__(TPB) void svf_finish_bwd_kernel(const float* __restrict__ dgrid, const float* __restrict__ mat,
                                                             float* __restrict__ du, unsigned* __restrict__ amax_out, int D, int H,
                                                             int W) {
  __shared__ __attribute__((aligned(16))) float sg[CHUNK * 3];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long ovox = (long long)D * H * W;
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
  const long long row = ((long long)n * ovox + vb) * 3;
  stage_rows(dgrid + row, cnt, sg, tid);
  __syncthreads();
  float M[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) M[i] = mat ? mat[n * 12 + i] : 0.f;
  const float sz = (float)D / (float)(D - 1), sy = (float)H / (float)(H - 1), sx = (float)W / (float)(W - 1);
  float m = 0.f;
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
        sg[l * 3] = gx; sg[l * 3 + 1] = gy; sg[l * 3 + 2] = gz;
      }
      m = fmaxf(m, fmaxf(finite_abs(gx), fmaxf(finite_abs(gy), finite_abs(gz))));
    }
  }
  if (amax_out) publish_max(m, amax_out + n);
  __syncthreads();
  unstage_rows(du + row, cnt, sg, tid);
}

static bool svf_args_ok(int N, int D, int H, int W) { return N >= 1 && N <= 65535 && grid_fits(D, H, W); }
static inline dim3 svf_launch(long long ovox, int N) { return dim3(ceil_div(ovox, (long long)CHUNK), N); }
// the smallest ev with V <= 2^ev
static int voxel_exp(long long ovox) {
  int ev = 0;
  while ((1ll << ev) < ovox) ++ev;
  return ev;
}

}  // namespace

/* out[w] = add[w] + U(first[w]), U the border-clamped trilinear interpolant of the displacement u; all (N, D, H, W, 3).
   first == NULL: first = Ids + u and add = u (add is not read): one squaring step.  out must not overlap u. */
KMH_API int kmh_svf_compose(const float* u, const float* first, const float* add, float* out, int N, int D, int H, int W,
                            void* stream) {
  if (!svf_args_ok(N, D, H, W) || !u || !out || out == u || (first && !add)) return -22;
  const long long ovox = (long long)D * H * W;
  if (first)
    svf_compose_kernel<true><<<svf_launch(ovox, N), TPB, 0, (hipStream_t)stream>>>(u, first, add, out, D, H, W);
  else
    svf_compose_kernel<false><<<svf_launch(ovox, N), TPB, 0, (hipStream_t)stream>>>(u, nullptr, nullptr, out, D, H, W);
  return KMH_LAUNCH_CHECK();
}

/* Workspace of kmh_svf_square_bwd: the fixed-point accumulators, four 64-bit words per voxel. */
KMH_API size_t kmh_svf_square_bwd_ws_bytes(int N, int D, int H, int W) {
  return svf_args_ok(N, D, H, W) ? (size_t)N * D * H * W * 4 * sizeof(unsigned long long) : 0;
}

/* The transpose of one squaring step: du (the cotangent of u) from g (the cotangent of u + U(Ids + u)); du may be g.  amax_in (N)
   holds the bits of the largest finite |g| per sample (kmh_svf_finish_bwd or the previous call wrote it); amax_out (N, zeroed by
   the caller, or NULL) receives that of du. */
KMH_API int kmh_svf_square_bwd(const float* u, const float* g, float* du, const unsigned* amax_in, unsigned* amax_out, int N, int D,
                               int H, int W, void* ws, void* stream) {
  if (!svf_args_ok(N, D, H, W) || !u || !g || !du || !amax_in || !ws || du == u) return -22;
  const long long ovox = (long long)D * H * W;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(ws, 0, (size_t)N * ovox * 4 * sizeof(unsigned long long), s);
  if (e != hipSuccess) return (int)e;
  const int ev = voxel_exp(ovox);
  svf_square_bwd_kernel<<<svf_launch(ovox, N), TPB, 0, s>>>(u, g, du, (unsigned long long*)ws, amax_in, ev, D, H, W);
  svf_square_bwd_final_kernel<<<svf_launch(ovox, N), TPB, 0, s>>>(du, (const unsigned long long*)ws, du, amax_in, amax_out, ev, ovox);
  return KMH_LAUNCH_CHECK();
}

/* grid = Ids + u (mat NULL) or affine_grid(mat) + L (s * u); out may be u.  With a matrix every axis needs two voxels. */
KMH_API int kmh_svf_finish_fwd(const float* u, const float* mat, float* out, int N, int D, int H, int W, void* stream) {
  if (!svf_args_ok(N, D, H, W) || !u || !out || (mat && (D < 2 || H < 2 || W < 2))) return -22;
  svf_finish_fwd_kernel<<<svf_launch((long long)D * H * W, N), TPB, 0, (hipStream_t)stream>>>(u, mat, out, D, H, W);
  return KMH_LAUNCH_CHECK();
}

/* The transpose of kmh_svf_finish_fwd in u: du = s * (L^T dgrid), or dgrid; amax_out (N, zeroed by the caller, or NULL): the bits of
   the largest finite |du| per sample. */
KMH_API int kmh_svf_finish_bwd(const float* dgrid, const float* mat, float* du, unsigned* amax_out, int N, int D, int H, int W,
                               void* stream) {
  if (!svf_args_ok(N, D, H, W) || !dgrid || !du || du == dgrid || (mat && (D < 2 || H < 2 || W < 2))) return -22;
  svf_finish_bwd_kernel<<<svf_launch((long long)D * H * W, N), TPB, 0, (hipStream_t)stream>>>(dgrid, mat, du, amax_out, D, H, W);
  return KMH_LAUNCH_CHECK();
}
