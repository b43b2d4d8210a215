// Sampling grids as transforms (keymorph_amd/fields.py): compose two grids, invert one, and the voxel displacement
// field that the Jacobian metrics of loss_ops read.
//
// A grid (n, D, H, W, 3) -- xyz, normalised, align_corners=False -- is, as a function of space, its own trilinear
// interpolant with border clamping: exactly what the sampler does to any volume.  So the coordinate, the clamp, the
// NaN rule and the blend are the sampler's (sampler_taps.h), and so is the chunk walk: a workgroup owns 1024 consecutive
// voxels, one per lane per pass, and the AoS rows go through LDS so that global accesses are 16-byte coalesced.
// What differs is the OPERAND: a grid is gathered channels-last, the two x-corners of a row are 24 contiguous bytes
// (two 12-byte buffer loads), and no (n, 3, D, H, W) copy is made.
//
// compose: HBM-bound, 12 B in + 12 B out per voxel plus the gathers (8 taps of 12 B from L2 / Infinity Cache).
// invert: per-voxel Newton in registers, one gather round per step; bound by the latency of those rounds.
// displacement: streaming, 24 B per voxel.
#include "grid_coords.h"      // ident: the voxel-centre lattice, shared with bspline.hip
#include "sampler_taps.h"
#include "field_taps.h"      // Vox, TapG, gather8_g, grid_fits: shared with svf.hip

namespace {

// ---- identity ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void field_identity_kernel(float* __restrict__ out, int H, int W, long long ovox) {
  __shared__ __attribute__((aligned(16))) float sg[CHUNK * 3];
  const int n = blockIdx.y, tid = threadIdx.x;
  const int D = (int)(ovox / ((long long)H * W));
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
#pragma unroll
  for (int u = 0; u < PASSES; ++u) {
    const int l = tid + u * TPB;
    const Vox p = vox_of(vb + l, H, W);       // (past the volume: values nobody stores)
    sg[l * 3] = ident(p.i, W); sg[l * 3 + 1] = ident(p.j, H); sg[l * 3 + 2] = ident(p.k, D);
  }
  __syncthreads();
  unstage_rows(out + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
}

// ---- compose -------------------------------------------------------------------------------------------------
// out[w] = then interpolated at first[w]: per channel the blend8 of the sampler on the same 8 corner values, so the
// result is bit-identical to sampling the (n, 3, D, H, W) copy of `then` with `first`.
__global__ __launch_bounds__(TPB) void field_compose_kernel(const float* __restrict__ first, const float* __restrict__ then,
                                                            float* __restrict__ out, int D, int H, int W, long long ovox) {
  __shared__ __attribute__((aligned(16))) float sg[CHUNK * 3];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
  stage_rows(first + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
  __syncthreads();
  const unsigned bytes = 12u * (unsigned)(D * H * W);
  const __amdgpu_buffer_rsrc_t r = make_rsrc(then + (long long)n * D * H * W * 3, bytes);
  constexpr int ILP = 2;       // voxels whose 8 gathers are in flight together
#pragma unroll 1
  for (int j0 = 0; j0 < PASSES; j0 += ILP) {
    Tap t[ILP];
    TapG q[ILP];
#pragma unroll
    for (int u = 0; u < ILP; ++u) {
      const int l = tid + (j0 + u) * TPB;
      t[u] = make_tap(sg[l * 3], sg[l * 3 + 1], sg[l * 3 + 2], D, H, W);
      q[u] = make_tapg(t[u], D, H, W);
      if (l >= cnt) park(q[u], bytes);
    }
    float v[ILP][3][8];
#pragma unroll
    for (int u = 0; u < ILP; ++u) gather8_g(r, q[u], v[u]);
#pragma unroll
    for (int u = 0; u < ILP; ++u) {
      const int l = tid + (j0 + u) * TPB;       // each lane owns its rows of sg: coordinates in, composed grid out
#pragma unroll
      for (int c = 0; c < 3; ++c) sg[l * 3 + c] = blend8(v[u][c], t[u].fx, t[u].fy, t[u].fz);
    }
  }
  __syncthreads();
  unstage_rows(out + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
}

// ---- invert --------------------------------------------------------------------------------------------------
// Per voxel w: solve grid(c) = Ids[w] for c by Newton steps, everything in registers.  One step = the 8 taps of the cell
// of c (24 floats), residual r = Ids[w] - grid(c), the 3x3 Jacobian d grid / d c of the same taps (clamp mask of
// unnorm_clip included), c += J^-1 r limited to one voxel per axis and clamped to [-1, 1].  Where J is near-singular
// relative to the affine start (a fold, or the flat band between the border and the first voxel centre, where the
// clamp mask zeroes a column) the step goes through the start's linear part L instead.
// The trip count differs per lane: the wave loops until none of its lanes is active.
struct InvStats { int unconv; int iters; float maxres; int pad; };

__device__ __forceinline__ float clamp11(float c) { return fminf(fmaxf(c, -1.f), 1.f); }      // NaN -> -1

__global__ __launch_bounds__(TPB) void field_invert_kernel(const float* __restrict__ grid, const float* __restrict__ start,
                                                           float* __restrict__ out, unsigned char* __restrict__ conv,
                                                           InvStats* __restrict__ part, int D, int H, int W, float tol,
                                                           int max_iters) {
  __shared__ __attribute__((aligned(16))) float sg[CHUNK * 3];
  __shared__ float sm[12];
  __shared__ int red_i[2][TPB / kWave];
  __shared__ float red_f[TPB / kWave];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long ovox = (long long)D * H * W;
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
  if (tid < 12) sm[tid] = start[n * 12 + tid];
  __syncthreads();
  float A[3][4];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) A[i][j] = sm[i * 4 + j];
  const float detL = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                     A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
  const unsigned bytes = 12u * (unsigned)ovox;
  const __amdgpu_buffer_rsrc_t r = make_rsrc(grid + (long long)n * ovox * 3, bytes);
  const float lim[3] = {2.f / (float)W, 2.f / (float)H, 2.f / (float)D};      // one voxel, normalised
  int n_unconv = 0, n_iters = 0;
  float maxres = 0.f;
#pragma unroll 1
  for (int u = 0; u < PASSES; ++u) {
    const int l = tid + u * TPB;
    const Vox p = vox_of(vb + l, H, W);
    const float T[3] = {ident(p.i, W), ident(p.j, H), ident(p.k, D)};
    float c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = clamp11(fmaf(A[a][0], T[0], fmaf(A[a][1], T[1], fmaf(A[a][2], T[2], A[a][3]))));
    bool active = l < cnt, ok = false;
    float res = 0.f;
    int it = 0;
    while (__builtin_amdgcn_ballot_w64(active) != 0) {
      if (active) {
        // c is finite and inside [-1, 1], so every tap address is inside the grid
        const Tap t = make_tap(c[0], c[1], c[2], D, H, W);
        const TapG q = make_tapg(t, D, H, W);
        float v[3][8];
        gather8_g(r, q, v);
        float rr[3], J[3][3];
        const float m[3] = {t.mx, t.my, t.mz};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          rr[k] = T[k] - blend8(v[k], t.fx, t.fy, t.fz);
          blend_grads(v[k], t.fx, t.fy, t.fz, J[k][0], J[k][1], J[k][2]);
#pragma unroll
          for (int a = 0; a < 3; ++a) J[k][a] *= m[a];
        }
        res = fmaxf(fabsf(rr[0]), fmaxf(fabsf(rr[1]), fabsf(rr[2])));      // (fmaxf drops a NaN: tested on the components)
        if (!(fabsf(rr[0]) <= 3.0e38f && fabsf(rr[1]) <= 3.0e38f && fabsf(rr[2]) <= 3.0e38f)) {
          // NaN or Inf met: flagged, c stays the last finite iterate
          active = false;
        } else if (res <= tol) {
          ok = true; active = false;
        } else if (it >= max_iters) {
          active = false;
        } else {
          // cofactors of J
          const float c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2],
                      c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
          const float det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
          float d[3];
          if (det * detL > 0.05f) {                   // (false for NaN too)
            const float id = 1.f / det;
            const float c10 = J[0][2] * J[2][1] - J[0][1] * J[2][2], c11 = J[0][0] * J[2][2] - J[0][2] * J[2][0],
                        c12 = J[0][1] * J[2][0] - J[0][0] * J[2][1];
            const float c20 = J[0][1] * J[1][2] - J[0][2] * J[1][1], c21 = J[0][2] * J[1][0] - J[0][0] * J[1][2],
                        c22 = J[0][0] * J[1][1] - J[0][1] * J[1][0];
            d[0] = (c00 * rr[0] + c10 * rr[1] + c20 * rr[2]) * id;
            d[1] = (c01 * rr[0] + c11 * rr[1] + c21 * rr[2]) * id;
            d[2] = (c02 * rr[0] + c12 * rr[1] + c22 * rr[2]) * id;
          } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) d[a] = A[a][0] * rr[0] + A[a][1] * rr[1] + A[a][2] * rr[2];
          }
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            const float s = fminf(fmaxf(d[a], -lim[a]), lim[a]);      // NaN -> -lim
            c[a] = clamp11(c[a] + s);
          }
          ++it;
        }
      }
    }
    sg[l * 3] = c[0]; sg[l * 3 + 1] = c[1]; sg[l * 3 + 2] = c[2];
    if (l < cnt) {
      conv[(long long)n * ovox + vb + l] = ok ? 1 : 0;
      n_unconv += ok ? 0 : 1;
      n_iters += it;
      if (ok) maxres = fmaxf(maxres, res);
    }
  }
  __syncthreads();
  unstage_rows(out + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
  // per-block partials, reduced in a fixed order (integers and a max: the same bits every run)
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    n_unconv += __shfl_xor(n_unconv, o, kWave);
    n_iters += __shfl_xor(n_iters, o, kWave);
  }
  maxres = wave_max(maxres);
  if ((tid & (kWave - 1)) == 0) { red_i[0][tid / kWave] = n_unconv; red_i[1][tid / kWave] = n_iters; red_f[tid / kWave] = maxres; }
  __syncthreads();
  if (tid == 0) {
    InvStats s = {0, 0, 0.f, 0};
#pragma unroll
    for (int w = 0; w < TPB / kWave; ++w) {
      s.unconv += red_i[0][w]; s.iters += red_i[1][w]; s.maxres = fmaxf(s.maxres, red_f[w]);
    }
    part[(long long)n * gridDim.x + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(TPB) void field_invert_final_kernel(const InvStats* __restrict__ part, int nb,
                                                                 long long* __restrict__ unconverged,
                                                                 float* __restrict__ max_residual,
                                                                 long long* __restrict__ iterations) {
  __shared__ long long red_u[TPB / kWave], red_t[TPB / kWave];
  __shared__ float red_f[TPB / kWave];
  const int n = blockIdx.x, tid = threadIdx.x;
  long long un = 0, its = 0;
  float mr = 0.f;
  for (int b = tid; b < nb; b += TPB) {
    const InvStats s = part[(long long)n * nb + b];
    un += s.unconv; its += s.iters; mr = fmaxf(mr, s.maxres);
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) { un += __shfl_xor(un, o, kWave); its += __shfl_xor(its, o, kWave); }
  mr = wave_max(mr);
  if ((tid & (kWave - 1)) == 0) { red_u[tid / kWave] = un; red_t[tid / kWave] = its; red_f[tid / kWave] = mr; }
  __syncthreads();
  if (tid == 0) {
    un = its = 0; mr = 0.f;
#pragma unroll
    for (int w = 0; w < TPB / kWave; ++w) { un += red_u[w]; its += red_t[w]; mr = fmaxf(mr, red_f[w]); }
    unconverged[n] = un;
    max_residual[n] = mr;
    if (iterations) iterations[n] = its;
  }
}

// ---- displacement <-> grid -----------------------------------------------------------------------------------
// disp (n, 3, D, H, W), channels (z, y, x), voxels: (g - Ids) * S / 2 -- the subtraction first, so a grid near the
// identity loses nothing to the scaling.  The permute between the AoS grid and the planar field is the LDS staging.
__global__ __launch_bounds__(TPB) void field_to_disp_kernel(const float* __restrict__ grid, float* __restrict__ disp, int D,
                                                            int H, int W) {
  __shared__ __attribute__((aligned(16))) float sg[CHUNK * 3];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long ovox = (long long)D * H * W;
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
  stage_rows(grid + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
  __syncthreads();
  const float hx = 0.5f * (float)W, hy = 0.5f * (float)H, hz = 0.5f * (float)D;
  float* o = disp + (long long)n * 3 * ovox + vb;
#pragma unroll
  for (int u = 0; u < PASSES; ++u) {
    const int l = tid + u * TPB;
    if (l < cnt) {
      const Vox p = vox_of(vb + l, H, W);
      o[l] = (sg[l * 3 + 2] - ident(p.k, D)) * hz;
      o[ovox + l] = (sg[l * 3 + 1] - ident(p.j, H)) * hy;
      o[2 * ovox + l] = (sg[l * 3] - ident(p.i, W)) * hx;
    }
  }
}

__global__ __launch_bounds__(TPB) void field_from_disp_kernel(const float* __restrict__ disp, float* __restrict__ grid, int D,
                                                              int H, int W) {
  __shared__ __attribute__((aligned(16))) float sg[CHUNK * 3];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long ovox = (long long)D * H * W;
  const long long vb = (long long)blockIdx.x * CHUNK;
  const int cnt = chunk_count(ovox, vb);
  const float hx = 0.5f * (float)W, hy = 0.5f * (float)H, hz = 0.5f * (float)D;
  const float* d = disp + (long long)n * 3 * ovox + vb;
#pragma unroll
  for (int u = 0; u < PASSES; ++u) {
    const int l = tid + u * TPB;
    if (l < cnt) {
      const Vox p = vox_of(vb + l, H, W);
      sg[l * 3] = d[2 * ovox + l] / hx + ident(p.i, W);
      sg[l * 3 + 1] = d[ovox + l] / hy + ident(p.j, H);
      sg[l * 3 + 2] = d[l] / hz + ident(p.k, D);
    }
  }
  __syncthreads();
  unstage_rows(grid + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
}

static inline dim3 field_launch(long long ovox, int N) { return dim3(ceil_div(ovox, (long long)CHUNK), N); }
static bool lattice_fits(int N, int D, int H, int W) {
  return N >= 1 && N <= 65535 && D >= 1 && H >= 1 && W >= 1 && (long long)D * H * W < (1ll << 31);
}

}  // namespace

KMH_API int kmh_field_identity(float* out, int N, int D, int H, int W, void* stream) {
  if (!lattice_fits(N, D, H, W)) return -22;
  const long long ovox = (long long)D * H * W;
  field_identity_kernel<<<field_launch(ovox, N), TPB, 0, (hipStream_t)stream>>>(out, H, W, ovox);
  return KMH_LAUNCH_CHECK();
}

KMH_API int kmh_field_compose(const float* first, const float* then, float* out, int N, int Do, int Ho, int Wo, int D, int H,
                              int W, void* stream) {
  if (!lattice_fits(N, Do, Ho, Wo) || !grid_fits(D, H, W)) return -22;
  const long long ovox = (long long)Do * Ho * Wo;
  field_compose_kernel<<<field_launch(ovox, N), TPB, 0, (hipStream_t)stream>>>(first, then, out, D, H, W, ovox);
  return KMH_LAUNCH_CHECK();
}

KMH_API size_t kmh_field_invert_ws_bytes(int N, int D, int H, int W) {
  return (size_t)N * (size_t)ceil_div((long long)D * H * W, (long long)CHUNK) * sizeof(InvStats);
}

KMH_API int kmh_field_invert(const float* grid, const float* start, float* out, unsigned char* converged,
                             long long* unconverged, float* max_residual, long long* iterations, int N, int D, int H, int W,
                             float tol, int max_iters, void* ws, void* stream) {
  if (!lattice_fits(N, D, H, W) || !grid_fits(D, H, W) || D < 2 || H < 2 || W < 2 || max_iters < 0 || !(tol >= 0.f)) return -22;
  const long long ovox = (long long)D * H * W;
  const dim3 g = field_launch(ovox, N);
  hipStream_t s = (hipStream_t)stream;
  field_invert_kernel<<<g, TPB, 0, s>>>(grid, start, out, converged, (InvStats*)ws, D, H, W, tol, max_iters);
  field_invert_final_kernel<<<N, TPB, 0, s>>>((const InvStats*)ws, (int)g.x, unconverged, max_residual, iterations);
  return KMH_LAUNCH_CHECK();
}

KMH_API int kmh_field_to_displacement(const float* grid, float* disp, int N, int D, int H, int W, void* stream) {
  if (!lattice_fits(N, D, H, W)) return -22;
  field_to_disp_kernel<<<field_launch((long long)D * H * W, N), TPB, 0, (hipStream_t)stream>>>(grid, disp, D, H, W);
  return KMH_LAUNCH_CHECK();
}

KMH_API int kmh_field_from_displacement(const float* disp, float* grid, int N, int D, int H, int W, void* stream) {
  if (!lattice_fits(N, D, H, W)) return -22;
  field_from_disp_kernel<<<field_launch((long long)D * H * W, N), TPB, 0, (hipStream_t)stream>>>(disp, grid, D, H, W);
  return KMH_LAUNCH_CHECK();
}
