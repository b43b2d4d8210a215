// LC2 / ImageLC2 (keymorph/loss_ops.py:250-391): linear correlation of linear combinations, the multimodal (US-MR) similarity.
//
// A batch of N cubic volumes (S^3, channel 1 dropped) is tiled into nP^3 non-overlapping P^3 patches per volume (nP = S / P,
// the remainder dropped: ImageLC2's unfold; LC2 is the case P = S, one patch per volume).  Patch p, radius r, w = 2r + 1,
// pad = (P - w) / 2 >= 1 (P - w even): the centred w^3 crop of the patch gives n = w^3 columns A_i = [mr_i, g_i, 1] and
// b_i = us_i, where g = |(mr(x-1) - mr(x+1), mr(y-1) - mr(y+1), mr(z-1) - mr(z+1))| (the reference's conv3d with f, padding 1;
// its zero padding is never read because pad >= 1).  With C = A A^T / n + alpha I, Atb = A b / n, c = C^-1 Atb:
//   var = mean(b^2) - mean(b)^2,  dist = mean(b^2) + c^T C c - 2 c^T Atb,  sym = clamp((var - dist) / max(var, beta), 0, 1).
//
// lc2_fwd_kernel   one workgroup per (patch, radius): streams the crop, forms g from mr and its halo in registers, accumulates the
//                  nine moments in fp64 (wave reductions + LDS, fixed order), solves the 3x3 SPD system in closed form (fp64) and
//                  writes sym and the backward coefficients to the workspace.
// lc2_out_kernel   one workgroup: per-patch mean over the radii, and the mean over the patches (reduction "mean"), fixed order.
// lc2_bwd_kernel   one lane per voxel of the whole (N, S, S, S) volume, writes d/d(us) and d/d(mr) everywhere (zeros outside the
//                  crops and their 1-voxel halos: no memset, no read-modify-write).  Gather form: a voxel sums its direct terms and,
//                  for mr, the +-d_k / g terms of its up to six crop neighbours, over every radius (LC2's crops are nested).
//
// Derivatives (q = c^T Atb, so var - dist = q - mean(b)^2; e_i = c^T A_i the fitted value; den = max(var, beta)):
//   d sym / d b_i  = s (e_i - mb) - t (b_i - mb)
//   d sym / d mr_i = s c0 (b_i - e_i)        (through A's first row)
//   d sym / d g_i  = s c1 (b_i - e_i)        (then through g = |d|: d g_i / d d_k = d_k / g_i, and 0 where g_i = 0, as torch.norm)
// with s = 2 / (n den) and t = 2 (var - dist) / (n den^2) [var >= beta], both 0 unless 0 <= raw sym <= 1: torch's clamp_min and
// clamp pass the gradient where the input is >= the bound (resp. within the bounds, bounds included).
#include "common.h"

namespace {
constexpr int TPB = 256;
constexpr int kRows = TPB / kWave;       // backward block: 64 voxels of a row x 4 rows
constexpr int kMaxRadii = 8;
constexpr int kMaxRadius = 511;          // w = 1023: w^3 < 2^31 (the forward kernel's crop index is an int)
constexpr int kCoef = 8;                 // doubles per (patch, radius): s, t, c0, c1, c2, mean(b), sym, unused

struct Lc2Args {
  const float* us;
  const float* mr;
  int N, S, P, nP, B, R;
  int hlo;                               // first local coordinate of the largest crop's halo (the smallest pad - 1)
  int radius[kMaxRadii];
  double alpha, beta;
};

// |(d_x, d_y, d_z)| of mr at flat index v (all six neighbours exist), fp64; d[k] = the difference along x, y, z
__device__ __forceinline__ double grad_norm(const float* __restrict__ mr, long long v, long long sy, long long sz, double d[3]) {
  d[0] = (double)mr[v - 1] - (double)mr[v + 1];
  d[1] = (double)mr[v - sy] - (double)mr[v + sy];
  d[2] = (double)mr[v - sz] - (double)mr[v + sz];
  return sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}

__global__ __launch_bounds__(TPB) void lc2_fwd_kernel(Lc2Args a, double* __restrict__ ws) {
  __shared__ double part[TPB / kWave][9];
  const int p = blockIdx.x, ri = blockIdx.y;
  const int w = 2 * a.radius[ri] + 1, pad = (a.P - w) / 2;
  int q = p;
  const int px = q % a.nP;
  q /= a.nP;
  const int py = q % a.nP;
  q /= a.nP;
  const int pz = q % a.nP, n = q / a.nP;
  const long long sy = a.S, sz = (long long)a.S * a.S;
  const long long base = (long long)n * sz * a.S + (long long)(pz * a.P + pad) * sz + (long long)(py * a.P + pad) * sy +
                         (px * a.P + pad);
  const int count = w * w * w;
  // moments: 0 m, 1 g, 2 m^2, 3 m g, 4 g^2, 5 b, 6 b^2, 7 m b, 8 g b
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < count; i += TPB) {
    const int cx = i % w, t = i / w, cy = t % w, cz = t / w;
    const long long v = base + cz * sz + cy * sy + cx;
    double d[3];
    const double m = a.mr[v], b = a.us[v], g = grad_norm(a.mr, v, sy, sz, d);
    acc[0] += m;
    acc[1] += g;
    acc[2] += m * m;
    acc[3] += m * g;
    acc[4] += g * g;
    acc[5] += b;
    acc[6] += b * b;
    acc[7] += m * b;
    acc[8] += g * b;
  }
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) part[wid][k] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    double v = part[0][k];
    for (int j = 1; j < TPB / kWave; ++j) v += part[j][k];
    acc[k] = v;
  }
  const double inv = 1.0 / count, al = a.alpha;
  const double C00 = acc[2] * inv + al, C01 = acc[3] * inv, C02 = acc[0] * inv;
  const double C11 = acc[4] * inv + al, C12 = acc[1] * inv, C22 = 1.0 + al;
  const double v0 = acc[7] * inv, v1 = acc[8] * inv, v2 = acc[5] * inv;
  // c = C^-1 Atb through the adjugate of the symmetric 3x3 C
  const double A00 = C11 * C22 - C12 * C12, A01 = C02 * C12 - C01 * C22, A02 = C01 * C12 - C02 * C11;
  const double A11 = C00 * C22 - C02 * C02, A12 = C01 * C02 - C00 * C12, A22 = C00 * C11 - C01 * C01;
  const double rdet = 1.0 / (C00 * A00 + C01 * A01 + C02 * A02);
  const double c0 = (A00 * v0 + A01 * v1 + A02 * v2) * rdet;
  const double c1 = (A01 * v0 + A11 * v1 + A12 * v2) * rdet;
  const double c2 = (A02 * v0 + A12 * v1 + A22 * v2) * rdet;
  const double mb = v2, sb2 = acc[6] * inv;
  const double var = sb2 - mb * mb;
  const double Cc0 = C00 * c0 + C01 * c1 + C02 * c2, Cc1 = C01 * c0 + C11 * c1 + C12 * c2, Cc2 = C02 * c0 + C12 * c1 + C22 * c2;
  const double dist = sb2 + (c0 * Cc0 + c1 * Cc1 + c2 * Cc2) - 2.0 * (c0 * v0 + c1 * v1 + c2 * v2);
  const double num = var - dist;
  const bool open_den = var >= a.beta;
  const double den = open_den ? var : a.beta;
  const double raw = num / den;
  const bool open = raw >= 0.0 && raw <= 1.0;
  const double sym = raw < 0.0 ? 0.0 : (raw > 1.0 ? 1.0 : raw);       // NaN stays NaN, as torch.clamp
  double* o = ws + ((long long)p * a.R + ri) * kCoef;
  o[0] = open ? 2.0 * inv / den : 0.0;
  o[1] = open && open_den ? 2.0 * inv * num / (den * den) : 0.0;
  o[2] = c0;
  o[3] = c1;
  o[4] = c2;
  o[5] = mb;
  o[6] = sym;
  o[7] = 0.0;
}

// out[p] = mean over the radii of sym (reduce_mean == 0), or out[0] = the mean of that over the B patches
__global__ __launch_bounds__(TPB) void lc2_out_kernel(const double* __restrict__ ws, int B, int R, int reduce_mean,
                                                      float* __restrict__ out) {
  __shared__ double scratch[TPB / kWave];
  double acc = 0.0;
  for (int p = threadIdx.x; p < B; p += TPB) {
    double s = 0.0;
    for (int ri = 0; ri < R; ++ri) s += ws[((long long)p * R + ri) * kCoef + 6];
    s /= R;
    if (reduce_mean) acc += s;
    else out[p] = (float)s;
  }
  if (reduce_mean) {
    acc = block_sum(acc, scratch);
    if (threadIdx.x == 0) out[0] = (float)(acc / B);
  }
}

// tile q = ((n S + z) nyb + yb) nxb + xb of the backward: 64 voxels of a row (threadIdx.x) x 4 rows of one z slice (threadIdx.y)
__device__ __forceinline__ void lc2_bwd_tile(const Lc2Args& a, const double* __restrict__ ws, const float* __restrict__ gout,
                                             int reduce_mean, float* __restrict__ dus, float* __restrict__ dmr, int nxb, int nyb,
                                             int q) {
  const int xb = q % nxb;
  q /= nxb;
  const int yb = q % nyb;
  const int nz = q / nyb;                       // n S + z
  const int x = xb * kWave + threadIdx.x, y = yb * kRows + threadIdx.y;
  if (x >= a.S || y >= a.S) return;
  const int n = nz / a.S, z = nz - n * a.S;
  const long long sy = a.S, sz = (long long)a.S * a.S;
  const long long j = (long long)nz * sz + (long long)y * sy + x;
  {
    // a row (one wave: y and z are wave-uniform) outside every patch's largest halo band in y or z: zeros, nothing else
    const int pz = z / a.P, py = y / a.P, lz = z - pz * a.P, ly = y - py * a.P;
    if (pz >= a.nP || py >= a.nP || lz < a.hlo || lz > a.P - 1 - a.hlo || ly < a.hlo || ly > a.P - 1 - a.hlo) {
      if (dus) dus[j] = 0.f;
      if (dmr) dmr[j] = 0.f;
      return;
    }
  }
  double gu = 0.0, gm = 0.0;
  bool touched = false;
  int p = 0;
  const int pz = z / a.P, py = y / a.P, px = x / a.P;
  if (pz < a.nP && py < a.nP && px < a.nP) {
    const int l[3] = {x - px * a.P, y - py * a.P, z - pz * a.P};      // local coordinates (x, y, z) in the patch
    const long long stride[3] = {1, sy, sz};
    p = ((n * a.nP + pz) * a.nP + py) * a.nP + px;
    for (int ri = 0; ri < a.R; ++ri) {
      const int w = 2 * a.radius[ri] + 1, pad = (a.P - w) / 2;
      if (l[0] < pad - 1 || l[0] > pad + w || l[1] < pad - 1 || l[1] > pad + w || l[2] < pad - 1 || l[2] > pad + w) continue;
      touched = true;
      const double* c = ws + ((long long)p * a.R + ri) * kCoef;
      const double s = c[0], t = c[1], c0 = c[2], c1 = c[3], c2 = c[4], mb = c[5];
      if (s == 0.0 && t == 0.0) continue;                              // clamp closed: no gradient from this crop
      const bool in0 = l[0] >= pad && l[0] < pad + w, in1 = l[1] >= pad && l[1] < pad + w, in2 = l[2] >= pad && l[2] < pad + w;
      if (in0 && in1 && in2) {
        double d[3];
        const double m = a.mr[j], b = a.us[j], g = grad_norm(a.mr, j, sy, sz, d);
        const double e = c0 * m + c1 * g + c2;
        gu += s * (e - mb) - t * (b - mb);
        gm += s * c0 * (b - e);
      }
      // crop neighbour i = j + sgn e_k: d_k(i) = mr(i - e_k) - mr(i + e_k) holds mr_j with the sign sgn
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const bool other = k == 0 ? (in1 && in2) : (k == 1 ? (in0 && in2) : (in0 && in1));
        if (!other) continue;
#pragma unroll
        for (int sgn = -1; sgn <= 1; sgn += 2) {
          const int lk = l[k] + sgn;
          if (lk < pad || lk >= pad + w) continue;
          const long long i = j + sgn * stride[k];
          double d[3];
          const double g = grad_norm(a.mr, i, sy, sz, d);
          if (g > 0.0) {
            const double G = s * c1 * ((double)a.us[i] - (c0 * (double)a.mr[i] + c1 * g + c2));
            gm += sgn * (G * d[k] / g);
          }
        }
      }
    }
  }
  float ou = 0.f, om = 0.f;
  if (touched) {
    const double scale = (double)gout[reduce_mean ? 0 : p] / (reduce_mean ? (double)a.R * a.B : (double)a.R);
    ou = (float)(gu * scale);
    om = (float)(gm * scale);
  }
  if (dus) dus[j] = ou;
  if (dmr) dmr[j] = om;
}

// block (64, 4), one tile per workgroup
__global__ __launch_bounds__(TPB) void lc2_bwd_kernel(Lc2Args a, const double* __restrict__ ws, const float* __restrict__ gout,
                                                      int reduce_mean, float* __restrict__ dus, float* __restrict__ dmr) {
  lc2_bwd_tile(a, ws, gout, reduce_mean, dus, dmr, (a.S + kWave - 1) / kWave, (a.S + kRows - 1) / kRows, blockIdx.x);
}

int lc2_setup(Lc2Args& a, const float* us, const float* mr, int N, int S, int P, const int* radii, int R, double alpha,
              double beta) {
  if (!us || !mr || !radii || N < 1 || P < 3 || S < P || R < 1 || R > kMaxRadii) return -22;
  const long long nblk = (long long)N * S * ((S + kRows - 1) / kRows) * ((S + kWave - 1) / kWave);
  if (nblk > 0x7fffffffll) return -22;                                // the backward's tile index is an int
  a.us = us;
  a.mr = mr;
  a.N = N;
  a.S = S;
  a.P = P;
  a.nP = S / P;
  const long long B = (long long)N * a.nP * a.nP * a.nP;
  if (B < 1 || B > 0x7fffffffll) return -22;
  a.B = (int)B;
  a.R = R;
  for (int k = 0; k < kMaxRadii; ++k) a.radius[k] = 0;
  for (int k = 0; k < R; ++k) {
    const int r = radii[k];
    if (r < 0 || r > P || 2 * r + 1 > P - 2 || (P - 2 * r - 1) % 2 != 0) return -22;   // pad >= 1, the crop exactly w wide
    if (r > kMaxRadius) return -22;                                                     // w^3 fits an int
    a.radius[k] = r;
    if (k == 0 || (P - 2 * r - 1) / 2 - 1 < a.hlo) a.hlo = (P - 2 * r - 1) / 2 - 1;
  }
  a.alpha = alpha;
  a.beta = beta;
  return 0;
}
}  // namespace

/* Workspace of kmh_lc2_fwd / kmh_lc2_bwd: 8 doubles per (patch, radius). */
KMH_API size_t kmh_lc2_ws_bytes(int num_patches, int num_radii) {
  if (num_patches < 0 || num_radii < 0) return 0;
  return (size_t)num_patches * num_radii * kCoef * sizeof(double);
}

/* us, mr: (N, S, S, S) float32 contiguous; P^3 patches tiled without overlap (nP = S / P per axis, the remainder dropped; patch
 * index ((n nP + pz) nP + py) nP + px); radii: HOST array of R <= 8 radii, each with P - (2r + 1) even and >= 2, r <= 511.
 * out: B = N nP^3 floats (reduce_mean == 0: per patch, the mean of sym over the radii) or one float (reduce_mean != 0: the mean
 * over the patches).  ws: kmh_lc2_ws_bytes(B, R) bytes, kept for kmh_lc2_bwd.  keymorph/loss_ops.py:262-302 and 335-391 */
KMH_API int kmh_lc2_fwd(const float* us, const float* mr, int N, int S, int P, const int* radii, int R, double alpha,
                        double beta, int reduce_mean, void* ws, float* out, void* stream) {
  Lc2Args a;
  const int rc = lc2_setup(a, us, mr, N, S, P, radii, R, alpha, beta);
  if (rc) return rc;
  if (!ws || !out) return -22;
  hipStream_t s = (hipStream_t)stream;
  lc2_fwd_kernel<<<dim3((unsigned)a.B, (unsigned)R), TPB, 0, s>>>(a, (double*)ws);
  lc2_out_kernel<<<1, TPB, 0, s>>>((const double*)ws, a.B, R, reduce_mean, out);
  return KMH_LAUNCH_CHECK();
}

/* Gradients of kmh_lc2_fwd's output: gout holds B floats (reduce_mean == 0) or one float; ws as written by kmh_lc2_fwd for the
 * same arguments.  dus, dmr: (N, S, S, S) float32, every voxel written (zeros outside the crops and their 1-voxel halos); either
 * may be null.  keymorph/loss_ops.py:262-302 and 335-391 (the reference's autograd) */
KMH_API int kmh_lc2_bwd(const float* us, const float* mr, const float* gout, int N, int S, int P, const int* radii, int R,
                        int reduce_mean, const void* ws, float* dus, float* dmr, void* stream) {
  Lc2Args a;
  const int rc = lc2_setup(a, us, mr, N, S, P, radii, R, 0.0, 0.0);
  if (rc) return rc;
  if (!ws || !gout) return -22;
  if (!dus && !dmr) return 0;
  hipStream_t s = (hipStream_t)stream;
  const long long nblk = (long long)N * S * ((S + kRows - 1) / kRows) * ((S + kWave - 1) / kWave);
  lc2_bwd_kernel<<<(unsigned)nblk, dim3(kWave, kRows), 0, s>>>(a, (const double*)ws, gout, reduce_mean, dus, dmr);
  return KMH_LAUNCH_CHECK();
}
