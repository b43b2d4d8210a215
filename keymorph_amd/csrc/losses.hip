// Reductions that follow the sampler but sample nothing themselves: MSE and soft Dice sums with their backward pieces
// (keymorph/loss_ops.py:9-63), argmax -> one-hot, and the Jacobian determinant of a dense map.
#include "sampler_taps.h"

namespace {

// ----------------------------------------------------------------------------------------------
// reductions
constexpr int RED_BLOCKS = 2048;

__global__ __launch_bounds__(TPB) void sqdiff_partial_kernel(const float* __restrict__ a,
                                                             const float* __restrict__ b, long long n,
                                                             double* __restrict__ partial) {
  float acc = 0.f;
  double dacc = 0.0;
  const long long n4 = n >> 2;
  const float4* a4 = reinterpret_cast<const float4*>(a);
  const float4* b4 = reinterpret_cast<const float4*>(b);
  int cnt = 0;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n4; i += (long long)gridDim.x * TPB) {
    float4 p = a4[i], q = b4[i];
    float d0 = p.x - q.x, d1 = p.y - q.y, d2 = p.z - q.z, d3 = p.w - q.w;
    acc += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    if (++cnt == 64) { dacc += acc; acc = 0.f; cnt = 0; }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    float d = a[n4 * 4 + threadIdx.x] - b[n4 * 4 + threadIdx.x];
    acc += d * d;
  }
  dacc += acc;
  __shared__ double red[TPB / kWave];
  double s = block_sum<double>(dacc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(TPB) void finalize_mean_kernel(const double* __restrict__ partial, int np,
                                                            double inv_n, float* __restrict__ out) {
  // fixed summation order (deterministic); 8 independent loads in flight per lane
  double s8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int i = threadIdx.x;
  for (; i + 7 * TPB < np; i += 8 * TPB) {
#pragma unroll
    for (int k = 0; k < 8; ++k) s8[k] += partial[i + k * TPB];
  }
  for (int k = 0; i < np; i += TPB, ++k) s8[k & 7] += partial[i];
  double s = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
  __shared__ double red[TPB / kWave];
  s = block_sum<double>(s, red);
  if (threadIdx.x == 0) out[0] = (float)(s * inv_n);
}

__global__ __launch_bounds__(TPB) void mse_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                      const float* __restrict__ gscale, long long n,
                                                      float* __restrict__ da) {
  const float s = gscale[0] * 2.f / (float)n;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB)
    da[i] = s * (a[i] - b[i]);
}

// Dice: per row r: {sum t*p, sum p*p, sum t*t}.  grid (bx, R); partial (R, bx, 3) doubles.
__global__ __launch_bounds__(TPB) void dice_partial_kernel(const float* __restrict__ pred,
                                                           const float* __restrict__ target, long long V,
                                                           double* __restrict__ partial) {
  const int r = blockIdx.y;
  const float* p = pred + (long long)r * V;
  const float* t = target + (long long)r * V;
  double s0 = 0, s1 = 0, s2 = 0;
  float a0 = 0, a1 = 0, a2 = 0;
  int cnt = 0;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < V; i += (long long)gridDim.x * TPB) {
    float pv = p[i], tv = t[i];
    a0 += tv * pv; a1 += pv * pv; a2 += tv * tv;
    if (++cnt == 256) { s0 += a0; s1 += a1; s2 += a2; a0 = a1 = a2 = 0.f; cnt = 0; }
  }
  s0 += a0; s1 += a1; s2 += a2;
  __shared__ double red[TPB / kWave];
  s0 = block_sum<double>(s0, red);
  s1 = block_sum<double>(s1, red);
  s2 = block_sum<double>(s2, red);
  if (threadIdx.x == 0) {
    double* o = partial + ((long long)r * gridDim.x + blockIdx.x) * 3;
    o[0] = s0; o[1] = s1; o[2] = s2;
  }
}

__global__ __launch_bounds__(TPB) void dice_finalize_kernel(const double* __restrict__ partial, int nb,
                                                            float* __restrict__ sums) {
  const int r = blockIdx.x;
  double s0 = 0, s1 = 0, s2 = 0;
  for (int i = threadIdx.x; i < nb; i += TPB) {
    const double* o = partial + ((long long)r * nb + i) * 3;
    s0 += o[0]; s1 += o[1]; s2 += o[2];
  }
  __shared__ double red[TPB / kWave];
  s0 = block_sum<double>(s0, red);
  s1 = block_sum<double>(s1, red);
  s2 = block_sum<double>(s2, red);
  if (threadIdx.x == 0) { sums[r * 3] = (float)s0; sums[r * 3 + 1] = (float)s1; sums[r * 3 + 2] = (float)s2; }
}

__global__ __launch_bounds__(TPB) void rows_axpby_kernel(const float* __restrict__ t, const float* __restrict__ p,
                                                         const float* __restrict__ ca, const float* __restrict__ cb,
                                                         long long V, float* __restrict__ out) {
  const int r = blockIdx.y;
  const float a = ca[r], b = cb[r];
  const long long base = (long long)r * V;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < V; i += (long long)gridDim.x * TPB)
    out[base + i] = a * t[base + i] + b * p[base + i];
}

__global__ __launch_bounds__(TPB) void argmax_onehot_kernel(const float* __restrict__ pred, int C, long long V,
                                                            float* __restrict__ out) {
  const int n = blockIdx.y;
  const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
  if (i >= V) return;
  const float* p = pred + (long long)n * C * V + i;
  // torch.argmax's rule: the first NaN if there is one, otherwise the first maximum
  float best = p[0];
  int bi = 0;
  for (int c = 1; c < C; ++c) {
    float v = p[(long long)c * V];
    if (v > best || (v != v && best == best)) { best = v; bi = c; }
  }
  float* o = out + (long long)n * C * V + i;
  for (int c = 0; c < C; ++c) o[(long long)c * V] = (c == bi) ? 1.f : 0.f;
}

}  // namespace

// ----------------------------------------------------------------------------------------------
// Jacobian determinant of a dense map (keymorph/loss_ops.py:161-247, eval metrics jdstd / jdlessthan0):
// J[a][c] = d disp_c / d axis_a by central differences (0.5 (f[i+1] - f[i-1]), zero outside the volume) + I, on
// the volume cropped by 2 voxels per side.  One pass: optional per-voxel determinant + {sum, sum^2, #(<= 0)}.
__global__ __launch_bounds__(TPB) void jacdet_kernel(const float* __restrict__ disp, long long cstride,
                                                     long long vstride, int D, int H, int W, float* __restrict__ jd,
                                                     double* __restrict__ partial /* (nblocks, 3) */) {
  const int Di = D - 4, Hi = H - 4, Wi = W - 4;
  const long long total = (long long)Di * Hi * Wi;
  double s = 0, ss = 0, neg = 0;
  for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total; e += (long long)gridDim.x * TPB) {
    const int x = (int)(e % Wi) + 2, y = (int)((e / Wi) % Hi) + 2, z = (int)(e / ((long long)Wi * Hi)) + 2;
    float J[3][3];   // [axis a][component c]
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* p = disp + c * cstride;
      auto at = [&](int zz, int yy, int xx) { return p[(((long long)zz * H + yy) * W + xx) * vstride]; };
      J[0][c] = 0.5f * at(z + 1, y, x) - 0.5f * at(z - 1, y, x);
      J[1][c] = 0.5f * at(z, y + 1, x) - 0.5f * at(z, y - 1, x);
      J[2][c] = 0.5f * at(z, y, x + 1) - 0.5f * at(z, y, x - 1);
    }
    J[0][0] += 1.f; J[1][1] += 1.f; J[2][2] += 1.f;
    // same expansion (and association) as the reference
    const float det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) -
                      J[1][0] * (J[0][1] * J[2][2] - J[0][2] * J[2][1]) +
                      J[2][0] * (J[0][1] * J[1][2] - J[0][2] * J[1][1]);
    if (jd) jd[e] = det;
    s += det; ss += (double)det * det; neg += det <= 0.f ? 1.0 : 0.0;
  }
  __shared__ double red[TPB / kWave];
  s = block_sum<double>(s, red);
  ss = block_sum<double>(ss, red);
  neg = block_sum<double>(neg, red);
  if (threadIdx.x == 0) { partial[blockIdx.x * 3] = s; partial[blockIdx.x * 3 + 1] = ss; partial[blockIdx.x * 3 + 2] = neg; }
}

__global__ __launch_bounds__(TPB) void jacdet_final_kernel(const double* __restrict__ partial, int nb, double count,
                                                           double* __restrict__ out /* mean, std (ddof 0), #<=0, count */) {
  double s = 0, ss = 0, neg = 0;
  for (int i = threadIdx.x; i < nb; i += TPB) { s += partial[i * 3]; ss += partial[i * 3 + 1]; neg += partial[i * 3 + 2]; }
  __shared__ double red[TPB / kWave];
  s = block_sum<double>(s, red);
  ss = block_sum<double>(ss, red);
  neg = block_sum<double>(neg, red);
  if (threadIdx.x == 0) {
    const double mean = s / count;
    double var = ss / count - mean * mean;
    if (var < 0) var = 0;
    out[0] = mean; out[1] = sqrt(var); out[2] = neg; out[3] = count;
  }
}

int kmh_launch_finalize_mean(const double* partial, int np, double inv_n, float* out, hipStream_t s) {
  finalize_mean_kernel<<<1, TPB, 0, s>>>(partial, np, inv_n, out);
  return KMH_LAUNCH_CHECK();
}

KMH_API int kmh_mse_fwd(const float* a, const float* b, long long n, float* out, void* ws, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int nb = (int)((n / 4 + TPB - 1) / TPB);
  if (nb > RED_BLOCKS) nb = RED_BLOCKS;
  if (nb < 1) nb = 1;
  sqdiff_partial_kernel<<<nb, TPB, 0, s>>>(a, b, n, (double*)ws);
  return kmh_launch_finalize_mean((const double*)ws, nb, 1.0 / (double)n, out, s);
}

KMH_API int kmh_mse_bwd(const float* a, const float* b, const float* gscale, long long n, float* da,
                        void* stream) {
  int nb = (int)((n + TPB - 1) / TPB);
  if (nb > 4096) nb = 4096;
  mse_bwd_kernel<<<nb, TPB, 0, (hipStream_t)stream>>>(a, b, gscale, n, da);
  return KMH_LAUNCH_CHECK();
}

KMH_API int kmh_dice_sums(const float* pred, const float* target, int R, long long V, float* sums, void* ws,
                          void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int nb = (int)((V + TPB * 8 - 1) / (TPB * 8));
  int cap = 65536 / (R > 0 ? R : 1);
  if (cap < 1) return -22;
  if (nb > cap) nb = cap;
  if (nb > 1024) nb = 1024;
  if (nb < 1) nb = 1;
  dice_partial_kernel<<<dim3(nb, R), TPB, 0, s>>>(pred, target, V, (double*)ws);
  dice_finalize_kernel<<<R, TPB, 0, s>>>((const double*)ws, nb, sums);
  return KMH_LAUNCH_CHECK();
}

KMH_API int kmh_rows_axpby(const float* t, const float* p, const float* ca, const float* cb, int R,
                           long long V, float* out, void* stream) {
  int nb = (int)((V + TPB * 4 - 1) / (TPB * 4));
  if (nb > 2048) nb = 2048;
  if (nb < 1) nb = 1;
  rows_axpby_kernel<<<dim3(nb, R), TPB, 0, (hipStream_t)stream>>>(t, p, ca, cb, V, out);
  return KMH_LAUNCH_CHECK();
}

KMH_API int kmh_argmax_onehot(const float* pred, int N, int C, long long V, float* out, void* stream) {
  argmax_onehot_kernel<<<dim3(ceil_div(V, TPB), N), TPB, 0, (hipStream_t)stream>>>(pred, C, V, out);
  return KMH_LAUNCH_CHECK();
}

/* disp: 3 components of a (D,H,W) map, component c at disp + c*cstride, voxel v at + v*vstride (NCDHW: cstride =
 * D*H*W, vstride = 1; a permuted (D,H,W,3) grid: cstride = 1, vstride = 3).  jd (D-4,H-4,W-4) or NULL;
 * stats[4] doubles = {mean, std (ddof 0), #(det <= 0), #voxels}.  keymorph/loss_ops.py:161-247 */
KMH_API int kmh_jacobian_det(const float* disp, long long cstride, long long vstride, int D, int H, int W, float* jd,
                             double* stats, void* ws, void* stream) {
  if (D < 5 || H < 5 || W < 5) return -22;
  hipStream_t s = (hipStream_t)stream;
  const long long total = (long long)(D - 4) * (H - 4) * (W - 4);
  int nb = ceil_div(total, TPB);
  if (nb > 4096) nb = 4096;
  jacdet_kernel<<<nb, TPB, 0, s>>>(disp, cstride, vstride, D, H, W, jd, (double*)ws);
  jacdet_final_kernel<<<1, TPB, 0, s>>>((const double*)ws, nb, (double)total, stats);
  return KMH_LAUNCH_CHECK();
}
