// Evaluation metrics of the reference (keymorph/loss_ops.py:66-158; callers scripts/pairwise_register_eval.py:329-331,
// groupwise_register_eval.py:492-511): the Hausdorff distance between the "brain surfaces" (channel 0) of two segmentations,
// and the label counts behind fast_dice / dice.
//
// Hausdorff: exact separable Euclidean distance transform, one pass per axis, per sample and for both masks in each launch.
//   surface_bits   S = A & ~erode(A) (6-neighbour cross, border 0) as one bit per voxel, 64 voxels of a row per word (ballot)
//   pass_w         1-D distance along W to the nearest surface bit of the row: g1 = (k sx)^2, or +inf
//   pass_col<MAP>  Meijster's lower envelope per line along H (writes g2 = g1 + (dy sy)^2), then along D: the D pass writes no
//                  map, it folds max(dist^2) over the OTHER mask's surface voxels into one int64-bit atomic max per sample
//                  (distances are >= 0, so their bit patterns order like the values).  Lines along H / D are laid out with the
//                  lanes of a block on adjacent w: every streaming load and store is coalesced.  Meijster's two stacks live in
//                  LDS at 16 bits per entry (4 B per line element); the parabola values at stack entries are gathered from the
//                  map (L1 / L2).
// Every value is (((kx sx)^2 + (ky sy)^2) + (kz sz)^2) of integer offsets, evaluated in fp64 in that order.  For the reference's
// sampling (1.25, 1.25, 10) every term is a multiple of 1/16 far below 2^53: the map is exact and sqrt of the max equals the value
// scipy's feature transform + fp64 sqrt produces.
#include "common.h"

namespace {
constexpr int TPB = 256;
constexpr int kMaxLine = 16384;          // LDS stacks: LPB lines x L entries x 4 B <= 64 KiB with LPB >= 1

// dtype codes of the C ABI: 0 f32, 1 f64, 2 f16, 3 bf16, 4 one byte (bool / uint8 / int8), 5 int16, 6 int32, 7 int64.
// "!= 0" on the bit pattern: floats ignore the sign bit (-0.0 is zero, NaN and denormals are set), integers compare every bit.
__device__ __forceinline__ bool nonzero(const unsigned char* p, int dt, long long i) {
  switch (dt) {
    case 0: return (((const unsigned*)p)[i] & 0x7fffffffu) != 0u;
    case 1: return (((const unsigned long long*)p)[i] & 0x7fffffffffffffffull) != 0ull;
    case 2:
    case 3: return (((const unsigned short*)p)[i] & 0x7fffu) != 0u;
    case 4: return p[i] != 0;
    case 5: return ((const unsigned short*)p)[i] != 0u;
    case 6: return ((const unsigned*)p)[i] != 0u;
    default: return ((const unsigned long long*)p)[i] != 0ull;
  }
}

struct EdtArgs {
  const unsigned char* src[2];   // channel 0 of one sample, (D, H, W) contiguous
  int dt[2];
  unsigned long long* bits[2];   // D*H rows x nw words
  double* g1[2];                 // D*H*W
  double* g2[2];
  int D, H, W, nw;
  double sz, sy, sx;
};

// one wave = 64 consecutive voxels of one row; blockIdx.y = mask
__global__ __launch_bounds__(TPB) void surface_bits_kernel(EdtArgs a) {
  const int m = blockIdx.y;
  const long long wave = ((long long)blockIdx.x * TPB + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const long long rows = (long long)a.D * a.H;
  if (wave >= rows * a.nw) return;                   // wave-uniform
  const long long row = wave / a.nw;
  const int x = (int)(wave % a.nw) * 64 + lane;
  const int d = (int)(row / a.H), h = (int)(row % a.H);
  const unsigned char* s = a.src[m];
  const int dt = a.dt[m];
  bool surf = false;
  if (x < a.W) {
    const long long HW = (long long)a.H * a.W, v = row * a.W + x;
    if (nonzero(s, dt, v)) {
      const bool inner = d > 0 && d < a.D - 1 && h > 0 && h < a.H - 1 && x > 0 && x < a.W - 1 &&
                         nonzero(s, dt, v - 1) && nonzero(s, dt, v + 1) && nonzero(s, dt, v - a.W) &&
                         nonzero(s, dt, v + a.W) && nonzero(s, dt, v - HW) && nonzero(s, dt, v + HW);
      surf = !inner;
    }
  }
  const unsigned long long word = __ballot(surf);
  if (lane == 0) a.bits[m][wave] = word;
}

// g1[v] = (k sx)^2 with k = distance along W to the nearest surface bit of the row; +inf for a row without one
__global__ __launch_bounds__(TPB) void pass_w_kernel(EdtArgs a) {
  const int m = blockIdx.y;
  const long long V = (long long)a.D * a.H * a.W;
  const long long v = (long long)blockIdx.x * TPB + threadIdx.x;
  if (v >= V) return;
  const long long row = v / a.W;
  const int x = (int)(v % a.W), c = x >> 6, b = x & 63;
  const unsigned long long* rw = a.bits[m] + row * a.nw;
  int k = -1;
  unsigned long long w = rw[c] & (b == 63 ? ~0ull : ((2ull << b) - 1ull));   // bits <= x
  int cl = c;
  while (w == 0ull && cl > 0) w = rw[--cl];
  if (w) k = x - (cl * 64 + 63 - __clzll((long long)w));
  w = rw[c] & (~0ull << b);                                                  // bits >= x
  int cr = c;
  while (w == 0ull && cr < a.nw - 1) w = rw[++cr];
  if (w) {
    const int r = cr * 64 + __ffsll((long long)w) - 1 - x;
    if (k < 0 || r < k) k = r;
  }
  double g = __builtin_huge_val();
  if (k >= 0) {
    const double dx = (double)k * a.sx;
    g = dx * dx;
  }
  a.g1[m][v] = g;
}

// Meijster's lower envelope along one axis: lines (o, w), element p at base + p * stride with base = o * ostride + w.
// MAP = 0 (the H pass): g1 -> g2.  MAP = 1 (the D pass, evaluation): max over the other mask's surface voxels into
// out_bits[0] (int64 atomic max).  MAP = 2 (the D pass, distance map of mask 0 for tests): g2 -> out_map.
// Block = LPB lanes on LPB adjacent w of one o; blockIdx.y = mask.  Dynamic LDS: 2 stacks x L x LPB uint16.
template <int MAP>
__global__ __launch_bounds__(64) void pass_col_kernel(EdtArgs a, int L, long long stride, long long ostride, int LPB,
                                                      double sp, long long* out_bits, double* out_map) {
  extern __shared__ unsigned short stk[];
  const int m = blockIdx.y;
  const int nwb = (a.W + LPB - 1) / LPB;
  const int o = blockIdx.x / nwb;
  const int lane = threadIdx.x;
  const int w = (blockIdx.x % nwb) * LPB + lane;
  const bool live = w < a.W;
  const double* g = (MAP == 0 ? a.g1[m] : a.g2[m]) + (long long)o * ostride + w;
  unsigned short* S = stk + lane;
  unsigned short* T = stk + (long long)L * LPB + lane;
  const double sp2 = sp * sp;

  // the evaluation pass skips lines on which the other mask has no surface voxel (o = h, the line runs along d)
  const unsigned long long* ob = a.bits[1 - m];
  bool work = live;
  if (MAP == 1 && live) {
    bool any = false;
    for (int u = 0; u < L && !any; ++u) any = (ob[((long long)u * a.H + o) * a.nw + (w >> 6)] >> (w & 63)) & 1ull;
    work = any;
  }

  long long best = -1;     // bits of the largest squared distance folded (MAP == 1)
  if (work) {
    // forward: build the envelope of the finite parabolas g[p] + ((x - p) sp)^2
    int k = -1;
    double gtop = 0.0;
    double gn = g[0];
    for (int p = 0; p < L; ++p) {
      const double gp = gn;
      if (p + 1 < L) gn = g[(long long)(p + 1) * stride];
      if (__builtin_isinf(gp)) continue;
      int s = 0;
      while (k >= 0) {
        s = S[k * LPB];
        const int t = T[k * LPB];
        const double ds = (double)(t - s) * sp, dp = (double)(t - p) * sp;
        if (gtop + ds * ds > gp + dp * dp) {
          if (--k >= 0) gtop = g[(long long)S[k * LPB] * stride];
        } else {
          break;
        }
      }
      if (k < 0) {
        k = 0;
        S[0] = (unsigned short)p;
        T[0] = 0;
        gtop = gp;
      } else {
        // first x where p is strictly lower: x* = (gp - gs + (p^2 - s^2) sp^2) / (2 (p - s) sp^2)
        const double num = (gp - gtop) + ((double)p * p - (double)s * s) * sp2;
        const double xs = num / (2.0 * (p - s) * sp2);
        if (xs < (double)(L - 1)) {
          int t = (int)floor(xs) + 1;
          const int tt = T[k * LPB];
          if (t <= tt) t = tt + 1;        // rounding at a near-tie: keep the regions ordered
          if (t < L) {
            ++k;
            S[k * LPB] = (unsigned short)p;
            T[k * LPB] = (unsigned short)t;
            gtop = gp;
          }
        }
      }
    }
    // backward: evaluate the envelope
    int sk = k >= 0 ? S[k * LPB] : 0;
    double gs = k >= 0 ? g[(long long)sk * stride] : 0.0;
    for (int u = L - 1; u >= 0; --u) {
      if (k > 0 && u < T[k * LPB]) {
        do { --k; } while (k > 0 && u < T[k * LPB]);
        sk = S[k * LPB];
        gs = g[(long long)sk * stride];
      }
      double f = __builtin_huge_val();
      if (k >= 0) {
        const double du = (double)(u - sk) * sp;
        f = gs + du * du;
      }
      if (MAP == 0) {
        a.g2[m][(long long)o * ostride + w + (long long)u * stride] = f;
      } else if (MAP == 2) {
        out_map[(long long)o * ostride + w + (long long)u * stride] = f;
      } else if ((ob[((long long)u * a.H + o) * a.nw + (w >> 6)] >> (w & 63)) & 1ull) {
        const long long fb = __double_as_longlong(f);
        if (fb > best) best = fb;
      }
    }
  }
  if (MAP == 1) {
    if (LPB == 64) {
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        const long long other = __shfl_xor(best, d, 64);
        if (other > best) best = other;
      }
      if (lane == 0 && best >= 0) atomicMax(out_bits, best);
    } else if (best >= 0) {
      atomicMax(out_bits, best);
    }
  }
}

__global__ void fill_ll_kernel(long long* p, int n, long long v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

size_t edt_ws_bytes(int D, int H, int W, int nmask) {
  const size_t V = (size_t)D * H * W, nw = ((size_t)W + 63) / 64;
  return nmask * (align256((size_t)D * H * nw * 8) + 2 * align256(V * 8));
}

int lines_per_block(int L) {
  int lpb = 64;
  while (lpb > 1 && (long long)lpb * L * 4 > 65536) lpb >>= 1;
  return lpb;
}

int edt_setup(EdtArgs& a, const void* src0, const void* src1, int dt0, int dt1, int D, int H, int W, double sz, double sy,
              double sx, void* ws, int nmask) {
  if (D < 1 || H < 1 || W < 1 || D > kMaxLine || H > kMaxLine || !ws) return -22;
  if (dt0 < 0 || dt0 > 7 || dt1 < 0 || dt1 > 7) return -22;
  if (!(sz > 0) || !(sy > 0) || !(sx > 0)) return -22;
  a.src[0] = (const unsigned char*)src0;
  a.src[1] = (const unsigned char*)src1;
  a.dt[0] = dt0;
  a.dt[1] = dt1;
  a.D = D; a.H = H; a.W = W; a.nw = (W + 63) / 64;
  a.sz = sz; a.sy = sy; a.sx = sx;
  const size_t V = (size_t)D * H * W;
  char* p = (char*)ws;
  for (int m = 0; m < 2; ++m) {
    if (m >= nmask) { a.bits[m] = a.bits[0]; a.g1[m] = a.g1[0]; a.g2[m] = a.g2[0]; continue; }
    a.bits[m] = (unsigned long long*)p; p += align256((size_t)D * H * a.nw * 8);
    a.g1[m] = (double*)p; p += align256(V * 8);
    a.g2[m] = (double*)p; p += align256(V * 8);
  }
  return 0;
}

// surface bits, the W pass and the H pass of every mask of `a` (nmask = gridDim.y)
void edt_first_passes(const EdtArgs& a, int nmask, hipStream_t s) {
  const long long waves = (long long)a.D * a.H * a.nw;
  surface_bits_kernel<<<dim3((unsigned)((waves * 64 + TPB - 1) / TPB), nmask), TPB, 0, s>>>(a);
  const long long V = (long long)a.D * a.H * a.W;
  pass_w_kernel<<<dim3((unsigned)((V + TPB - 1) / TPB), nmask), TPB, 0, s>>>(a);
  const int lpb = lines_per_block(a.H);
  const int nwb = (a.W + lpb - 1) / lpb;
  pass_col_kernel<0><<<dim3((unsigned)((long long)a.D * nwb), nmask), lpb, (size_t)lpb * a.H * 4, s>>>(
      a, a.H, a.W, (long long)a.H * a.W, lpb, a.sy, nullptr, nullptr);
}

// labels of fast_dice / dice: argmax over C channels (first NaN, else first maximum, like torch.argmax), or for BIN the
// 0/1 value of a byte map; per-block LDS histograms of |x = l|, |y = l|, |x = l and y = l|, then 64-bit atomics
template <typename T, bool BIN>
__global__ __launch_bounds__(TPB) void label_counts_kernel(const T* __restrict__ x, const T* __restrict__ y, int N, int C,
                                                           long long V, int nlab, unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned hist[];     // 3 x nlab
  for (int i = threadIdx.x; i < 3 * nlab; i += TPB) hist[i] = 0u;
  __syncthreads();
  const long long total = (long long)N * V, step = (long long)gridDim.x * TPB;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += step) {
    int lx, ly;
    if (BIN) {
      lx = x[i] != 0;
      ly = y[i] != 0;
    } else {
      const long long n = i / V, base = n * C * V + (i - n * V);
      T bx = x[base], by = y[base];
      lx = 0;
      ly = 0;
      for (int c = 1; c < C; ++c) {
        const T vx = x[base + (long long)c * V], vy = y[base + (long long)c * V];
        if (bx == bx && (vx > bx || vx != vx)) { bx = vx; lx = c; }
        if (by == by && (vy > by || vy != vy)) { by = vy; ly = c; }
      }
    }
    atomicAdd(&hist[lx], 1u);
    atomicAdd(&hist[nlab + ly], 1u);
    if (lx == ly) atomicAdd(&hist[2 * nlab + lx], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * nlab; i += TPB)
    if (hist[i]) atomicAdd(&counts[i], (unsigned long long)hist[i]);
}
}  // namespace

/* Per-sample workspace of kmh_hausdorff3d (surface bits and two fp64 maps for each of the two masks). */
KMH_API size_t kmh_hausdorff3d_ws_bytes(int D, int H, int W) { return edt_ws_bytes(D, H, W, 2); }

/* a, b: channel 0 of N samples, sample n at a + n * sstride_a elements, each (D, H, W) contiguous, element type dtype_a /
 * dtype_b (0 f32, 1 f64, 2 f16, 3 bf16, 4 one byte, 5 int16, 6 int32, 7 int64; a voxel is set iff its value != 0).
 * out_sq[n] = max(max dist_A^2 over surface(B), max dist_B^2 over surface(A)) with voxel spacing (sz, sy, sx) along (D, H, W);
 * +inf if exactly one surface is empty, NaN (all bits set) if both are.  ws: kmh_hausdorff3d_ws_bytes(D, H, W) bytes.
 * keymorph/loss_ops.py:121-158 */
KMH_API int kmh_hausdorff3d(const void* a, const void* b, int dtype_a, int dtype_b, long long sstride_a, long long sstride_b,
                            int N, int D, int H, int W, double sz, double sy, double sx, void* ws, double* out_sq,
                            void* stream) {
  if (!a || !b || !out_sq || N < 1) return -22;
  static const int esize[8] = {4, 8, 2, 2, 1, 2, 4, 8};
  EdtArgs e;
  int rc = edt_setup(e, a, b, dtype_a, dtype_b, D, H, W, sz, sy, sx, ws, 2);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  fill_ll_kernel<<<(N + 255) / 256, 256, 0, s>>>((long long*)out_sq, N, -1ll);
  const int lpb = lines_per_block(D);
  const int nwb = (W + lpb - 1) / lpb;
  for (int n = 0; n < N; ++n) {
    e.src[0] = (const unsigned char*)a + (long long)n * sstride_a * esize[dtype_a];
    e.src[1] = (const unsigned char*)b + (long long)n * sstride_b * esize[dtype_b];
    edt_first_passes(e, 2, s);
    pass_col_kernel<1><<<dim3((unsigned)((long long)H * nwb), 2), lpb, (size_t)lpb * D * 4, s>>>(
        e, D, (long long)H * W, W, lpb, sz, (long long*)out_sq + n, nullptr);
  }
  return KMH_LAUNCH_CHECK();
}

/* Workspace of kmh_edt3d_sq. */
KMH_API size_t kmh_edt3d_sq_ws_bytes(int D, int H, int W) { return edt_ws_bytes(D, H, W, 1); }

/* The squared distance map behind kmh_hausdorff3d, for one mask (tests): out[v] = squared distance from voxel v to the
 * nearest surface voxel of `a` (one (D, H, W) volume, contiguous), +inf if the surface is empty. */
KMH_API int kmh_edt3d_sq(const void* a, int dtype, int D, int H, int W, double sz, double sy, double sx, void* ws, double* out,
                         void* stream) {
  if (!a || !out) return -22;
  EdtArgs e;
  int rc = edt_setup(e, a, a, dtype, dtype, D, H, W, sz, sy, sx, ws, 1);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  edt_first_passes(e, 1, s);
  const int lpb = lines_per_block(D);
  const int nwb = (W + lpb - 1) / lpb;
  pass_col_kernel<2><<<dim3((unsigned)((long long)H * nwb), 1), lpb, (size_t)lpb * D * 4, s>>>(
      e, D, (long long)H * W, W, lpb, sz, nullptr, out);
  return KMH_LAUNCH_CHECK();
}

/* Label counts of two maps: counts[0:nlab] = |x = l|, counts[nlab:2 nlab] = |y = l|, counts[2 nlab:3 nlab] = |x = l and y = l|
 * (uint64, zeroed by the caller).  C > 0: x, y are (N, C, V) of dtype (0 f32, 1 f64) and the label is the channel argmax
 * (nlab = C).  C == 0: x, y are N * V bytes, label = (value != 0), nlab = 2.  C <= 4096.  keymorph/loss_ops.py:66-111 */
KMH_API int kmh_label_counts(const void* x, const void* y, int dtype, int N, int C, long long V, unsigned long long* counts,
                             void* stream) {
  if (!x || !y || !counts || N < 1 || V < 1 || C < 0 || C > 4096) return -22;
  const int nlab = C == 0 ? 2 : C;
  long long nb = ((long long)N * V + TPB * 16 - 1) / (TPB * 16);
  if (nb > 2048) nb = 2048;
  const size_t lds = (size_t)3 * nlab * 4;
  hipStream_t s = (hipStream_t)stream;
  if (C == 0)
    label_counts_kernel<unsigned char, true><<<(int)nb, TPB, lds, s>>>((const unsigned char*)x, (const unsigned char*)y, N, 1,
                                                                       V, nlab, counts);
  else if (dtype == 0)
    label_counts_kernel<float, false><<<(int)nb, TPB, lds, s>>>((const float*)x, (const float*)y, N, C, V, nlab, counts);
  else if (dtype == 1)
    label_counts_kernel<double, false><<<(int)nb, TPB, lds, s>>>((const double*)x, (const double*)y, N, C, V, nlab, counts);
  else
    return -22;
  return KMH_LAUNCH_CHECK();
}
