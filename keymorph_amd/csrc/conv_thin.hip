// Direct fp32 3x3x3 convolutions (padding 1, NDHWC) for THIN layers: the brain extractor's Simple_Unet
// (keymorph/model.py:533-616) has layers with 1, 4 or 8 channels on one side (1 -> 4, 4 -> 8, 8 -> 1, 1 -> 1 and the
// transposed pairs of their data gradients), which the split-operand matrix kernels (conv_bf.hip, conv_wgrad.hip) are not
// built for: their vector paths want whole 8-channel input chunks and Cout % 4 == 0.  At most 27 * 8 * 16 multiply-adds per
// voxel: these layers are memory bound, so plain VALU FMAs in exact fp32 are enough.
//
//   kmh_conv3d_thin_fwd   y = conv(x, w) + bias [ReLU]             one thread per voxel, all Cout accumulators in registers
//   kmh_conv3d_thin_dgrad dx = conv^T(dz [masked], w)              the SAME kernel: the weights are staged flipped / transposed
//   kmh_conv3d_thin_wgrad dw, db = correlations of x with dz       per-block partial sums -> workspace -> fixed-order second pass
//
// A workgroup owns a 2 x 4 x 32 brick of voxels (W fastest: a wave covers two 32-voxel rows, 128 * C contiguous bytes each) and
// stages its 4 x 6 x 34 halo through LDS channel-major ([c][z][y][x]: lanes read consecutive words, no bank conflicts); the
// weights sit in LDS too and are read as wave-wide broadcasts.  Per voxel: 4 * Cin B read (+ halo overlap, 2.6x in LDS only)
// and 4 * Cout B written.  No float atomics anywhere: gradients are bitwise repeatable.
#include "common.h"

namespace {
constexpr int TPB = 256;
constexpr int TX = 32, TY = 4, TZ = 2;                      // brick = TPB voxels
constexpr int HX = TX + 2, HY = TY + 2, HZ = TZ + 2;        // halo
constexpr int HVOL = HX * HY * HZ;                          // 816 words per channel
constexpr int MAX_CIN = 8;                                  // 26 KB of halo at most
constexpr int MAX_COUT = 16;

struct Brick { int x0, y0, z0, n; };
__device__ __forceinline__ Brick brick_of(int b, int tx, int ty, int tz) {
  Brick k;
  k.x0 = (b % tx) * TX; b /= tx;
  k.y0 = (b % ty) * TY; b /= ty;
  k.z0 = (b % tz) * TZ; b /= tz;
  k.n = b;
  return k;
}

// halo of brick k of x (N, D, H, W, C) -> s[c][hz][hy][hx]; zero outside the volume; `mask` (same shape as x) | NULL zeroes
// the elements whose mask value is not > 0 (a ReLU output: the masked gradient).  A halo row is one contiguous run of
// HX * C floats in memory: consecutive threads read consecutive words.
__device__ __forceinline__ void stage_halo(const float* __restrict__ x, const float* __restrict__ mask, float* s, const Brick& k,
                                           int D, int H, int W, int C) {
  const int row = HX * C;
  for (int e = threadIdx.x; e < HZ * HY * row; e += TPB) {
    const int r = e / row, q = e - r * row;
    const int hx = q / C, c = q - hx * C;
    const int hz = r / HY, hy = r - hz * HY;
    const int gz = k.z0 + hz - 1, gy = k.y0 + hy - 1, gx = k.x0 + hx - 1;
    float v = 0.f;
    if (gz >= 0 && gz < D && gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const long long g = ((((long long)k.n * D + gz) * H + gy) * W + gx) * C + c;
      v = x[g];
      if (mask && !(mask[g] > 0.f)) v = 0.f;
    }
    s[c * HVOL + (hz * HY + hy) * HX + hx] = v;
  }
}

// transposed == 0: w (COUT, Cin, 27), sW[tap][ci][co] = w[co][ci][tap]                           (forward)
// transposed == 1: w (Cin, COUT, 27) is the FORWARD layer's filter, sW[tap][ci][co] = w[ci][co][26 - tap]   (data gradient)
template <int COUT>
__global__ __launch_bounds__(TPB) void thin_conv_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ y, int D, int H, int W, int Cin, int transposed,
                                                        int relu_out, int tx, int ty, int tz) {
  extern __shared__ float smem[];
  float* sW = smem;                             // 27 * Cin * COUT
  float* sIn = smem + 27 * Cin * COUT;          // Cin * HVOL
  const Brick k = brick_of(blockIdx.x, tx, ty, tz);
  for (int e = threadIdx.x; e < 27 * Cin * COUT; e += TPB) {
    const int co = e % COUT, ci = (e / COUT) % Cin, tap = e / (COUT * Cin);
    sW[e] = transposed ? w[(ci * COUT + co) * 27 + (26 - tap)] : w[(co * Cin + ci) * 27 + tap];
  }
  stage_halo(x, mask, sIn, k, D, H, W, Cin);
  __syncthreads();
  const int lx = threadIdx.x % TX, ly = (threadIdx.x / TX) % TY, lz = threadIdx.x / (TX * TY);
  const int gx = k.x0 + lx, gy = k.y0 + ly, gz = k.z0 + lz;
  if (gx >= W || gy >= H || gz >= D) return;
  float acc[COUT];
#pragma unroll
  for (int co = 0; co < COUT; ++co) acc[co] = bias ? bias[co] : 0.f;
  for (int tap = 0; tap < 27; ++tap) {
    const int off = ((lz + tap / 9) * HY + ly + (tap / 3) % 3) * HX + lx + tap % 3;
    for (int ci = 0; ci < Cin; ++ci) {
      const float v = sIn[ci * HVOL + off];
      const float* wr = sW + (tap * Cin + ci) * COUT;
#pragma unroll
      for (int co = 0; co < COUT; ++co) acc[co] = __fmaf_rn(v, wr[co], acc[co]);
    }
  }
  float* o = y + ((((long long)k.n * D + gz) * H + gy) * W + gx) * COUT;
#pragma unroll
  for (int co = 0; co < COUT; ++co) o[co] = relu_out ? fmaxf(acc[co], 0.f) : acc[co];
}

// ---- weight (and bias) gradient --------------------------------------------------------------------------------------
// Entry p of the result: p < 27 * Cin * Cout -> (tap, ci, co) = (p / (Cin Cout), (p / Cout) % Cin, p % Cout), the sum over
// voxels v of x[v + tap][ci] * dz[v][co]; the last Cout entries are the bias gradient, the sum of dz[v][co].  P <= WG_MAXP.
// A block walks bricks b, b + G, b + 2 G, ... (a fixed function of the shape); within a brick, work item (p, s) sums the
// voxels s, s + S, ... (S = slices = TPB / P when P < TPB, else 1) in fixed order.  Block partials go to ws[block][p];
// the second kernel adds them per entry in a fixed order, in double.
constexpr int WG_MAXP = 1024;
constexpr int WG_ITEMS = WG_MAXP / TPB;          // work items per thread at most

__global__ __launch_bounds__(TPB) void thin_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                         const float* __restrict__ dzmask, float* __restrict__ ws, int D, int H,
                                                         int W, int Cin, int Cout, int tx, int ty, int tz, int nbricks) {
  extern __shared__ float smem[];
  float* sIn = smem;                            // Cin * HVOL
  float* sD = smem + Cin * HVOL;                // Cout * TPB, channel-major
  float* sRed = sD + Cout * TPB;                // WG_MAXP
  const int PW = 27 * Cin * Cout, P = PW + Cout;
  const int S = P < TPB ? TPB / P : 1;
  const int nitems = P * S;
  float acc[WG_ITEMS];
#pragma unroll
  for (int q = 0; q < WG_ITEMS; ++q) acc[q] = 0.f;
  for (int b = blockIdx.x; b < nbricks; b += gridDim.x) {
    const Brick k = brick_of(b, tx, ty, tz);
    __syncthreads();                            // the previous brick's readers are done
    stage_halo(x, nullptr, sIn, k, D, H, W, Cin);
    for (int e = threadIdx.x; e < TPB * Cout; e += TPB) {
      const int v = e / Cout, co = e - v * Cout;
      const int gx = k.x0 + v % TX, gy = k.y0 + (v / TX) % TY, gz = k.z0 + v / (TX * TY);
      float d = 0.f;
      if (gx < W && gy < H && gz < D) {
        const long long g = ((((long long)k.n * D + gz) * H + gy) * W + gx) * Cout + co;
        d = dz[g];
        if (dzmask && !(dzmask[g] > 0.f)) d = 0.f;
      }
      sD[co * TPB + v] = d;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < WG_ITEMS; ++q) {
      const int item = threadIdx.x + q * TPB;
      if (item >= nitems) break;
      const int p = item % P, s = item / P;
      float a = acc[q];
      if (p < PW) {
        const int co = p % Cout, ci = (p / Cout) % Cin, tap = p / (Cout * Cin);
        const float* xs = sIn + ci * HVOL + ((tap / 9) * HY + (tap / 3) % 3) * HX + tap % 3;
        const float* ds = sD + co * TPB;
        for (int v = s; v < TPB; v += S)
          a = __fmaf_rn(xs[((v / (TX * TY)) * HY + (v / TX) % TY) * HX + v % TX], ds[v], a);
      } else {
        const float* ds = sD + (p - PW) * TPB;
        for (int v = s; v < TPB; v += S) a = __fadd_rn(a, ds[v]);
      }
      acc[q] = a;
    }
  }
  // slices of one entry are added in slice order by one thread
  __syncthreads();
#pragma unroll
  for (int q = 0; q < WG_ITEMS; ++q) {
    const int item = threadIdx.x + q * TPB;
    if (item < nitems) sRed[item] = acc[q];       // item = s * P + p
  }
  __syncthreads();
  for (int p = threadIdx.x; p < P; p += TPB) {
    float a = sRed[p];
    for (int s = 1; s < S; ++s) a = __fadd_rn(a, sRed[s * P + p]);
    ws[(long long)blockIdx.x * P + p] = a;
  }
}

// one block per entry p: thread t adds the partials of blocks t, t + TPB, ... in double, then a fixed tree over the threads
__global__ __launch_bounds__(TPB) void thin_wgrad_final_kernel(const float* __restrict__ ws, int nblocks, int Cin, int Cout,
                                                               float* __restrict__ dw, float* __restrict__ db) {
  __shared__ double red[TPB];
  const int PW = 27 * Cin * Cout, P = PW + Cout, p = blockIdx.x;
  double a = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += TPB) a += (double)ws[(long long)b * P + p];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int h = TPB / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (p < PW) {
      const int co = p % Cout, ci = (p / Cout) % Cin, tap = p / (Cout * Cin);
      dw[(co * Cin + ci) * 27 + tap] = (float)red[0];
    } else if (db) {
      db[p - PW] = (float)red[0];
    }
  }
}

struct Geo { int tx, ty, tz, nbricks; bool ok; };
Geo geometry(int N, int D, int H, int W, int Cin, int Cout) {
  Geo g{0, 0, 0, 0, false};
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return g;
  const long long V = (long long)N * D * H * W;
  if (V * (Cin > Cout ? Cin : Cout) >= (1ll << 31)) return g;
  g.tx = ceil_div(W, TX); g.ty = ceil_div(H, TY); g.tz = ceil_div(D, TZ);
  const long long nb = (long long)g.tx * g.ty * g.tz * N;
  if (nb >= (1ll << 31)) return g;
  g.nbricks = (int)nb;
  g.ok = true;
  return g;
}

int wgrad_blocks(int nbricks) { return nbricks < 1024 ? nbricks : 1024; }

template <int COUT>
int launch_conv(const float* x, const float* mask, const float* w, const float* bias, float* y, const Geo& g, int D, int H,
                int W, int Cin, int transposed, int relu_out, hipStream_t s) {
  const size_t lds = (size_t)(27 * Cin * COUT + Cin * HVOL) * sizeof(float);
  thin_conv_kernel<COUT><<<g.nbricks, TPB, lds, s>>>(x, mask, w, bias, y, D, H, W, Cin, transposed, relu_out, g.tx, g.ty, g.tz);
  return KMH_LAUNCH_CHECK();
}

int conv_any(const float* x, const float* mask, const float* w, const float* bias, float* y, int N, int D, int H, int W, int Cin,
             int Cout, int transposed, int relu_out, void* stream) {
  const Geo g = geometry(N, D, H, W, Cin, Cout);
  if (!g.ok || !x || !w || !y || Cin > MAX_CIN || Cout > MAX_COUT) return -22;
  hipStream_t s = (hipStream_t)stream;
  switch (Cout) {
    case 1: return launch_conv<1>(x, mask, w, bias, y, g, D, H, W, Cin, transposed, relu_out, s);
    case 4: return launch_conv<4>(x, mask, w, bias, y, g, D, H, W, Cin, transposed, relu_out, s);
    case 8: return launch_conv<8>(x, mask, w, bias, y, g, D, H, W, Cin, transposed, relu_out, s);
    case 16: return launch_conv<16>(x, mask, w, bias, y, g, D, H, W, Cin, transposed, relu_out, s);
    default: return -22;
  }
}
}  // namespace

/* 1 if kmh_conv3d_thin_fwd / _dgrad serve a launch with these input / output channel counts (of THAT launch). */
KMH_API int kmh_conv3d_thin_ok(int Cin, int Cout) {
  return (Cin >= 1 && Cin <= MAX_CIN && (Cout == 1 || Cout == 4 || Cout == 8 || Cout == 16)) ? 1 : 0;
}
/* 1 if kmh_conv3d_thin_wgrad serves a layer Cin -> Cout. */
KMH_API int kmh_conv3d_thin_wgrad_ok(int Cin, int Cout) {
  return (Cin >= 1 && Cin <= MAX_CIN && Cout >= 1 && Cout <= MAX_COUT && 27 * Cin * Cout + Cout <= WG_MAXP) ? 1 : 0;
}

/* y (N,D,H,W,Cout) = conv3x3x3(x (N,D,H,W,Cin), w (Cout,Cin,3,3,3), padding 1) + bias (Cout)|NULL, ReLU if relu_out. */
KMH_API int kmh_conv3d_thin_fwd(const float* x, const float* w, const float* bias, float* y, int N, int D, int H, int W, int Cin,
                                int Cout, int relu_out, void* stream) {
  return conv_any(x, nullptr, w, bias, y, N, D, H, W, Cin, Cout, 0, relu_out, stream);
}

/* dx (N,D,H,W,Cin) = data gradient of the layer w (Cout,Cin,3,3,3) for dz (N,D,H,W,Cout); dzmask (dz's shape)|NULL: the
 * layer's ReLU output, dz counts as 0 where it is not > 0. */
KMH_API int kmh_conv3d_thin_dgrad(const float* dz, const float* dzmask, const float* w, float* dx, int N, int D, int H, int W,
                                  int Cin, int Cout, void* stream) {
  return conv_any(dz, dzmask, w, nullptr, dx, N, D, H, W, Cout, Cin, 1, 0, stream);
}

KMH_API size_t kmh_conv3d_thin_wgrad_ws_bytes(int N, int D, int H, int W, int Cin, int Cout) {
  const Geo g = geometry(N, D, H, W, Cin, Cout);
  if (!g.ok) return 0;
  return (size_t)wgrad_blocks(g.nbricks) * (27 * Cin * Cout + Cout) * sizeof(float);
}

/* dw (Cout,Cin,3,3,3) and db (Cout)|NULL of the layer for input x (N,D,H,W,Cin) and output gradient dz (N,D,H,W,Cout)
 * [masked by dzmask as above].  Partial sums go through ws (kmh_conv3d_thin_wgrad_ws_bytes) and are added in a fixed order:
 * two calls give bit-identical results. */
KMH_API int kmh_conv3d_thin_wgrad(const float* x, const float* dz, const float* dzmask, float* dw, float* db, int N, int D,
                                  int H, int W, int Cin, int Cout, void* ws, void* stream) {
  const Geo g = geometry(N, D, H, W, Cin, Cout);
  if (!g.ok || !x || !dz || !dw || !ws || !kmh_conv3d_thin_wgrad_ok(Cin, Cout)) return -22;
  hipStream_t s = (hipStream_t)stream;
  const int nb = wgrad_blocks(g.nbricks), P = 27 * Cin * Cout + Cout;
  const size_t lds = (size_t)(Cin * HVOL + Cout * TPB + WG_MAXP) * sizeof(float);
  thin_wgrad_kernel<<<nb, TPB, lds, s>>>(x, dz, dzmask, (float*)ws, D, H, W, Cin, Cout, g.tx, g.ty, g.tz, g.nbricks);
  if (int e = KMH_LAUNCH_CHECK()) return e;
  thin_wgrad_final_kernel<<<P, TPB, 0, s>>>((const float*)ws, nb, Cin, Cout, dw, db);
  return KMH_LAUNCH_CHECK();
}
