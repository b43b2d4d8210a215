// Free-form deformation: a dense sampling grid from a coarse lattice of cubic B-spline control points (ops.bspline_grid), its
// gradient back to the lattice, and the bending penalty of a lattice (ops.bspline_bending).  DESIGN.md section 8e.
//
// Definition.  ctrl (N, 3, Cz, Cy, Cx), channel k = the displacement of grid component k (x, y, z), normalised units.  An axis
// of S voxels and C control points has K = C - 3 cells over [-1, 1]; voxel centre g = (2i + 1) / S - 1 has u = (g + 1) K / 2,
// cell = clamp(floor(u), 0, C - 4), t = u - cell, and the uniform cubic B-spline weights B0..B3(t) on control points
// cell .. cell + 3.   out[n, z, y, x, :] = base + sum_{c,b,a} Bz_c By_b Bx_a ctrl[n, :, cz + c, cy + b, cx + a],
// base = the lattice identity of fields.hip (mat == NULL) or exactly what kmh_affine_grid_fwd writes for mat.
//
// u is a ratio of integers, u = (2i + 1) K / (2S), so cell and the numerator of t are computed exactly (lat_w) and t is ONE
// rounded division: a voxel centre that sits on a knot gets t = 0 of the right-hand cell, never a value either side of it.
//
// (kmh_bspline_disp_fwd: the sum alone, without the base -- what ops.svf_grid exponentiates.)
// Forward: a workgroup owns a tile of TY x TX voxels of one z-slice.  The z-contraction of the few lattice rows the tile touches
// goes to LDS once (Q[k][b][a] = sum_c Bz_c ctrl[k, cz + c, b, a]), each lane takes runs of four voxels along x, contracts y for
// the run's cell (48 LDS reads, reused while the cell does not change) and x per voxel; the kernel is bound by its 12 B store.
//
// Backward: dctrl = B^T dgrid, separable, store-and-sum (no atomics, every sum in a fixed order, so runs are bit-identical and a
// batch equals its samples): contract x into (N, D, H, Cx, 3) -- dgrid is read from HBM once, coalesced, through LDS, and each
// lane owns one (row, control point) and walks its support in ascending x --, then y into (N, D, Cy, Cx, 3), then z into dctrl.
// The second and third pass are one kernel (an axis contraction with the untouched axes flattened either side); their inputs
// are 14 % and 2 % of dgrid at 256^3 with spacing 8.  Every pass accumulates in double and stores floats.
#include "common.h"
#include "grid_coords.h"      // lin, lin_step, affine_coord_chain: the base of a grid with a matrix is kmh_affine_grid_fwd's; ident

namespace {

constexpr int TPB = 256;

struct LatW { int cell; float w[4]; };

__device__ __forceinline__ void bspline_weights(float t, float (&w)[4]) {
  const float s = 1.f - t, t2 = t * t, t3 = t2 * t;
  w[0] = s * s * s * (1.f / 6.f);
  w[1] = (3.f * t3 - 6.f * t2 + 4.f) * (1.f / 6.f);
  w[2] = (-3.f * t3 + 3.f * t2 + 3.f * t + 1.f) * (1.f / 6.f);
  w[3] = t3 * (1.f / 6.f);
}

// cell = floor((2i + 1) K / (2S)) <= K - 1 = C - 4 for every i < S (the clamp of the definition never acts on exact integers)
__device__ __forceinline__ int lat_cell(int i, int S, int C) {
  return (int)((unsigned long long)(2ll * i + 1) * (unsigned)(C - 3) / (2ull * (unsigned)S));
}
__device__ __forceinline__ LatW lat_w(int i, int S, int C) {
  const unsigned long long num = (unsigned long long)(2ll * i + 1) * (unsigned)(C - 3), den = 2ull * (unsigned)S;
  const unsigned long long cell = num / den;
  LatW r;
  r.cell = (int)cell;
  bspline_weights((float)(unsigned)(num - cell * den) / (float)(unsigned)den, r.w);
  return r;
}
// the first voxel whose cell is >= m (S if there is none): (2x + 1) K >= 2 S m  <=>  x >= ceil(2 S m / K) / 2 rounded down.
// Control point a weighs on the voxels whose cell is a - 3 .. a: [lat_first(a - 3), lat_first(a + 1)).
__host__ __device__ __forceinline__ int lat_first(long long m, int S, int K) {
  if (m <= 0) return 0;
  if (m >= K) return S;
  const unsigned long long q = (2ull * (unsigned)S * (unsigned long long)m + (unsigned)K - 1) / (unsigned)K;
  return (int)(q >> 1);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
constexpr int FWD_TX = 256, FWD_TY = 16;      // the largest tile
constexpr int FWD_Q_FLOATS = 8192;            // LDS floats for Q (3 channels x rows x columns of the lattice a tile touches)

// lattice rows (columns) that T consecutive voxels of an axis can touch: floor((T - 1) K / S) + 1 cells, + 3
static long long lat_span(int T, int S, int C) { return (long long)(T - 1) * (C - 3) / S + 5; }

// DISP: the spline alone (kmh_bspline_disp_fwd: no base is added, mat is not read) -- the same code with the base left out
template <bool DISP>
__global__ __launch_bounds__(TPB) void bspline_fwd_kernel(const float* __restrict__ ctrl, const float* __restrict__ mat,
                                                          float* __restrict__ out, int D, int H, int W, int Cz, int Cy, int Cx,
                                                          int TY, int TX, int tiles_y, int tiles_x) {
  extern __shared__ __attribute__((aligned(16))) float sQ[];
  __shared__ LatW sWx[FWD_TX], sWy[FWD_TY];
  __shared__ float sM[12];
  const int n = blockIdx.y, tid = threadIdx.x;
  const unsigned bid = blockIdx.x;
  const int tx = (int)(bid % (unsigned)tiles_x), ty = (int)((bid / (unsigned)tiles_x) % (unsigned)tiles_y);
  const int z = (int)(bid / ((unsigned)tiles_x * (unsigned)tiles_y));
  const int y0 = ty * TY, x0 = tx * TX;
  const int nyv = H - y0 < TY ? H - y0 : TY, nxv = W - x0 < TX ? W - x0 : TX;
  for (int i = tid; i < nxv; i += TPB) sWx[i] = lat_w(x0 + i, W, Cx);
  for (int i = tid; i < nyv; i += TPB) sWy[i] = lat_w(y0 + i, H, Cy);
  if (!DISP && mat && tid < 12) sM[tid] = mat[n * 12 + tid];
  const LatW wz = lat_w(z, D, Cz);
  const int cx_lo = lat_cell(x0, W, Cx), cy_lo = lat_cell(y0, H, Cy);
  const int nx = lat_cell(x0 + nxv - 1, W, Cx) + 4 - cx_lo, ny = lat_cell(y0 + nyv - 1, H, Cy) + 4 - cy_lo;
  const int plane = ny * nx;
  const long long cs = (long long)Cy * Cx;
  for (int idx = tid; idx < 3 * plane; idx += TPB) {
    const int k = idx / plane, r = idx - k * plane, b = r / nx, a = r - b * nx;
    const float* p = ctrl + (((long long)(n * 3 + k) * Cz + wz.cell) * Cy + cy_lo + b) * Cx + cx_lo + a;
    sQ[idx] = fmaf(wz.w[3], p[3 * cs], fmaf(wz.w[2], p[2 * cs], fmaf(wz.w[1], p[cs], wz.w[0] * p[0])));
  }
  __syncthreads();
  float M[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) M[i] = mat ? sM[i] : 0.f;
  const float bz = mat ? lin(z, D, lin_step(D)) : ident(z, D);
  const float sy = lin_step(H), sx = lin_step(W);
  const long long nvox = (long long)D * H * W;
  const int runs = (nxv + 3) / 4;
  for (int item = tid; item < nyv * runs; item += TPB) {
    const int ry = item / runs, rx = (item - ry * runs) * 4, y = y0 + ry;
    const LatW wy = sWy[ry];
    const int rb = (wy.cell - cy_lo) * nx - cx_lo;
    const float by = mat ? lin(y, H, sy) : ident(y, H);
    const int cnt = nxv - rx < 4 ? nxv - rx : 4;
    float r[12], P[4][3];
    int pc = -1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < cnt) {
        const LatW wx = sWx[rx + i];
        if (wx.cell != pc) {      // the y-contraction of this x-cell's four lattice columns
          pc = wx.cell;
#pragma unroll
          for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int a = 0; a < 4; ++a) {
              const float* q = sQ + k * plane + rb + pc + a;
              P[a][k] = fmaf(wy.w[3], q[3 * nx], fmaf(wy.w[2], q[2 * nx], fmaf(wy.w[1], q[nx], wy.w[0] * q[0])));
            }
        }
        const int x = x0 + rx + i;
        float b3[3];      // the base, (x, y, z)
        if (DISP) {
          b3[0] = b3[1] = b3[2] = 0.f;
        } else if (mat) {
          affine_coord_chain(M, bz, by, lin(x, W, sx), b3[0], b3[1], b3[2]);
        } else {
          b3[0] = ident(x, W); b3[1] = by; b3[2] = bz;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float d = fmaf(wx.w[3], P[3][k], fmaf(wx.w[2], P[2][k], fmaf(wx.w[1], P[1][k], wx.w[0] * P[0][k])));
          r[i * 3 + k] = DISP ? d : b3[k] + d;
        }
      }
    }
    const long long v = (long long)n * nvox + ((long long)z * H + y) * W + x0 + rx;
    float* o = out + v * 3;
    if (cnt == 4 && (v & 3) == 0) {
      float4* o4 = reinterpret_cast<float4*>(o);
      o4[0] = make_float4(r[0], r[1], r[2], r[3]);
      o4[1] = make_float4(r[4], r[5], r[6], r[7]);
      o4[2] = make_float4(r[8], r[9], r[10], r[11]);
    } else {
      for (int i = 0; i < cnt; ++i) { o[i * 3] = r[i * 3]; o[i * 3 + 1] = r[i * 3 + 1]; o[i * 3 + 2] = r[i * 3 + 2]; }
    }
  }
}

// ---- backward, pass x ------------------------------------------------------------------------------------------------------------
// t1[n, row, a, k] = sum_x Bx(x -> a) dgrid[n, row, x, k], row = z H + y.  A workgroup owns TR rows x TA control points (one lane
// each, TR TA <= TPB, rows fastest) and walks the voxels of their supports in chunks of XC: the chunk's rows and its weight
// table go to LDS.
constexpr int BWD_XC = 512, BWD_G_VOX = 2048;      // voxels per chunk and row; voxels of all rows of a chunk
constexpr int STAGE_B = 8;                         // loads in flight per lane while staging

__global__ __launch_bounds__(TPB) void bspline_bwd_x_kernel(const float* __restrict__ dgrid, float* __restrict__ t1, long long rows,
                                                            int W, int Cx, int TR, int TA, int XC, int atiles, int vec4) {
  // LDS banks.  The lanes of a wave are TR rows x 64 / TR control points, rows fastest: the rows of one control point read the
  // same weight (a broadcast) and their own row of sG, whose pitch P is odd, so they fall on different banks; the weights are
  // four planes [j][x], so that neighbouring control points (one cell = W / (Cx - 3) voxels apart) are that many banks apart.
  // (Lanes along the control points of one row with [x][4] weights were 18 lanes to a bank: 250 us of LDS time at 256^3.)
  extern __shared__ __attribute__((aligned(16))) float sG[];      // [TR][P], then the tables
  const int P = (XC * 3) | 1;
  float* sW = sG + (size_t)TR * P;                                // [4][XC]
  int* sC = reinterpret_cast<int*>(sW + (size_t)XC * 4);          // [XC]
  const int n = blockIdx.y, tid = threadIdx.x;
  const unsigned bid = blockIdx.x;
  const int at = (int)(bid % (unsigned)atiles);
  const long long r0 = (long long)(bid / (unsigned)atiles) * TR;
  const int nr = rows - r0 < TR ? (int)(rows - r0) : TR;
  const int a0 = at * TA, na = Cx - a0 < TA ? Cx - a0 : TA, K = Cx - 3;
  const int ry = tid % TR, a = a0 + tid / TR;
  const bool active = ry < nr && a < a0 + na;
  const int xlo = lat_first((long long)a - 3, W, K), xhi = lat_first((long long)a + 1, W, K);
  const int xbeg = lat_first((long long)a0 - 3, W, K), xend = lat_first((long long)a0 + na, W, K);
  const float* dg = dgrid + ((long long)n * rows + r0) * W * 3;
  double acc[3] = {0.0, 0.0, 0.0};      // 0.3 VALU cycles per voxel more than float: hidden under the HBM read
  for (int X0 = xbeg; X0 < xend; X0 += XC) {
    const int xc = xend - X0 < XC ? xend - X0 : XC;
    __syncthreads();
    for (int i = tid; i < xc; i += TPB) {
      const LatW w = lat_w(X0 + i, W, Cx);
      sC[i] = w.cell;
      sW[i] = w.w[0]; sW[XC + i] = w.w[1]; sW[2 * XC + i] = w.w[2]; sW[3 * XC + i] = w.w[3];
    }
    // STAGE_B loads in flight per lane before the first goes to LDS (one at a time, the loop is a chain of HBM latencies:
    // measured 241 us of the 314 us backward at 256^3); 16-byte loads where rows, chunk and pointer allow
    const int seg = xc * 3;
    if (vec4 && (seg & 3) == 0 && ((X0 * 3) & 3) == 0) {
      const int seg4 = seg / 4, tot = nr * seg4;
      for (int base = 0; base < tot; base += TPB * STAGE_B) {
        float4 v[STAGE_B];
#pragma unroll
        for (int u = 0; u < STAGE_B; ++u) {
          const int idx = base + u * TPB + tid, r = idx / seg4, j = idx - r * seg4;
          if (idx < tot) v[u] = reinterpret_cast<const float4*>(dg + ((long long)r * W + X0) * 3)[j];
        }
#pragma unroll
        for (int u = 0; u < STAGE_B; ++u) {
          const int idx = base + u * TPB + tid, r = idx / seg4, j = idx - r * seg4;
          if (idx < tot) {
            float* d = sG + (size_t)r * P + 4 * j;
            d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
          }
        }
      }
    } else {
      const int tot = nr * seg;
      for (int base = 0; base < tot; base += TPB * STAGE_B) {
        float v[STAGE_B];
#pragma unroll
        for (int u = 0; u < STAGE_B; ++u) {
          const int idx = base + u * TPB + tid, r = idx / seg, j = idx - r * seg;
          if (idx < tot) v[u] = dg[((long long)r * W + X0) * 3 + j];
        }
#pragma unroll
        for (int u = 0; u < STAGE_B; ++u) {
          const int idx = base + u * TPB + tid, r = idx / seg, j = idx - r * seg;
          if (idx < tot) sG[(size_t)r * P + j] = v[u];
        }
      }
    }
    __syncthreads();
    if (active) {
      const int lo = (xlo > X0 ? xlo : X0) - X0, hi = (xhi < X0 + xc ? xhi : X0 + xc) - X0;
      const float* g = sG + (size_t)ry * P;
      for (int i = lo; i < hi; ++i) {
        const double w = (double)sW[((a - sC[i]) & 3) * XC + i];      // a - cell is 0 .. 3 inside the support
        acc[0] += w * (double)g[i * 3]; acc[1] += w * (double)g[i * 3 + 1]; acc[2] += w * (double)g[i * 3 + 2];
      }
    }
  }
  if (active) {
    float* o = t1 + (((long long)n * rows + r0 + ry) * Cx + a) * 3;
    o[0] = (float)acc[0]; o[1] = (float)acc[1]; o[2] = (float)acc[2];
  }
}

// ---- backward, passes y and z: one axis contracted -------------------------------------------------------------------------------
// in (O, S, I) -> out[o, c, j] = sum_s B(s -> c) in[o, s, j], ascending s, in double.  A workgroup owns one (o, c) and TPB
// consecutive j; the weights of the support go through LDS, TPB at a time.  PERMUTE (the last pass, I = plane x 3): written as
// (O, 3, C, plane), which is dctrl's layout.
template <bool PERMUTE>
__global__ __launch_bounds__(TPB) void bspline_bwd_axis_kernel(const float* __restrict__ in, float* __restrict__ out, int S, int C,
                                                               long long I, int jblocks) {
  __shared__ float sW[TPB];
  const int tid = threadIdx.x;
  const unsigned bid = blockIdx.x;
  const long long j = (long long)(bid % (unsigned)jblocks) * TPB + tid;
  const long long oc = (long long)(bid / (unsigned)jblocks) + (long long)blockIdx.y * (gridDim.x / (unsigned)jblocks);
  const int c = (int)(oc % C);
  const long long o = oc / C;
  const int lo = lat_first((long long)c - 3, S, C - 3), hi = lat_first((long long)c + 1, S, C - 3);
  const float* p = in + o * S * I + j;
  double acc = 0.0;
  for (int s0 = lo; s0 < hi; s0 += TPB) {
    const int cnt = hi - s0 < TPB ? hi - s0 : TPB;
    __syncthreads();
    if (tid < cnt) {
      const LatW w = lat_w(s0 + tid, S, C);
      sW[tid] = w.w[(c - w.cell) & 3];
    }
    __syncthreads();
    if (j < I) {
      int i = 0;
      for (; i + STAGE_B <= cnt; i += STAGE_B) {      // STAGE_B loads in flight, added in the same ascending order
        float v[STAGE_B];
#pragma unroll
        for (int u = 0; u < STAGE_B; ++u) v[u] = p[(long long)(s0 + i + u) * I];
#pragma unroll
        for (int u = 0; u < STAGE_B; ++u) acc += (double)sW[i + u] * (double)v[u];
      }
      for (; i < cnt; ++i) acc += (double)sW[i] * (double)p[(long long)(s0 + i) * I];
    }
  }
  if (j >= I) return;
  if (PERMUTE) {
    const long long sp = j / 3, plane = I / 3;
    const int k = (int)(j - sp * 3);
    out[((o * 3 + k) * C + c) * plane + sp] = (float)acc;
  } else {
    out[(o * C + c) * I + j] = (float)acc;
  }
}

// ---- bending ---------------------------------------------------------------------------------------------------------------------
// out[n] = sum over the three lattice axes of the mean of (q[i - 1] - 2 q[i] + q[i + 1])^2 over that axis' differenced tensor
// (3 channels x (C_axis - 2) x the other two sizes).  Doubles, a fixed order: up to BEND_BLOCKS workgroups per sample (their
// number depends on the lattice alone, so a batch equals its samples) leave one partial each, a second launch adds them in order.
// (One workgroup per sample walked the 35^3 x 3 lattice of a 256^3 volume in 640 us, a third of the optimisation step.)
constexpr int BEND_BLOCKS = 64, BEND_PER_BLOCK = 4096;
struct Lat3 { int C[3]; long long st[3]; double inv[3]; long long total; };

__device__ __forceinline__ Lat3 make_lat3(int Cz, int Cy, int Cx) {
  Lat3 L;
  L.C[0] = Cz; L.C[1] = Cy; L.C[2] = Cx;
  L.st[0] = (long long)Cy * Cx; L.st[1] = Cx; L.st[2] = 1;
  L.total = 3ll * Cz * Cy * Cx;
#pragma unroll
  for (int a = 0; a < 3; ++a) L.inv[a] = 1.0 / ((double)(L.total / L.C[a]) * (double)(L.C[a] - 2));
  return L;
}
__device__ __forceinline__ void lat3_index(const Lat3& L, long long e, int (&i)[3]) {
  i[2] = (int)(e % L.C[2]);
  const long long r = e / L.C[2];
  i[1] = (int)(r % L.C[1]);
  i[0] = (int)((r / L.C[1]) % L.C[0]);
}

__global__ __launch_bounds__(TPB) void bspline_bending_fwd_kernel(const float* __restrict__ q, double* __restrict__ partial,
                                                                  int Cz, int Cy, int Cx) {
  __shared__ double red[TPB / kWave];
  const Lat3 L = make_lat3(Cz, Cy, Cx);
  const float* p = q + (long long)blockIdx.y * L.total;
  double acc = 0.0;
  for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < L.total; e += (long long)gridDim.x * TPB) {
    int i[3];
    lat3_index(L, e, i);
    const double c = (double)p[e];
#pragma unroll
    for (int a = 0; a < 3; ++a)
      if (i[a] >= 1 && i[a] <= L.C[a] - 2) {
        const double d = (double)p[e - L.st[a]] - 2.0 * c + (double)p[e + L.st[a]];      // exact: the inputs are floats
        acc += d * d * L.inv[a];
      }
  }
  const double s = block_sum<double>(acc, red);
  if (threadIdx.x == 0) partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

__global__ void bspline_bending_final_kernel(const double* __restrict__ partial, int nb, float* __restrict__ out, int N) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += partial[(long long)n * nb + b];
  out[n] = (float)s;
}

// dq[e] = gout[n] sum_axis (2 / count) (d[i - 1] - 2 d[i] + d[i + 1]), d[j] = the second difference centred on j, 1 <= j <= C - 2
__global__ __launch_bounds__(TPB) void bspline_bending_bwd_kernel(const float* __restrict__ q, const float* __restrict__ gout,
                                                                  float* __restrict__ dq, int Cz, int Cy, int Cx) {
  const Lat3 L = make_lat3(Cz, Cy, Cx);
  const long long e = (long long)blockIdx.x * TPB + threadIdx.x;
  if (e >= L.total) return;
  const int n = blockIdx.y;
  const float* p = q + (long long)n * L.total;
  int i[3];
  lat3_index(L, e, i);
  double acc = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int C = L.C[a], c = i[a];
    const long long st = L.st[a];
    double s = 0.0;
    if (c >= 2) s += (double)p[e - 2 * st] - 2.0 * (double)p[e - st] + (double)p[e];
    if (c >= 1 && c <= C - 2) s -= 2.0 * ((double)p[e - st] - 2.0 * (double)p[e] + (double)p[e + st]);
    if (c <= C - 3) s += (double)p[e] - 2.0 * (double)p[e + st] + (double)p[e + 2 * st];
    acc += 2.0 * L.inv[a] * s;
  }
  dq[(long long)n * L.total + e] = (float)((double)gout[n] * acc);
}

static bool bspline_args_ok(int N, int D, int H, int W, int Cz, int Cy, int Cx) {
  return N >= 1 && N <= 65535 && D >= 1 && H >= 1 && W >= 1 && (long long)D * H * W < (1ll << 31) && Cz >= 4 && Cy >= 4 &&
         Cx >= 4 && (long long)Cz * Cy * Cx < (1ll << 31);
}

struct BwdPlan { long long rows; int TR, TA, XC, atiles; size_t lds, t1_bytes, t2_bytes; };
static BwdPlan bwd_plan(int N, int D, int H, int W, int Cy, int Cx) {
  BwdPlan p;
  p.rows = (long long)D * H;
  p.TA = Cx < TPB ? Cx : TPB;
  p.TR = TPB / p.TA;
  if (p.TR > p.rows) p.TR = (int)p.rows;
  p.XC = BWD_G_VOX / p.TR < BWD_XC ? BWD_G_VOX / p.TR : BWD_XC;
  if (p.XC > W) p.XC = W;
  p.atiles = ceil_div(Cx, p.TA);
  p.lds = ((size_t)p.TR * ((p.XC * 3) | 1) + (size_t)p.XC * 5) * sizeof(float);
  p.t1_bytes = ((size_t)N * p.rows * Cx * 3 * sizeof(float) + 255) & ~(size_t)255;
  p.t2_bytes = ((size_t)N * D * Cy * Cx * 3 * sizeof(float) + 255) & ~(size_t)255;
  return p;
}

}  // namespace

// out = base + spline (disp false) or the spline alone (disp true, mat unused): one launch plan for both
static int bspline_fwd_launch(bool disp, const float* ctrl, const float* mat, float* out, int N, int D, int H, int W, int Cz, int Cy,
                              int Cx, void* stream) {
  if (!bspline_args_ok(N, D, H, W, Cz, Cy, Cx) || !ctrl || !out) return -22;
  // the largest tile whose lattice rows x columns fit the LDS budget (a one-voxel tile touches 4 x 4: always fits)
  int TX = W < FWD_TX ? W : FWD_TX, TY = H < FWD_TY ? H : FWD_TY;
  while (lat_span(TY, H, Cy) * lat_span(TX, W, Cx) * 3 > FWD_Q_FLOATS) {
    if (TY > 1) TY = (TY + 1) / 2;
    else TX = (TX + 1) / 2;
  }
  const int tiles_x = ceil_div(W, TX), tiles_y = ceil_div(H, TY);
  const long long blocks = (long long)tiles_x * tiles_y * D;      // <= the number of voxels < 2^31
  const size_t lds = (size_t)(lat_span(TY, H, Cy) * lat_span(TX, W, Cx) * 3) * sizeof(float);
  const dim3 g((unsigned)blocks, (unsigned)N);
  if (disp)
    bspline_fwd_kernel<true><<<g, TPB, lds, (hipStream_t)stream>>>(ctrl, mat, out, D, H, W, Cz, Cy, Cx, TY, TX, tiles_y, tiles_x);
  else
    bspline_fwd_kernel<false><<<g, TPB, lds, (hipStream_t)stream>>>(ctrl, mat, out, D, H, W, Cz, Cy, Cx, TY, TX, tiles_y, tiles_x);
  return KMH_LAUNCH_CHECK();
}

KMH_API int kmh_bspline_grid_fwd(const float* ctrl, const float* mat, float* out, int N, int D, int H, int W, int Cz, int Cy,
                                 int Cx, void* stream) {
  return bspline_fwd_launch(false, ctrl, mat, out, N, D, H, W, Cz, Cy, Cx, stream);
}

/* The spline alone, out (N, D, H, W, 3) = sum B ctrl: kmh_bspline_grid_fwd without its base (a displacement that is a small
   fraction of a voxel keeps all its bits); kmh_bspline_grid_bwd is the transpose of both. */
KMH_API int kmh_bspline_disp_fwd(const float* ctrl, float* out, int N, int D, int H, int W, int Cz, int Cy, int Cx, void* stream) {
  return bspline_fwd_launch(true, ctrl, nullptr, out, N, D, H, W, Cz, Cy, Cx, stream);
}

/* Workspace of kmh_bspline_grid_bwd: the x-contracted (N, D, H, Cx, 3) and the y-contracted (N, D, Cy, Cx, 3) intermediates. */
KMH_API size_t kmh_bspline_grid_ws_bytes(int N, int D, int H, int W, int Cz, int Cy, int Cx) {
  if (!bspline_args_ok(N, D, H, W, Cz, Cy, Cx)) return 0;
  const BwdPlan p = bwd_plan(N, D, H, W, Cy, Cx);
  return p.t1_bytes + p.t2_bytes;
}

KMH_API int kmh_bspline_grid_bwd(const float* dgrid, float* dctrl, int N, int D, int H, int W, int Cz, int Cy, int Cx, void* ws,
                                 void* stream) {
  if (!bspline_args_ok(N, D, H, W, Cz, Cy, Cx) || !dgrid || !dctrl || !ws) return -22;
  const BwdPlan p = bwd_plan(N, D, H, W, Cy, Cx);
  hipStream_t s = (hipStream_t)stream;
  float* t1 = (float*)ws;
  float* t2 = (float*)((char*)ws + p.t1_bytes);
  const long long xblocks = (long long)ceil_div(p.rows, p.TR) * p.atiles;
  const long long Iy = (long long)Cx * 3, Iz = (long long)Cy * Cx * 3;
  const int jby = ceil_div(Iy, TPB), jbz = ceil_div(Iz, TPB);
  const long long yblocks = (long long)D * Cy * jby, zblocks = (long long)Cz * jbz;      // per sample
  if (xblocks >= (1ll << 31) || yblocks >= (1ll << 31) || zblocks >= (1ll << 31)) return -22;
  // 16-byte loads while staging: every row starts on a 16-byte boundary (W 3 floats a multiple of 4)
  const int vec4 = ((size_t)dgrid & 15) == 0 && (W * 3ll) % 4 == 0;
  bspline_bwd_x_kernel<<<dim3((unsigned)xblocks, (unsigned)N), TPB, p.lds, s>>>(dgrid, t1, p.rows, W, Cx, p.TR, p.TA, p.XC,
                                                                               p.atiles, vec4);
  bspline_bwd_axis_kernel<false><<<dim3((unsigned)yblocks, (unsigned)N), TPB, 0, s>>>(t1, t2, H, Cy, Iy, jby);
  bspline_bwd_axis_kernel<true><<<dim3((unsigned)zblocks, (unsigned)N), TPB, 0, s>>>(t2, dctrl, D, Cz, Iz, jbz);
  return KMH_LAUNCH_CHECK();
}

/* ws: kmh_bspline_bending_ws_bytes(N) bytes, the per-workgroup partial sums. */
KMH_API size_t kmh_bspline_bending_ws_bytes(int N) { return N < 1 ? 0 : (size_t)N * BEND_BLOCKS * sizeof(double); }

KMH_API int kmh_bspline_bending_fwd(const float* q, float* out, int N, int Cz, int Cy, int Cx, void* ws, void* stream) {
  if (!bspline_args_ok(N, 1, 1, 1, Cz, Cy, Cx) || !q || !out || !ws) return -22;
  int nb = ceil_div(3ll * Cz * Cy * Cx, BEND_PER_BLOCK);
  if (nb > BEND_BLOCKS) nb = BEND_BLOCKS;
  hipStream_t s = (hipStream_t)stream;
  bspline_bending_fwd_kernel<<<dim3(nb, N), TPB, 0, s>>>(q, (double*)ws, Cz, Cy, Cx);
  bspline_bending_final_kernel<<<ceil_div(N, 64), 64, 0, s>>>((const double*)ws, nb, out, N);
  return KMH_LAUNCH_CHECK();
}

KMH_API int kmh_bspline_bending_bwd(const float* q, const float* gout, float* dq, int N, int Cz, int Cy, int Cx, void* stream) {
  if (!bspline_args_ok(N, 1, 1, 1, Cz, Cy, Cx) || !q || !gout || !dq) return -22;
  const long long blocks = (3ll * Cz * Cy * Cx + TPB - 1) / TPB;
  bspline_bending_bwd_kernel<<<dim3((unsigned)blocks, (unsigned)N), TPB, 0, (hipStream_t)stream>>>(q, gout, dq, Cz, Cy, Cx);
  return KMH_LAUNCH_CHECK();
}
