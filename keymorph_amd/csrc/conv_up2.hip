// The fused decoder operator ("up2") of the split-operand 3x3x3 convolution (the arithmetic: conv_bf.hip, common.h).
// Kernels in this file:
//   conv3_up2_fwd_kernel<TERMS, AMP>      forward over the low-resolution tensor, 8 pre-summed taps per output parity
//   conv3_up2_dgrad_kernel<TERMS, AMP>    data gradient at LOW resolution, 64 pre-summed taps
//   up2_wgrad_gemm_kernel<TERMS, AMP>     weight gradient as a GEMM over box sums of dz; up2_wgrad_reduce_kernel
//   up2_wgrad_fold_kernel<AMP, MODE>      the same without the box-sum tensor
//   pack_weight_up_kernel<TERMS>, pack_weight_upt_kernel<TERMS>
//
// 3x3x3 convolution over a NEAREST-UPSAMPLED (x2) tensor without the upsampled tensor: the decoder's first convolution
// reads cat(skip, up2(low)); for the `low` channels the 27 taps of an output voxel of parity p = (pz, py, px) fall on
// only 2 x 2 x 2 low-resolution voxels (per axis: parity 0 -> offsets {-1: tap -1; 0: taps 0, +1}, parity 1 ->
// {0: taps -1, 0; +1: tap +1}), so with the taps of one low voxel summed beforehand (pack_weight_up_kernel) every
// output costs 8 multiply-adds per channel instead of 27.  Zero padding is consistent: padded positions -1 / 2L map to
// the low voxels -1 / L, which are outside too.  The kernel writes the low channels' contribution (descaled, no bias
// / ReLU); kmh_conv3d_fwd_bf over the skip channels then adds it in its epilogue (`addend`).
// Workgroup = 32 x 4 x 1 low voxels (-> 64 x 8 x 2 outputs), 8 waves: wave = ((pz, py), 32-cout tile) and holds both
// px parities of 4 rows (8 accumulator tiles); K = 16 = (low tap jx = lane half) x 8 channels; 4 tap pairs per parity.
// Chunks are double-buffered in LDS: the loads of chunk c+1 are in flight during the MFMAs of chunk c.
#include <cstdlib>
#include "conv_split.h"
#include "stats_final.h"

namespace {

constexpr int UX = 32, UY = 4;
constexpr int UHX = UX + 2, UHY = UY + 2, UPL = UHX * UHY * 3;      // 612 halo voxels of the low tensor
constexpr int UP_TPB = 512;
constexpr int UP_NST = 32;                                          // 8 parities x 4 tap pairs

template <int TERMS>
__global__ __launch_bounds__(256) void pack_weight_up_kernel(const float* __restrict__ w, __bf16* __restrict__ out,
                                                             int Cout, int Ctot, int cofs, int Cl, int CoutP, int nchunk,
                                                             const float* __restrict__ wscale) {
  const long long total = (long long)nchunk * UP_NST * 2 * CoutP * 8;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int c = (int)(e & 7);
    long long r = e >> 3;
    const int col = (int)(r % CoutP); r /= CoutP;
    const int h = (int)(r & 1); r >>= 1;
    const int su = (int)(r % UP_NST);
    const int chunk = (int)(r / UP_NST);
    const int ci = chunk * 8 + c, p = su >> 2, st = su & 3;
    const int par[3] = {p >> 2, (p >> 1) & 1, p & 1}, j[3] = {st >> 1, st & 1, h};
    int lo[3], hi[3];                                   // tap range (0..2) of each axis that lands on low offset j
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = par[a] == 0 ? (j[a] == 0 ? 0 : 1) : (j[a] == 0 ? 0 : 2);
      hi[a] = par[a] == 0 ? (j[a] == 0 ? 0 : 2) : (j[a] == 0 ? 1 : 2);
    }
    float v = 0.f;
    if (ci < Cl && col < Cout) {
      const float* wr = w + ((long long)col * Ctot + cofs + ci) * 27;
      for (int kz = lo[0]; kz <= hi[0]; ++kz)
        for (int ky = lo[1]; ky <= hi[1]; ++ky)
          for (int kx = lo[2]; kx <= hi[2]; ++kx) v += wr[kz * 9 + ky * 3 + kx];
    }
    float rem = wscale ? v * wscale[0] : v;
#pragma unroll
    for (int t = 0; t < TERMS; ++t) {
      float back;
      const unsigned short hb = to16<TERMS>(rem, back);
      reinterpret_cast<unsigned short*>(out)[((((long long)chunk * TERMS + t) * UP_NST + su) * 2 + h) * CoutP * 8 +
                                             (long long)col * 8 + c] = hb;
      rem -= back;
    }
  }
}

template <int TERMS, bool AMP = false>
__global__ __launch_bounds__(UP_TPB, 2) void conv3_up2_fwd_kernel(
    const float* __restrict__ xl, const float* __restrict__ scale, const float* __restrict__ shift, int Ctot, int cofs,
    const bf16x8* __restrict__ wp, float* __restrict__ y, int Dl, int Hl, int Wl, int Cl, int Cout, int CoutP,
    int tiles_x, int tiles_y, const float* __restrict__ ascale, const float* __restrict__ wscale) {
  __shared__ bf16x8 sIn[2][TERMS][UPL];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int n = blockIdx.z;
  const int ncog = (Cout + 63) / 64;
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  const int cog = item % ncog, brick = item / ncog;
  const int bx = brick % tiles_x, by = (brick / tiles_x) % tiles_y, zl = brick / (tiles_x * tiles_y);
  const int x0 = bx * UX, y0 = by * UY;
  const int pz = (wv >> 1) & 1, py = wv & 1, nt = wv >> 2;
  const int co = cog * 64 + 32 * nt + li;

  f32x16 acc[2][UY];
#pragma unroll
  for (int pl = 0; pl < 2; ++pl)
#pragma unroll
    for (int m = 0; m < UY; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[pl][m][r] = 0.f;
  const float sA = ascale ? ascale[0] : 1.f;
  const float desc = (ascale ? ascale[1] : 1.f) * (wscale ? wscale[1] : 1.f);
  const int nchunk = Cl / KC;

  // staging descriptors: up to 2 halo voxels per thread, the same for every chunk
  constexpr int NV = (UPL + UP_TPB - 1) / UP_TPB;      // 2
  int sv_rel[NV];
  bool sv_in[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = tid + i * UP_TPB;
    const int lx = v % UHX, ly = (v / UHX) % UHY, lz = v / (UHX * UHY);
    const int gx = x0 + lx - 1, gy = y0 + ly - 1, gz = zl + lz - 1;
    sv_in[i] = (v < UPL) && ((unsigned)gx < (unsigned)Wl) && ((unsigned)gy < (unsigned)Hl) && ((unsigned)gz < (unsigned)Dl);
    sv_rel[i] = sv_in[i] ? ((gz * Hl + gy) * Wl + gx) * Cl : 0;
  }
  const float* xn = xl + (long long)n * Dl * Hl * Wl * Cl;
  float pv[NV][8];
  auto fetch = [&](int ch) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const float* p = xn + sv_rel[i] + ch * KC;       // a valid address also for padding voxels (zeroed at commit)
      const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
      pv[i][0] = a.x; pv[i][1] = a.y; pv[i][2] = a.z; pv[i][3] = a.w;
      pv[i][4] = b.x; pv[i][5] = b.y; pv[i][6] = b.z; pv[i][7] = b.w;
    }
  };
  auto commit = [&](int ch, int stage) {
    float csc[8], csh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      csc[j] = (scale ? scale[(long long)n * Ctot + cofs + ch * KC + j] : 1.f) * sA;
      csh[j] = (scale ? shift[(long long)n * Ctot + cofs + ch * KC + j] : 0.f) * sA;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = tid + i * UP_TPB;
      if (v < UPL) {
        float val[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) val[j] = sv_in[i] ? pv[i][j] * csc[j] + csh[j] : 0.f;   // zero padding AFTER the norm
        bf16x8 parts[TERMS];
        split8<TERMS>(val, parts);
#pragma unroll
        for (int t = 0; t < TERMS; ++t) sIn[stage][t][v] = parts[t];
      }
    }
  };

  const int wbase = (pz * UHY + py) * UHX + li + lh;   // + (jz * UHY + jy + m) * UHX + px: this lane's A voxel
  const int subase = (pz * 4 + py * 2) * 4;            // first step of parity (pz, py, 0)
  fetch(0);
  commit(0, 0);
  __syncthreads();
  for (int ch = 0; ch < nchunk; ++ch) {
    const int stage = ch & 1;
    if (ch + 1 < nchunk) fetch(ch + 1);
    const bf16x8* wc = wp + (long long)ch * TERMS * UP_NST * 2 * CoutP + lh * CoutP + co;
    constexpr int BD = 4;                               // B ring depth over the wave's 8 (px, tap pair) steps
    bf16x8 bq[BD][TERMS];
#pragma unroll
    for (int d = 0; d < BD; ++d)
#pragma unroll
      for (int q = 0; q < TERMS; ++q)
        bq[d][q] = wc[((long long)(q * UP_NST + subase + d)) * 2 * CoutP];
#pragma unroll
    for (int k = 0; k < 8; ++k) {                       // k = px * 4 + tap pair
      const int pl = k >> 2, st = k & 3;
      bf16x8 b[TERMS];
#pragma unroll
      for (int q = 0; q < TERMS; ++q) b[q] = bq[k % BD][q];
      if (k + BD < 8) {
#pragma unroll
        for (int q = 0; q < TERMS; ++q)
          bq[k % BD][q] = wc[((long long)(q * UP_NST + subase + k + BD)) * 2 * CoutP];
      }
      const int off = wbase + ((st >> 1) * UHY + (st & 1)) * UHX + pl;
#pragma unroll
      for (int m = 0; m < UY; ++m) {
        bf16x8 a[TERMS];
#pragma unroll
        for (int q = 0; q < TERMS; ++q) a[q] = sIn[stage][q][off + m * UHX];
        if (TERMS == 3) {
          acc[pl][m] = mfma16<TERMS>(a[2], b[0], acc[pl][m]);
          acc[pl][m] = mfma16<TERMS>(a[1], b[1], acc[pl][m]);
          acc[pl][m] = mfma16<TERMS>(a[0], b[2], acc[pl][m]);
        }
        if constexpr (!AMP) {
          acc[pl][m] = mfma16<TERMS>(a[1], b[0], acc[pl][m]);
          acc[pl][m] = mfma16<TERMS>(a[0], b[1], acc[pl][m]);
        }
        acc[pl][m] = mfma16<TERMS>(a[0], b[0], acc[pl][m]);
      }
    }
    if (ch + 1 < nchunk) commit(ch + 1, stage ^ 1);    // the other stage: its readers finished a chunk ago
    __syncthreads();
  }
  // epilogue: one channel per lane in the accumulators -> 16 bytes per lane after a per-wave transposition through the
  // (now idle) fragment images: 32 store instructions per lane instead of 128 (the store path is issue-bound, see
  // conv3_fwd_g_kernel).  Cout % 4 == 0 is guaranteed by the caller (upcat_conv_ok: channels % 8 == 0).
  const int D = 2 * Dl, H = 2 * Hl, W = 2 * Wl;
  const int gz = 2 * zl + pz;
  float* tile = reinterpret_cast<float*>(&sIn[0][0][0]) + wv * (32 * 32);
  const int c4 = lane & 7, vx = lane >> 3;
  const int cq = cog * 64 + 32 * nt + 4 * c4;
  const bool cq_ok = cq < Cout;
#pragma unroll
  for (int pl = 0; pl < 2; ++pl)
#pragma unroll
    for (int m = 0; m < UY; ++m) {
#pragma unroll
      for (int r = 0; r < 16; ++r) tile[((r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + li] = acc[pl][m][r] * desc;
      const bool row_ok = cq_ok && y0 + m < Hl;
      const int gy = 2 * (y0 + m) + py;
      float* yp = y + ((((long long)n * D + gz) * H + gy) * W) * Cout + cq;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int xx = vx + 8 * k, xlw = x0 + xx;
        const float4 v = *reinterpret_cast<const float4*>(tile + xx * 32 + 4 * c4);
        if (row_ok && xlw < Wl) *reinterpret_cast<float4*>(yp + (long long)(2 * xlw + pl) * Cout) = v;
      }
    }
}

// ---- data gradient of the same operator: ds[m][ci] = sum over the 4 x 4 x 4 high-resolution positions u = 2m + t,
// t in {-1, 0, 1, 2} per axis, of Wt[t][co][ci] dz[u][co] -- the sum over a low voxel's 8 children of the gradient with
// respect to the upsampled tensor, computed at LOW resolution with 64 (pre-summed) taps instead of 8 x 27.  Per axis
// t <-> (output parity p, low offset index j) of the forward: -1 <-> (1, 1), 0 <-> (0, 1), 1 <-> (1, 0), 2 <-> (0, 0).
// Workgroup = 16 x 4 x 1 low voxels; LDS = the 34 x 10 x 4 high-resolution halo of dz (8 channels, hi + lo);
// wave = 32-channel tile of ci; K = 16 = (x tap pair) x 8 dz channels; 32 steps per chunk.
constexpr int DUX = 16, DUY = 4;                                           // low brick of the data gradient: 16 x 4 x 1
constexpr int DHX = 2 * DUX + 2, DHY = 2 * DUY + 2, DPL = DHX * DHY * 4;   // 34 x 10 x 4 = 1360 halo voxels of dz
constexpr int DUP_NST = 32;                                                // (tz, ty) x (x tap pair)
constexpr int DUP_TPB = 256;                                               // 4 waves = the 4 channel tiles of 128 ci

template <int TERMS>
__global__ __launch_bounds__(256) void pack_weight_upt_kernel(const float* __restrict__ w, __bf16* __restrict__ out,
                                                              int Cout, int Ctot, int cofs, int Cl, int CiP, int nchunk,
                                                              const float* __restrict__ wscale) {
  const long long total = (long long)nchunk * DUP_NST * 2 * CiP * 8;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int c = (int)(e & 7);                        // dz channel inside the chunk
    long long r = e >> 3;
    const int col = (int)(r % CiP); r /= CiP;          // input (low) channel
    const int h = (int)(r & 1); r >>= 1;
    const int s = (int)(r % DUP_NST);
    const int chunk = (int)(r / DUP_NST);
    const int co = chunk * 8 + c;
    const int idx[3] = {s >> 3, (s >> 1) & 3, 2 * (s & 1) + h};     // t + 1 per axis (z, y, x)
    int lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int par = (idx[a] + 1) & 1, j = idx[a] <= 1 ? 1 : 0;
      lo[a] = par == 0 ? (j == 0 ? 0 : 1) : (j == 0 ? 0 : 2);
      hi[a] = par == 0 ? (j == 0 ? 0 : 2) : (j == 0 ? 1 : 2);
    }
    float v = 0.f;
    if (co < Cout && col < Cl) {
      const float* wr = w + ((long long)co * Ctot + cofs + col) * 27;
      for (int kz = lo[0]; kz <= hi[0]; ++kz)
        for (int ky = lo[1]; ky <= hi[1]; ++ky)
          for (int kx = lo[2]; kx <= hi[2]; ++kx) v += wr[kz * 9 + ky * 3 + kx];
    }
    float rem = wscale ? v * wscale[0] : v;
#pragma unroll
    for (int t = 0; t < TERMS; ++t) {
      float back;
      const unsigned short hb = to16<TERMS>(rem, back);
      reinterpret_cast<unsigned short*>(out)[((((long long)chunk * TERMS + t) * DUP_NST + s) * 2 + h) * CiP * 8 +
                                             (long long)col * 8 + c] = hb;
      rem -= back;
    }
  }
}

template <int TERMS, bool AMP = false>
__global__ __launch_bounds__(DUP_TPB, TERMS == 2 ? 2 : 3) void conv3_up2_dgrad_kernel(
    const float* __restrict__ dz /* (N,2Dl,2Hl,2Wl,Cout) */, const bf16x8* __restrict__ wp,
    float* __restrict__ ds /* (N,Dl,Hl,Wl,Cl) */, int Dl, int Hl, int Wl, int Cl, int CiP, int Cout, int tiles_x,
    int tiles_y, const float* __restrict__ dscale, const float* __restrict__ wscale,
    double* __restrict__ stats_partial /* (N, bricks, Cl, 2) | NULL: per-brick (sum ds, sum ds^2) of every channel */,
    int in_blocked /* dz is channel-blocked (N, Cout/8, 2Dl, 2Hl, 2Wl, 8): a chunk's 32 bytes per voxel are contiguous ACROSS
                      voxels, whole lines per request instead of 32-byte pieces of 64-byte sectors */) {
  // Workgroup = 16 x 4 x 1 low voxels = two M tiles of (16 x, 2 y); wave = one 32-channel tile of ci, both M tiles.
  // 43.5 KB of LDS; two (f16x3, prefetching: 224 registers) or three (bf16x6) workgroups per CU, whose staging and MFMA
  // phases overlap.
  __shared__ bf16x8 sIn[TERMS][DPL];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int n = blockIdx.z;
  const int ncig = (Cl + 127) / 128;
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  const int cig = item % ncig, brick = item / ncig;
  const int bx = brick % tiles_x, by = (brick / tiles_x) % tiles_y, zl = brick / (tiles_x * tiles_y);
  const int x0 = bx * DUX, y0 = by * DUY;
  const int ci = cig * 128 + 32 * wv + li;
  const int D = 2 * Dl, H = 2 * Hl, W = 2 * Wl;

  f32x16 acc[2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
  const float sD = dscale ? dscale[0] : 1.f;
  const float desc = (dscale ? dscale[1] : 1.f) * (wscale ? wscale[1] : 1.f);
  const int nchunk = (Cout + KC - 1) / KC;
  const float* dn = dz + (long long)n * D * H * W * Cout;
  constexpr int NV = (DPL + DUP_TPB - 1) / DUP_TPB;    // 6
  // row li of an M tile = low voxel (x = li & 15, y = 2 mt + (li >> 4)); its halo origin is (2 y, 2 x)
  const int abase = (2 * (li >> 4)) * DHX + 2 * (li & 15) + lh;

  // the next chunk's halo is fetched into registers under this chunk's MFMAs (staging it at the top of its own chunk left
  // an HBM round trip exposed per chunk and workgroup)
  float4 pre[NV][2];
  auto fetch = [&](int ch) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = tid + i * DUP_TPB;
      pre[i][0] = pre[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (v < DPL) {
        const int lx = v % DHX, ly = (v / DHX) % DHY, lz = v / (DHX * DHY);
        const int gx = 2 * x0 - 1 + lx, gy = 2 * y0 - 1 + ly, gz = 2 * zl - 1 + lz;
        if ((unsigned)gx < (unsigned)W && (unsigned)gy < (unsigned)H && (unsigned)gz < (unsigned)D) {
          const long long vox = ((long long)gz * H + gy) * W + gx;
          const float* p = in_blocked ? dn + ((long long)ch * D * H * W + vox) * KC : dn + vox * Cout + ch * KC;
          if ((Cout & 3) == 0) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
              if (ch * KC + 4 * q < Cout) pre[i][q] = *reinterpret_cast<const float4*>(p + 4 * q);
          } else {
            float t8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (ch * KC + j < Cout) t8[j] = p[j];
            pre[i][0] = make_float4(t8[0], t8[1], t8[2], t8[3]);
            pre[i][1] = make_float4(t8[4], t8[5], t8[6], t8[7]);
          }
        }
      }
    }
  };
  constexpr bool PF = TERMS == 2;                       // (the three-term variant has no registers to spare: it fetches in place)
  if (PF) fetch(0);
  for (int ch = 0; ch < nchunk; ++ch) {
    __syncthreads();                                    // the previous chunk's readers are done
    if (!PF) fetch(ch);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = tid + i * DUP_TPB;
      if (v < DPL) {
        const float val[8] = {pre[i][0].x * sD, pre[i][0].y * sD, pre[i][0].z * sD, pre[i][0].w * sD,
                              pre[i][1].x * sD, pre[i][1].y * sD, pre[i][1].z * sD, pre[i][1].w * sD};
        bf16x8 parts[TERMS];
        split8<TERMS>(val, parts);
#pragma unroll
        for (int t = 0; t < TERMS; ++t) sIn[t][v] = parts[t];
      }
    }
    __syncthreads();
    if (PF && ch + 1 < nchunk) fetch(ch + 1);
    const bf16x8* wc = wp + (long long)ch * TERMS * DUP_NST * 2 * CiP + lh * CiP + ci;
    constexpr int BD = 4;
    bf16x8 bq[BD][TERMS];
#pragma unroll
    for (int d = 0; d < BD; ++d)
#pragma unroll
      for (int q = 0; q < TERMS; ++q) bq[d][q] = wc[((long long)(q * DUP_NST + d)) * 2 * CiP];
#pragma unroll 1
    for (int tz = 0; tz < 4; ++tz) {                    // 8 steps per z tap: the ring (depth 4) index stays constant
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) {
        const int s = tz * 8 + s8;
        bf16x8 b[TERMS];
#pragma unroll
        for (int q = 0; q < TERMS; ++q) b[q] = bq[s8 % BD][q];
        if (s + BD < DUP_NST) {
#pragma unroll
          for (int q = 0; q < TERMS; ++q) bq[s8 % BD][q] = wc[((long long)(q * DUP_NST + s + BD)) * 2 * CiP];
        }
        const int off = abase + (tz * DHY + (s8 >> 1)) * DHX + 2 * (s8 & 1);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          bf16x8 a[TERMS];
#pragma unroll
          for (int q = 0; q < TERMS; ++q) a[q] = sIn[q][off + 4 * m * DHX];
          if (TERMS == 3) {
            acc[m] = mfma16<TERMS>(a[2], b[0], acc[m]);
            acc[m] = mfma16<TERMS>(a[1], b[1], acc[m]);
            acc[m] = mfma16<TERMS>(a[0], b[2], acc[m]);
          }
          if constexpr (!AMP) {
            acc[m] = mfma16<TERMS>(a[1], b[0], acc[m]);
            acc[m] = mfma16<TERMS>(a[0], b[1], acc[m]);
          }
          acc[m] = mfma16<TERMS>(a[0], b[0], acc[m]);
        }
      }
    }
  }
  if (ci >= Cl) return;
  float s1 = 0.f, s2 = 0.f;                             // <= 32 values per lane: fp32, then fp64 per brick
#pragma unroll
  for (int m = 0; m < 2; ++m) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;  // row of the M tile
      const int gx = x0 + (row & 15), gy = y0 + 2 * m + (row >> 4);
      if (gx < Wl && gy < Hl) {
        const float v = acc[m][r] * desc;
        ds[((((long long)n * Dl + zl) * Hl + gy) * Wl + gx) * Cl + ci] = v;
        s1 += v;
        s2 = fmaf(v, v, s2);
      }
    }
  }
  if (stats_partial) {                                  // the consumer's GroupNorm backward wants sum ds per channel
    double d1 = (double)s1, d2 = (double)s2;
    d1 += __shfl_xor(d1, 32, 64);
    d2 += __shfl_xor(d2, 32, 64);
    if (lh == 0) {
      double* o = stats_partial + (((long long)n * gridDim.x / ncig + brick) * Cl + ci) * 2;
      o[0] = d1; o[1] = d2;
    }
  }
}

// ---- weight gradient of the same operator: C_n (Cl x J) = A_n^T B_n over the low-resolution voxels, A = the normalised
// low tensor (V x Cl), B = the box sums of dz (V x J, J = 27 Cout, norm.hip: up2_boxsum_kernel).  Both operands have the
// reduction index slowest, so both are transposed while they are staged (voxel pairs packed into 32-bit LDS words, like
// the 27-tap weight gradient's images).  Workgroup = 128 x 128 tile of C over one K slab, 32 voxels per step; wave = 64 x 64.
// Bound: a CU streams in ~10 B / cycle (256 CUs: 5.1 TB/s), this tile loads (128 + 128) x 4 B per 2 x 128 x 128 multiply-adds.  A
// 128 x 256 tile on 8 waves (1.33x the intensity) needs 176 registers = ONE workgroup per CU and is no faster (2.97 vs 2.86 ms).
constexpr int GK = 32;                        // voxels per staging step (64: two workgroups per CU, 5 % slower)
constexpr int GPITCH = GK * 2 + 16;           // bytes per LDS row (32 x 2 B + pad: 5 x 16 B, conflict-free b128 reads)
template <int TERMS, bool AMP = false>
__global__ __launch_bounds__(256, 3) void up2_wgrad_gemm_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                                float* __restrict__ Cp, int V, int Cl, int J, int kslab,
                                                                int ntn, int ntm, const float* __restrict__ ascale,
                                                                const float* __restrict__ bscale,
                                                                const float* __restrict__ a_scale /* (N, Cl) | NULL */,
                                                                const float* __restrict__ a_shift, int xcd) {
  __shared__ __attribute__((aligned(16))) unsigned char sA[TERMS][128 * GPITCH];
  __shared__ __attribute__((aligned(16))) unsigned char sB[TERMS][128 * GPITCH];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int n = blockIdx.z;
  // The column tiles of one (row tile, K slab) read the SAME rows of A.  Dealt round-robin over the XCDs, every XCD's L2 fetched
  // them for itself: 14.75 GB per launch for 7.25 GB of G at 64^3 x 128 x 1728 (PMC), and the launch ran at the HBM rate of THAT.
  // With one contiguous item range per XCD (xcd_remap) the tiles of a slab sit on one XCD and walk the slab together: A comes
  // from HBM once.  (xcd == 0: the round-robin order; the host always passes 1.)
  int item = xcd ? xcd_remap((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
  const int tn = item % ntn; item /= ntn;
  const int tm = item % ntm;
  const int slab = item / ntm;
  const int m0 = tm * 128, n0 = tn * 128;
  const int wm = wv & 1, wn = wv >> 1;
  const float sa = ascale ? ascale[0] : 1.f, sb = bscale ? bscale[0] : 1.f;
  const float desc = (ascale ? ascale[1] : 1.f) * (bscale ? bscale[1] : 1.f);
  const float* An = A + (long long)n * V * Cl;
  const float* Bn = B + (long long)n * V * J;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int k_beg = slab * kslab;
  int k_end = k_beg + kslab;
  if (k_end > V) k_end = V;
  // staging items: (voxel pair kp, column quad cq) -> 2 float4 loads, 4 packed words per term.  Eight consecutive lanes take the
  // eight quads of ONE 128-byte line of a voxel row (round 4; four lanes / 64-byte pieces before: 2.9 TB/s -> see DESIGN.md)
  constexpr int NKP = GK / 2, NIT = GK / 16;   // voxel pairs per step, staging items per thread
  float4 pa[NIT][2], pb[NIT][2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int e = tid + i * 256, cq = (e & 7) + 8 * (e / (8 * NKP)), kp = (e >> 3) & (NKP - 1);   // lanes: 8 quads (one line) x 8 voxel pairs
      const int k = k0 + 2 * kp;
      const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
      const int ca = m0 + 4 * cq, cb = n0 + 4 * cq;
      pa[i][0] = (k < k_end && ca < Cl) ? *reinterpret_cast<const float4*>(An + (long long)k * Cl + ca) : z4;
      pa[i][1] = (k + 1 < k_end && ca < Cl) ? *reinterpret_cast<const float4*>(An + (long long)(k + 1) * Cl + ca) : z4;
      pb[i][0] = (k < k_end && cb < J) ? *reinterpret_cast<const float4*>(Bn + (long long)k * J + cb) : z4;
      pb[i][1] = (k + 1 < k_end && cb < J) ? *reinterpret_cast<const float4*>(Bn + (long long)(k + 1) * J + cb) : z4;
    }
  };
  // GroupNorm's per-(sample, channel) affine of the A operand, applied while it is staged (a_scale != NULL): the caller
  // hands over the RAW low tensor and no normalised copy of it is written and read back
  float4 csc[NIT], csh[NIT];
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int e = tid + i * 256, cq = (e & 7) + 8 * (e / (8 * NKP)), ca = m0 + 4 * cq;
    csc[i] = make_float4(1.f, 1.f, 1.f, 1.f);
    csh[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a_scale && ca < Cl) {
      csc[i] = *reinterpret_cast<const float4*>(a_scale + (long long)n * Cl + ca);
      csh[i] = *reinterpret_cast<const float4*>(a_shift + (long long)n * Cl + ca);
    }
  }
  auto commit = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int e = tid + i * 256, cq = (e & 7) + 8 * (e / (8 * NKP)), kp = (e >> 3) & (NKP - 1);   // (2-way LDS write conflicts at most)
      const bool v0 = k0 + 2 * kp < k_end, v1 = k0 + 2 * kp + 1 < k_end;     // rows past the slab stay zero (no shift)
      const float a0[4] = {v0 ? fmaf(pa[i][0].x, csc[i].x, csh[i].x) : 0.f, v0 ? fmaf(pa[i][0].y, csc[i].y, csh[i].y) : 0.f,
                           v0 ? fmaf(pa[i][0].z, csc[i].z, csh[i].z) : 0.f, v0 ? fmaf(pa[i][0].w, csc[i].w, csh[i].w) : 0.f};
      const float a1[4] = {v1 ? fmaf(pa[i][1].x, csc[i].x, csh[i].x) : 0.f, v1 ? fmaf(pa[i][1].y, csc[i].y, csh[i].y) : 0.f,
                           v1 ? fmaf(pa[i][1].z, csc[i].z, csh[i].z) : 0.f, v1 ? fmaf(pa[i][1].w, csc[i].w, csh[i].w) : 0.f};
      const float b0[4] = {pb[i][0].x, pb[i][0].y, pb[i][0].z, pb[i][0].w}, b1[4] = {pb[i][1].x, pb[i][1].y, pb[i][1].z, pb[i][1].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned w[TERMS];
        split_pair<TERMS>(a0[j] * sa, a1[j] * sa, w);
#pragma unroll
        for (int t = 0; t < TERMS; ++t) *reinterpret_cast<unsigned*>(sA[t] + (4 * cq + j) * GPITCH + 4 * kp) = w[t];
        split_pair<TERMS>(b0[j] * sb, b1[j] * sb, w);
#pragma unroll
        for (int t = 0; t < TERMS; ++t) *reinterpret_cast<unsigned*>(sB[t] + (4 * cq + j) * GPITCH + 4 * kp) = w[t];
      }
    }
  };
  fetch(k_beg);
  for (int k0 = k_beg; k0 < k_end; k0 += GK) {
    __syncthreads();                           // the previous step's fragment reads are done
    commit(k0);
    __syncthreads();
    if (k0 + GK < k_end) fetch(k0 + GK);       // in flight during the MFMAs
#pragma unroll
    for (int s = 0; s < GK / 16; ++s) {
      bf16x8 a[2][TERMS], b[2][TERMS];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < TERMS; ++t) {
          a[i][t] = *reinterpret_cast<const bf16x8*>(sA[t] + (64 * wm + 32 * i + li) * GPITCH + (16 * s + 8 * lh) * 2);
          b[i][t] = *reinterpret_cast<const bf16x8*>(sB[t] + (64 * wn + 32 * i + li) * GPITCH + (16 * s + 8 * lh) * 2);
        }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (TERMS == 3) {
            acc[i][j] = mfma16<TERMS>(a[i][2], b[j][0], acc[i][j]);
            acc[i][j] = mfma16<TERMS>(a[i][1], b[j][1], acc[i][j]);
            acc[i][j] = mfma16<TERMS>(a[i][0], b[j][2], acc[i][j]);
          }
          if constexpr (!AMP) {
            acc[i][j] = mfma16<TERMS>(a[i][1], b[j][0], acc[i][j]);
            acc[i][j] = mfma16<TERMS>(a[i][0], b[j][1], acc[i][j]);
          }
          acc[i][j] = mfma16<TERMS>(a[i][0], b[j][0], acc[i][j]);
        }
    }
  }
  const int nslab = gridDim.x / (ntn * ntm);
  float* Cn = Cp + ((long long)n * nslab + slab) * Cl * J;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + 64 * wn + 32 * j + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + 64 * wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (row < Cl && col < J) Cn[(long long)row * J + col] = acc[i][j][r] * desc;
      }
    }
}

// C (N, Cl, J) = sum over the K slabs, fixed order, fp64
__global__ __launch_bounds__(256) void up2_wgrad_reduce_kernel(const float* __restrict__ Cp, int nslab, long long per,
                                                               float* __restrict__ C) {
  const int n = blockIdx.y;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long long)gridDim.x * 256) {
    double s = 0;
    for (int k = 0; k < nslab; ++k) s += Cp[((long long)n * nslab + k) * per + e];
    C[(long long)n * per + e] = (float)s;
  }
}


// ---- round 5: the same product with the box sums formed ON THE FLY (the 27 box-sum tensors -- 4.5 GB written by up2_boxsum and
// read back by the product above, which ran at the HBM rate of that -- never exist).  Reference: autograd of the decoder's
// interpolate(nearest x2) + cat + SingleConv (keymorph/unet3d/buildingblocks.py:471-475, :46-78).
// One K step = a 4 x 4 x 2 tile of low voxels (32).  Workgroup = 128 rows of Cl x (27 taps x 8 couts = 216 columns, 7 MFMA
// tiles) over a slab of K tiles; wave = one 32-row tile x all 7 column tiles (112 accumulators).  Per step: the tile's
// 10 x 10 x 6 window of dz (8 channels: 19 KB, prefetched during the previous step's MFMAs) goes to LDS as fp32, 192 threads form
// the 32 x 27 x 8 box sums from it with the additions of up2_boxsum_tiled_kernel in the same order (bit-identical sums), scale
// them by S_dz / 8, split them and write the B image; the A image (raw low tensor with GroupNorm's affine) as in the kernel above.
// Two workgroups per CU (76.5 KB of LDS each): one's box sums (VALU) run beside the other's MFMAs.
// Measured (profiles/r5r_up2_wgrad_fold.txt, N = 4, dz channel-blocked): 128 -> 64 at 128^3: 5.12 -> 2.95 ms, 256 -> 128 at 64^3:
// 1.91 -> 1.40 ms.  With the box sums AND the MFMAs compiled out a launch still takes 2.08 / 1.03 ms: the kernel is bound by what
// a CU can load (window 19.2 KB + A rows 16 KB per step: 9.2 GB per launch, mostly L2 hits, at ~ 10 B / cycle / CU); the box sums
// add 0.5 ms, the MFMAs 0.25.  Fetching the window before or after the box sums: no difference.
constexpr int WF_HX = 10, WF_HY = 10, WF_HZ = 6, WF_VOX = WF_HX * WF_HY * WF_HZ;      // window of a 4 x 4 x 2 low tile
constexpr int WF_NC = 224;                                                           // 216 columns, padded to 7 x 32
// MODE (round 5, last): the kernel is bound by what a CU can load, so two of its workgroups become the two halves of ONE
// 512-thread workgroup that share what they both read: MODE 1 = two cout octets over the same A rows (one A image, two windows
// and B images: 54.4 KB of loads per step instead of 70.4), MODE 2 = two 128-row tiles over the same window and box sums (one
// window and B image, two A images: 51.2 KB, and half the box-sum work).  MODE 0 = the 256-thread kernel, two per CU.
// Measured (profiles/r5y_up2_wgrad_fold_modes.txt): MODE 2 -5 % where it applies (256 -> 128 at 64^3: 1.38 -> 1.31 ms); MODE 1
// +3 % (128 -> 64 at 128^3: 2.79 -> 2.88 ms: 23 % fewer bytes, but one workgroup's phases no longer overlap another's) -- it is
// compiled, tested and selectable (KEYMORPH_UP2_FOLD_MODE=1), not chosen.
template <int MODE>
constexpr int wf_lds_bytes() {
  constexpr int NW = MODE == 1 ? 2 : 1, NA = MODE == 2 ? 2 : 1;
  return NW * (WF_VOX * 2 * 16 + 2 * WF_NC * GPITCH) + NA * (2 * 128 * GPITCH + 1024);
}
template <bool AMP, int MODE>
__global__ __launch_bounds__(MODE ? 512 : 256, MODE ? 1 : 2) void up2_wgrad_fold_kernel(
    const float* __restrict__ xl, const float* __restrict__ dz, float* __restrict__ Cp, int Dl, int Hl, int Wl, int Cl, int Cout,
    int tiles_x, int tiles_y, int ktiles, int tiles_per_slab, int ntm /* grid row tiles */, int nto /* grid column groups */,
    const float* __restrict__ ascale, const float* __restrict__ dscale, const float* __restrict__ a_scale,
    const float* __restrict__ a_shift, int dz_blocked, int xcd, const float* __restrict__ zero16) {
  constexpr int NW = MODE == 1 ? 2 : 1, NA = MODE == 2 ? 2 : 1;          // windows + B images, A images
  constexpr int TPBF = MODE ? 512 : 256;
  constexpr int W_BYTES = WF_VOX * 2 * 16, A_BYTES = 2 * 128 * GPITCH, B_BYTES = 2 * WF_NC * GPITCH;
  extern __shared__ __attribute__((aligned(16))) unsigned char wf_lds[];
  unsigned char* sW0 = wf_lds;                                                      // [NW][voxel][2 quads] fp32
  unsigned char* sA0 = sW0 + NW * W_BYTES;                                          // [NA][2 terms][128 rows][GPITCH]
  unsigned char* sB0 = sA0 + NA * A_BYTES;                                          // [NW][2 terms][224 rows][GPITCH]
  float* sC0 = reinterpret_cast<float*>(sB0 + NW * B_BYTES);                        // [NA][2][128]: GroupNorm's affine of the A rows
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int hf = MODE ? tid >> 8 : 0, t8 = tid & 255;                               // the thread's half, its index in it
  const int hw = MODE ? wv >> 2 : 0, wq = wv & 3;                                   // the wave's half, its 32-row tile
  const int n = blockIdx.z;
  int item = xcd ? xcd_remap((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
  const int tn = item % nto; item /= nto;                 // column group (the groups of one K slab read the same rows of xl)
  const int tm = item % ntm;
  const int slab = item / ntm;
  const int oct_t = MODE == 1 ? 2 * tn + hf : tn, oct_w = MODE == 1 ? 2 * tn + hw : tn;              // cout octet: staged / multiplied
  const int m0_t = (MODE == 2 ? 2 * tm + hf : tm) * 128, m0_w = (MODE == 2 ? 2 * tm + hw : tm) * 128;  // first row: staged / multiplied
  const int iw_t = MODE == 1 ? hf : 0, ia_t = MODE == 2 ? hf : 0;                   // the images this thread stages into
  const int D = 2 * Dl, H = 2 * Hl, W = 2 * Wl;
  const long long Vl = (long long)Dl * Hl * Wl, Vh = (long long)D * H * W;
  const float sa = ascale[0], sb = dscale[0] * 0.125f;                             // box sums: |sum of 8| <= 8 max|dz|
  const float desc = ascale[1] * dscale[1] * 8.f;
  const float* xn = xl + (long long)n * Vl * Cl;
  const float* dn = dz + (long long)n * Vh * Cout;
  f32x16 acc[7];
#pragma unroll
  for (int j = 0; j < 7; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  for (int e = tid; e < NW * 2 * 8 * GPITCH / 4; e += TPBF) {                       // columns 216 .. 223 stay zero
    const int im = e / (2 * 8 * GPITCH / 4), r = e % (2 * 8 * GPITCH / 4), t = r / (8 * GPITCH / 4), w = r % (8 * GPITCH / 4);
    reinterpret_cast<unsigned*>(sB0 + im * B_BYTES + t * WF_NC * GPITCH + 216 * GPITCH)[w] = 0u;
  }
  const int t_beg = slab * tiles_per_slab;
  int t_end = t_beg + tiles_per_slab;
  if (t_end > ktiles) t_end = ktiles;
  // staging: the window (600 voxels x 2 quads = 1200 float4) by LDS-DMA, the A rows (16 voxel pairs x 32 quads) through registers
  constexpr int NIW = MODE == 2 ? 3 : 5;                                            // window elements per thread
  constexpr int NIA = MODE == 1 ? 1 : 2;                                            // A items per thread
  float4 pa[NIA][2];
  int x0 = 0, y0 = 0, z0 = 0;                                                       // the tile the registers hold
  auto fetch_w = [&](int t) {                             // the window of tile t
    const int bx = t % tiles_x, by = (t / tiles_x) % tiles_y, bz = t / (tiles_x * tiles_y);
    const int wx = 8 * bx - 1, wy = 8 * by - 1, wz = 4 * bz - 1;
    float4* sWt = reinterpret_cast<float4*>(sW0 + iw_t * W_BYTES);
#pragma unroll
    for (int i = 0; i < NIW; ++i) {
      const int e = (MODE == 2 ? tid + i * 512 : t8 + i * 256), q = e & 1, v = e >> 1;
      const int lx = v % WF_HX, ly = (v / WF_HX) % WF_HY, lz = v / (WF_HX * WF_HY);
      const int ux = wx + lx, uy = wy + ly, uz = wz + lz;
      const bool in = e < 2 * WF_VOX && (unsigned)ux < (unsigned)W && (unsigned)uy < (unsigned)H && (unsigned)uz < (unsigned)D;
      const long long vox = in ? ((long long)uz * H + uy) * W + ux : 0;
      const float* src = dz_blocked ? dn + ((long long)oct_t * Vh + vox) * 8 + 4 * q : dn + vox * Cout + 8 * oct_t + 4 * q;
      // straight into the window (element e = lane-linear: 16 bytes per lane behind a wave-uniform base), no staging
      // registers; voxels outside the volume copy 16 bytes of zeros.  (Past element 1199 a lane must not write: what
      // follows the window in LDS is another image.)  Against the window through registers:
      // profiles/r5w_up2_wgrad_fold_window_by_lds_dma.txt.
      if (e < 2 * WF_VOX)
        __builtin_amdgcn_global_load_lds((kmh_glb_ptr)(in ? src : zero16), (kmh_lds_ptr)(sWt + (e - lane)), 16, 0, 0);
    }
  };
  auto fetch_a = [&](int t) {                             // the A rows of tile t (which becomes the tile the registers hold)
    const int bx = t % tiles_x, by = (t / tiles_x) % tiles_y, bz = t / (tiles_x * tiles_y);
    x0 = 4 * bx; y0 = 4 * by; z0 = 2 * bz;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < NIA; ++i) {
      const int e = (MODE == 1 ? tid : t8 + i * 256), cq = (e & 7) + 8 * (e >> 7), kp = (e >> 3) & 15;      // 8 lanes: one 128-byte line of a voxel row
      const int k = 2 * kp, gx = x0 + (k & 3), gy = y0 + ((k >> 2) & 3), gz = z0 + (k >> 4), ca = m0_t + 4 * cq;
      const bool rowok = gy < Hl && gz < Dl && ca < Cl;
      const float* src = xn + (((long long)gz * Hl + gy) * Wl + gx) * Cl + ca;
      pa[i][0] = (rowok && gx < Wl) ? *reinterpret_cast<const float4*>(src) : z4;
      pa[i][1] = (rowok && gx + 1 < Wl) ? *reinterpret_cast<const float4*>(src + Cl) : z4;
    }
  };
  if ((MODE == 2 ? t8 : tid) < 128) {
    const int c = MODE == 2 ? t8 : tid, ca = m0_t + c;
    float* sC = sC0 + ia_t * 256;
    sC[c] = (a_scale && ca < Cl) ? a_scale[(long long)n * Cl + ca] : 1.f;
    sC[128 + c] = (a_scale && ca < Cl) ? a_shift[(long long)n * Cl + ca] : 0.f;
  }
  auto commit = [&]() {                                   // registers -> the A image (tile x0, y0, z0)
    unsigned char* sA = sA0 + ia_t * A_BYTES;
    const float* sC = sC0 + ia_t * 256;
#pragma unroll
    for (int i = 0; i < NIA; ++i) {
      const int e = (MODE == 1 ? tid : t8 + i * 256), cq = (e & 7) + 8 * (e >> 7), kp = (e >> 3) & 15;
      const int k = 2 * kp, gx = x0 + (k & 3), gy = y0 + ((k >> 2) & 3), gz = z0 + (k >> 4);
      const bool rowok = gy < Hl && gz < Dl;
      const bool v0 = rowok && gx < Wl, v1 = rowok && gx + 1 < Wl;              // voxels past the volume: zero rows (no shift)
      const float4 sc = *reinterpret_cast<const float4*>(sC + 4 * cq), sh = *reinterpret_cast<const float4*>(sC + 128 + 4 * cq);
      const float a0[4] = {v0 ? fmaf(pa[i][0].x, sc.x, sh.x) : 0.f, v0 ? fmaf(pa[i][0].y, sc.y, sh.y) : 0.f,
                           v0 ? fmaf(pa[i][0].z, sc.z, sh.z) : 0.f, v0 ? fmaf(pa[i][0].w, sc.w, sh.w) : 0.f};
      const float a1[4] = {v1 ? fmaf(pa[i][1].x, sc.x, sh.x) : 0.f, v1 ? fmaf(pa[i][1].y, sc.y, sh.y) : 0.f,
                           v1 ? fmaf(pa[i][1].z, sc.z, sh.z) : 0.f, v1 ? fmaf(pa[i][1].w, sc.w, sh.w) : 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned w[2];
        split_pair<2>(a0[j] * sa, a1[j] * sa, w);
#pragma unroll
        for (int t = 0; t < 2; ++t) *reinterpret_cast<unsigned*>(sA + t * 128 * GPITCH + (4 * cq + j) * GPITCH + 4 * kp) = w[t];
      }
    }
  };
  auto boxes = [&]() {                                    // window -> the B image: thread = (low voxel m, kz, channel quad q)
    const int bt = MODE == 1 ? t8 : tid;                  // (MODE 1: 192 threads of each half; else the first 192 of the workgroup)
    if (bt >= 192) return;
    const float4* sW = reinterpret_cast<const float4*>(sW0 + iw_t * W_BYTES);
    unsigned char* sB = sB0 + iw_t * B_BYTES;
    // a WAVE = one kz: (q, low voxel m) vary over its lanes.  With kz across the lanes (round 5) three lanes of every quad of
    // lanes wrote the same bank of the B image (72 columns x 80 bytes = 0 mod 128 bytes between the kz groups) and read window
    // planes 32 banks apart: 58 % of the kernel's LDS-active cycles were bank conflicts at 59 % LDS busy
    // (profiles/r6n_lds_by_kernel.txt).  Same sums per (m, kz, q), same order: bit-identical.
    const int q = bt & 1, kz = bt >> 6, m = (bt >> 1) & 31;
    const int lmx = m & 3, lmy = (m >> 2) & 3, lmz = m >> 4;
    float4 Y[3][3];
#pragma unroll
    for (int a = 0; a < 9; ++a) (&Y[0][0])[a] = make_float4(0.f, 0.f, 0.f, 0.f);
    // window index i = u - (2m - 1) in 0..3 per axis; tap k (offset k - 1) sums i in {2 - k, 3 - k}
#pragma unroll
    for (int dzp = 0; dzp < 2; ++dzp) {
      const int lz = 2 * lmz + (2 - kz) + dzp;
#pragma unroll
      for (int iy = 0; iy < 4; ++iy) {
        const float4* row = sW + (((lz * WF_HY + 2 * lmy + iy) * WF_HX + 2 * lmx) * 2 + q);
        const float4 a4[4] = {row[0], row[2], row[4], row[6]};
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float4 u = a4[2 - kx], v = a4[3 - kx];
          const float4 xs = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
            if (iy == 2 - ky || iy == 3 - ky) {
              Y[ky][kx].x += xs.x; Y[ky][kx].y += xs.y; Y[ky][kx].z += xs.z; Y[ky][kx].w += xs.w;
            }
        }
        __builtin_amdgcn_sched_barrier(0);     // (one window row at a time: 32 rows hoisted together spill the accumulators)
      }
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) {
      const float4 y = (&Y[0][0])[a];
      const int col = (kz * 9 + a) * 8 + 4 * q;            // column = tap x 8 + cout within the octet
      unsigned w01[2], w23[2];
      split_pair<2>(y.x * sb, y.y * sb, w01);
      split_pair<2>(y.z * sb, y.w * sb, w23);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        unsigned char* base = sB + t * WF_NC * GPITCH + col * GPITCH + 2 * m;
        *reinterpret_cast<unsigned short*>(base) = (unsigned short)(w01[t] & 0xffffu);
        *reinterpret_cast<unsigned short*>(base + GPITCH) = (unsigned short)(w01[t] >> 16);
        *reinterpret_cast<unsigned short*>(base + 2 * GPITCH) = (unsigned short)(w23[t] & 0xffffu);
        *reinterpret_cast<unsigned short*>(base + 3 * GPITCH) = (unsigned short)(w23[t] >> 16);
      }
    }
  };
  if (t_beg < t_end) { fetch_w(t_beg); fetch_a(t_beg); }
  const unsigned char* sAw = sA0 + (MODE == 2 ? hw : 0) * A_BYTES;                  // the images this wave multiplies
  const unsigned char* sBw = sB0 + (MODE == 1 ? hw : 0) * B_BYTES;
  for (int t = t_beg; t < t_end; ++t) {
    __syncthreads();                           // the previous step's fragment reads are done
    commit();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // this lane's pieces of the window are in LDS
    __syncthreads();
    boxes();
    __syncthreads();
    if (t + 1 < t_end) {                       // the next window and A rows: during the MFMAs (after the box sums: the window is
      fetch_w(t + 1);                          // read, their registers are free again)
      fetch_a(t + 1);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 a[2], b[2];
#pragma unroll
      for (int q = 0; q < 2; ++q)
        a[q] = *reinterpret_cast<const bf16x8*>(sAw + q * 128 * GPITCH + (32 * wq + li) * GPITCH + (16 * s + 8 * lh) * 2);
#pragma unroll
      for (int j = 0; j < 7; ++j) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
          b[q] = *reinterpret_cast<const bf16x8*>(sBw + q * WF_NC * GPITCH + (32 * j + li) * GPITCH + (16 * s + 8 * lh) * 2);
        if constexpr (!AMP) {
          acc[j] = mfma16<2>(a[1], b[0], acc[j]);
          acc[j] = mfma16<2>(a[0], b[1], acc[j]);
        }
        acc[j] = mfma16<2>(a[0], b[0], acc[j]);
      }
    }
  }
  const int nslab = gridDim.x / (nto * ntm);
  const int J = 27 * Cout;
  float* Cn = Cp + ((long long)n * nslab + slab) * Cl * J;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const int col = 32 * j + li;
    const int jj = (col >> 3) * Cout + 8 * oct_w + (col & 7);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0_w + 32 * wq + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (row < Cl && col < 216) Cn[(long long)row * J + jj] = acc[j][r] * desc;
    }
  }
}

}  // namespace

// XCD-aware workgroup order of the two weight-gradient kernels: always on.  (The kernels keep the argument their retired A/B
// switch fed; taking it out changes their code and wants a timing of its own.)
constexpr int kUp2Xcd = 1;
// C (N, per) = the sum of the ns partial slabs of every sample; returns the launch status
static int up2_reduce(const void* ws, int ns, long long per, float* C, int N, hipStream_t s) {
  int nb = ceil_div(per, 256);
  if (nb > 1024) nb = 1024;
  up2_wgrad_reduce_kernel<<<dim3(nb, N), 256, 0, s>>>((const float*)ws, ns, per, C);
  return KMH_LAUNCH_CHECK();
}

static int up2_wgrad_slabs(int V, int Cl, int J, int N, int* kslab) {
  const int tiles = ceil_div(Cl, 128) * ceil_div(J, 128) * N;
  int want = 2048 / tiles;                    // ~2048 workgroups
  if (want < 1) want = 1;
  int ks = ceil_div(V, want);
  ks = (ks + GK - 1) / GK * GK;
  *kslab = ks;
  return ceil_div(V, ks);
}

KMH_API size_t kmh_up2_wgrad_gemm_ws_bytes(int N, int V, int Cl, int J) {
  int ks;
  const int ns = up2_wgrad_slabs(V, Cl, J, N, &ks);
  return (size_t)N * ns * Cl * J * sizeof(float);
}

/* C (N, Cl, J) = A^T B per sample: A (N, V, Cl) the normalised low tensor, B (N, V, J) the box sums (kmh_up2_boxsum);
 * Cl % 4 == 0, J % 4 == 0; ascale / bscale = {S, 1/S} range scales of A and B (terms == 2). */
KMH_API int kmh_up2_wgrad_gemm(const float* A, const float* B, float* C, int N, int V, int Cl, int J, int terms,
                               const float* ascale, const float* bscale, const float* a_scale, const float* a_shift,
                               void* ws, void* stream) {
  const bool amp = kmh_take_amp(terms);      // terms == 1: the fp16 kernels with hi x hi only (use_amp), for this call
  if ((Cl & 3) || (J & 3) || (terms != 2 && terms != 3) || (terms == 2 && (!ascale || !bscale)) || (!a_scale != !a_shift))
    return -22;
  int ks;
  const int ns = up2_wgrad_slabs(V, Cl, J, N, &ks);
  const int ntn = ceil_div(J, 128), ntm = ceil_div(Cl, 128);
  hipStream_t s = (hipStream_t)stream;
  dim3 g(ntn * ntm * ns, 1, N);
  if (terms == 2)
    if (amp)
      up2_wgrad_gemm_kernel<2, true><<<g, 256, 0, s>>>(A, B, (float*)ws, V, Cl, J, ks, ntn, ntm, ascale, bscale, a_scale, a_shift, kUp2Xcd);
    else
    up2_wgrad_gemm_kernel<2><<<g, 256, 0, s>>>(A, B, (float*)ws, V, Cl, J, ks, ntn, ntm, ascale, bscale, a_scale, a_shift, kUp2Xcd);
  else
    up2_wgrad_gemm_kernel<3><<<g, 256, 0, s>>>(A, B, (float*)ws, V, Cl, J, ks, ntn, ntm, ascale, bscale, a_scale, a_shift, kUp2Xcd);
  return up2_reduce(ws, ns, (long long)Cl * J, C, N, s);
}

// which fold kernel: 2 = two row tiles per workgroup (Cl > 128 with an even tile count), 1 = two cout octets, 0 = the 256-thread one
// (KEYMORPH_UP2_FOLD_MODE=0|1|2 forces one where it applies: A/B runs)
static int up2_fold_mode(int Cl, int Cout) {
  const int ntm = ceil_div(Cl, 128), nto = Cout / 8;
  int mode = (ntm % 2 == 0) ? 2 : 0;      // (MODE 1 measured 3 % SLOWER than two 256-thread workgroups per CU: forced only)
  const char* env = getenv("KEYMORPH_UP2_FOLD_MODE");       // (read per call: the tests switch it)
  if (env) {
    const int want = atoi(env);
    if (want == 0 || (want == 1 && nto % 2 == 0) || (want == 2 && ntm % 2 == 0)) mode = want;
  }
  return mode;
}

static int up2_fold_slabs(int N, int Dl, int Hl, int Wl, int Cl, int Cout, int* tiles_per_slab, int* ktiles) {
  const int kt = ceil_div(Wl, 4) * ceil_div(Hl, 4) * ceil_div(Dl, 2);
  const int mode = up2_fold_mode(Cl, Cout);
  const int per = (Cout / 8) * ceil_div(Cl, 128) * N / (mode ? 2 : 1);       // workgroups per slab
  int want = ceil_div(mode ? 256 : 512, per);               // one 512-thread or two 256-thread workgroups per CU
  if (want < 1) want = 1;
  if (want > kt) want = kt;
  const int tps = ceil_div(kt, want);
  *tiles_per_slab = tps;
  *ktiles = kt;
  return ceil_div(kt, tps);
}

/* 1 if kmh_up2_wgrad_fold takes this configuration (fp16 split, whole cout octets), else 0 */
KMH_API int kmh_up2_wgrad_fold_ok(int Cl, int Cout, int terms) {
  return (terms == 2 && Cl > 0 && (Cl & 3) == 0 && Cout > 0 && (Cout & 7) == 0) ? 1 : 0;
}

static inline size_t up2_fold_slab_bytes(int N, int Dl, int Hl, int Wl, int Cl, int Cout) {
  int tps, kt;
  const int ns = up2_fold_slabs(N, Dl, Hl, Wl, Cl, Cout, &tps, &kt);
  return (((size_t)N * ns * Cl * 27 * Cout * sizeof(float)) + 255) & ~(size_t)255;
}
/* the partial slabs + 256 bytes of zeros (the source of window voxels outside the volume; written by every call on its stream) */
KMH_API size_t kmh_up2_wgrad_fold_ws_bytes(int N, int Dl, int Hl, int Wl, int Cl, int Cout) {
  return up2_fold_slab_bytes(N, Dl, Hl, Wl, Cl, Cout) + 256;
}

template <bool AMP, int MODE>
static int launch_up2_fold(dim3 g, hipStream_t s, const float* xl, const float* dz, float* ws, int Dl, int Hl, int Wl, int Cl, int Cout,
                           int kt, int tps, int ntm, int nto, const float* ascale, const float* dscale, const float* a_scale,
                           const float* a_shift, int dz_blocked, const float* zero16) {
  constexpr int lds = wf_lds_bytes<MODE>();
  hipError_t e = hipFuncSetAttribute((const void*)up2_wgrad_fold_kernel<AMP, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return (int)e;
  up2_wgrad_fold_kernel<AMP, MODE><<<g, MODE ? 512 : 256, lds, s>>>(xl, dz, ws, Dl, Hl, Wl, Cl, Cout, ceil_div(Wl, 4), ceil_div(Hl, 4),
                                                                  kt, tps, ntm, nto, ascale, dscale, a_scale, a_shift, dz_blocked,
                                                                  kUp2Xcd, zero16);
  return 0;
}

/* C (N, Cl, 27 Cout) = kmh_up2_wgrad_gemm(xl, kmh_up2_boxsum(dz)) without the box-sum tensor: xl (N, Dl, Hl, Wl, Cl) the raw
 * low tensor (a_scale / a_shift: GroupNorm's affine, or both NULL), dz (N, 2Dl, 2Hl, 2Wl, Cout) or channel-blocked
 * (dz_blocked), ascale / dscale = {S, 1/S} range scales of the normalised low tensor and of dz; terms: 2, or 1 = hi x hi only
 * (use_amp); ws: kmh_up2_wgrad_fold_ws_bytes, 16-byte aligned. */
KMH_API int kmh_up2_wgrad_fold(const float* xl, const float* dz, float* C, int N, int Dl, int Hl, int Wl, int Cl, int Cout,
                               int terms, const float* ascale, const float* dscale, const float* a_scale, const float* a_shift,
                               int dz_blocked, void* ws, void* stream) {
  const bool amp = kmh_take_amp(terms);      // terms == 1: hi x hi only (use_amp), for this call
  if (!ws || ((uintptr_t)ws & 15) || !kmh_up2_wgrad_fold_ok(Cl, Cout, terms) || !ascale || !dscale || (!a_scale != !a_shift) || N <= 0 || N > 65535) return -22;
  int tps, kt;
  const int ns = up2_fold_slabs(N, Dl, Hl, Wl, Cl, Cout, &tps, &kt);
  const int mode = up2_fold_mode(Cl, Cout);
  const int nto = (Cout / 8) / (mode == 1 ? 2 : 1), ntm = ceil_div(Cl, 128) / (mode == 2 ? 2 : 1);      // as the grid sees them
  hipStream_t s = (hipStream_t)stream;
  dim3 g(nto * ntm * ns, 1, N);
  // 256 bytes of zeros behind the slabs: the LDS-DMA source of window voxels outside the volume.  From the caller's workspace,
  // zeroed on the caller's stream: no allocation, no host synchronisation, nothing process-wide (stream capture stays legal).
  const float* zero16 = (const float*)((const char*)ws + up2_fold_slab_bytes(N, Dl, Hl, Wl, Cl, Cout));
  if (hipMemsetAsync((void*)zero16, 0, 256, s) != hipSuccess) return -12;
  int rc;
#define KMH_FOLD(A, M) launch_up2_fold<A, M>(g, s, xl, dz, (float*)ws, Dl, Hl, Wl, Cl, Cout, kt, tps, ntm, nto, ascale, dscale, \
                                             a_scale, a_shift, dz_blocked, zero16)
  if (mode == 2) rc = amp ? KMH_FOLD(true, 2) : KMH_FOLD(false, 2);
  else if (mode == 1) rc = amp ? KMH_FOLD(true, 1) : KMH_FOLD(false, 1);
  else rc = amp ? KMH_FOLD(true, 0) : KMH_FOLD(false, 0);
#undef KMH_FOLD
  if (rc) return rc;
  return up2_reduce(ws, ns, (long long)Cl * 27 * Cout, C, N, s);
}

KMH_API size_t kmh_conv3d_up2_dgrad_pack_bytes(int Cout, int Cl, int terms) {
  const int CiP = (Cl + 127) & ~127;
  return (size_t)((Cout + 7) / 8) * terms * DUP_NST * 2 * CiP * 8 * sizeof(__bf16);
}

KMH_API int kmh_conv3d_up2_dgrad_pack_weight(const float* w, void* packed, int Cout, int Ctot, int cofs, int Cl, int terms,
                                             const float* wscale, void* stream) {
  if (cofs < 0 || cofs + Cl > Ctot || (terms != 2 && terms != 3) || (terms == 2 && !wscale)) return -22;
  const int CiP = (Cl + 127) & ~127, nchunk = (Cout + 7) / 8;
  const long long total = (long long)nchunk * DUP_NST * 2 * CiP * 8;
  int nb = ceil_div(total, 256);
  if (nb > 2048) nb = 2048;
  hipStream_t s = (hipStream_t)stream;
  if (terms == 2) pack_weight_upt_kernel<2><<<nb, 256, 0, s>>>(w, (__bf16*)packed, Cout, Ctot, cofs, Cl, CiP, nchunk, wscale);
  else pack_weight_upt_kernel<3><<<nb, 256, 0, s>>>(w, (__bf16*)packed, Cout, Ctot, cofs, Cl, CiP, nchunk, wscale);
  return KMH_LAUNCH_CHECK();
}

/* ds (N,Dl,Hl,Wl,Cl) = for every low voxel, the sum over its 8 children of the gradient of conv3(up2(.), w[:, cofs:cofs+Cl])
 * with respect to the upsampled tensor, from dz (N,2Dl,2Hl,2Wl,Cout) (no ReLU mask operand: dz is already masked). */
KMH_API size_t kmh_conv3d_up2_dgrad_stats_ws_bytes(int N, int Dl, int Hl, int Wl, int Cl) {
  return (size_t)N * ceil_div(Wl, DUX) * ceil_div(Hl, DUY) * Dl * Cl * 2 * sizeof(double);
}
/* stats_out (N,Cl,2) doubles | NULL (then stats_ws may be NULL): per-channel (sum ds, sum ds^2), from the epilogue */
KMH_API int kmh_conv3d_up2_dgrad(const float* dz, const void* packed, float* ds, int N, int Dl, int Hl, int Wl, int Cl,
                                 int Cout, int terms, const float* dscale, const float* wscale, void* stats_ws,
                                 double* stats_out, int in_blocked, void* stream) {
  const bool amp = kmh_take_amp(terms);      // terms == 1: the fp16 kernels with hi x hi only (use_amp), for this call
  if ((terms != 2 && terms != 3) || (terms == 2 && (!dscale || !wscale)) || (stats_out && !stats_ws)) return -22;
  if (in_blocked && (Cout & 7)) return -22;               // whole 8-channel chunks
  const int CiP = (Cl + 127) & ~127;
  const int tx = ceil_div(Wl, DUX), ty = ceil_div(Hl, DUY);
  dim3 g(tx * ty * Dl * ceil_div(Cl, 128), 1, N);
  hipStream_t s = (hipStream_t)stream;
  double* sp = stats_out ? (double*)stats_ws : nullptr;
  if (terms == 2)
    if (amp)
      conv3_up2_dgrad_kernel<2, true><<<g, DUP_TPB, 0, s>>>(dz, (const bf16x8*)packed, ds, Dl, Hl, Wl, Cl, CiP, Cout, tx, ty, dscale, wscale, sp, in_blocked);
    else
    conv3_up2_dgrad_kernel<2><<<g, DUP_TPB, 0, s>>>(dz, (const bf16x8*)packed, ds, Dl, Hl, Wl, Cl, CiP, Cout, tx, ty, dscale, wscale, sp, in_blocked);
  else
    conv3_up2_dgrad_kernel<3><<<g, DUP_TPB, 0, s>>>(dz, (const bf16x8*)packed, ds, Dl, Hl, Wl, Cl, CiP, Cout, tx, ty, dscale, wscale, sp, in_blocked);
  if (stats_out)
    kmh_stats::final_kernel<<<dim3(ceil_div(Cl * 2, 256 / kWave), N), 256, 0, s>>>(sp, tx * ty * Dl, Cl, stats_out);
  return KMH_LAUNCH_CHECK();
}

KMH_API size_t kmh_conv3d_up2_pack_bytes(int Cout, int Cl, int terms) {
  return (size_t)(Cl / 8) * terms * UP_NST * 2 * cout_pad(Cout) * 8 * sizeof(__bf16);
}

/* w (Cout, Ctot, 3,3,3): the channels [cofs, cofs + Cl) are the upsampled ones; wscale {S, 1/S} must leave room for the
 * sum of 8 taps (the host passes the 27-tap scale / 8). */
KMH_API int kmh_conv3d_up2_pack_weight(const float* w, void* packed, int Cout, int Ctot, int cofs, int Cl, int terms,
                                       const float* wscale, void* stream) {
  if ((Cl & 7) || cofs < 0 || cofs + Cl > Ctot || (terms != 2 && terms != 3) || (terms == 2 && !wscale)) return -22;
  const int CoutP = cout_pad(Cout), nchunk = Cl / 8;
  const long long total = (long long)nchunk * UP_NST * 2 * CoutP * 8;
  int nb = ceil_div(total, 256);
  if (nb > 2048) nb = 2048;
  hipStream_t s = (hipStream_t)stream;
  if (terms == 2) pack_weight_up_kernel<2><<<nb, 256, 0, s>>>(w, (__bf16*)packed, Cout, Ctot, cofs, Cl, CoutP, nchunk, wscale);
  else pack_weight_up_kernel<3><<<nb, 256, 0, s>>>(w, (__bf16*)packed, Cout, Ctot, cofs, Cl, CoutP, nchunk, wscale);
  return KMH_LAUNCH_CHECK();
}

/* y (N, 2Dl, 2Hl, 2Wl, Cout) = conv3(up2_nearest(norm(xl)), w[:, cofs:cofs+Cl]) with norm = the (N, Ctot) GroupNorm
 * coefficients at channel offset cofs -- the contribution of the upsampled half of a decoder's concatenated input
 * (keymorph/unet3d/buildingblocks.py:471-475 + 46-78), to be passed as `addend` to kmh_conv3d_fwd_bf over the skip
 * half.  No bias, no activation. */
KMH_API int kmh_conv3d_up2_fwd(const float* xl, const float* scale, const float* shift, int Ctot, int cofs,
                               const void* packed, float* y, int N, int Dl, int Hl, int Wl, int Cl, int Cout, int terms,
                               const float* ascale, const float* wscale, void* stream) {
  const bool amp = kmh_take_amp(terms);      // terms == 1: the fp16 kernels with hi x hi only (use_amp), for this call
  if ((Cl & 7) || (terms != 2 && terms != 3) || (terms == 2 && (!ascale || !wscale))) return -22;
  if ((long long)Dl * Hl * Wl * Cl >= (1ll << 31)) return -22;
  const int CoutP = cout_pad(Cout);
  const int tx = ceil_div(Wl, UX), ty = ceil_div(Hl, UY);
  dim3 g(tx * ty * Dl * ceil_div(Cout, 64), 1, N);
  hipStream_t s = (hipStream_t)stream;
  if (terms == 2)
    if (amp)
      conv3_up2_fwd_kernel<2, true><<<g, UP_TPB, 0, s>>>(xl, scale, shift, Ctot, cofs, (const bf16x8*)packed, y, Dl, Hl, Wl, Cl,
                                                Cout, CoutP, tx, ty, ascale, wscale);
    else
    conv3_up2_fwd_kernel<2><<<g, UP_TPB, 0, s>>>(xl, scale, shift, Ctot, cofs, (const bf16x8*)packed, y, Dl, Hl, Wl, Cl,
                                                Cout, CoutP, tx, ty, ascale, wscale);
  else
    conv3_up2_fwd_kernel<3><<<g, UP_TPB, 0, s>>>(xl, scale, shift, Ctot, cofs, (const bf16x8*)packed, y, Dl, Hl, Wl, Cl,
                                                Cout, CoutP, tx, ty, ascale, wscale);
  return KMH_LAUNCH_CHECK();
}
