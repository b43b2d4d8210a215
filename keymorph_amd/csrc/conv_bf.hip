// fp32-accurate 3x3x3 convolution on the 16-bit matrix cores: every fp32 operand is split exactly into 16-bit terms
// and each product is accumulated in fp32 from the significant term products --
//   TERMS = 2 ("f16x3", the default): operands range-scaled by a power of two, x S = hi + lo in fp16 (22 bits),
//              products hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16, exact descale in the epilogue;
//   TERMS = 3 ("bf16x6"): x = hi + mid + lo in bf16 (24 bits), six products on v_mfma_f32_32x32x16_bf16.
// Both are fp32-class (5e-7 against fp64, like the fp32 MFMA); on CDNA4 the 16-bit MFMA rate is 16x the fp32 MFMA rate,
// so this is 16/3 = 5.3x (16/6 = 2.7x) the fp32-MFMA roofline -- the 3xTF32 / BF16x9 idea on gfx950's 32x32x16 tile.
//
// Kernels in this file, the forward / data-gradient family (fused decoder operator: conv_up2.hip, weight gradient: conv_wgrad.hip):
//   conv3_fwd_bf_kernel<NT, TERMS, MR, ZP, ZT>   forward and data gradient (same kernel on tap-mirrored weights);
//                                                 NT = 32-wide cout tiles per wave, MR = rows per wave, ZP = z-paired N
//                                                 tile for Cout <= 16, ZT = output-plane pairs per brick
//   conv3_fwd_g_kernel<NT, ZP, POOL>             the same on big launches: persistent workgroups, LDS-DMA staging, eight waves
//   conv3_fwd_s_kernel<NT, ZP, SPLIT, POOL, AMP, SPARSE> one wave per SIMD, hand-counted waits (audited: keymorph_amd/isa_audit.py)
//   pack_weight_bf_kernel<TERMS>
//
// Forward: same brick / wave decomposition as conv.hip (32x8x2 output voxels per 4-wave workgroup, 4 rows x NT
// channel tiles per wave), but:
//   * the halo brick is split while it is staged (GroupNorm scale/shift, ReLU, fused ReLU-backward mask first, then
//     packed 16-bit conversions) into TERMS voxel-major LDS images of 16-byte rows (8 channels), so an A fragment is
//     ONE conflict-free ds_read_b128 per term: 32 consecutive voxels x 8 channels;
//   * K = 16 of an MFMA = 2 taps x 8 channels: lanes 0-31 carry tap 2s, lanes 32-63 tap 2s+1 (27 taps =
//     13 pairs + one half-empty step whose weights are zero);
//   * the filter is pre-packed as [cin/8][term][step][half][cout][8] 16-bit values, so a B fragment is one
//     512-byte-per-half-wave global_load_dwordx4 from L2, prefetched through a register ring;
//   * the epilogue can emit the (sum, sum of squares) per channel that the next GroupNorm needs.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include "conv_split.h"
#include "stats_final.h"
#include <type_traits>

namespace {

constexpr int TX = 32, TZ = 2;
constexpr int HX = TX + 2, HZ = TZ + 2;
// MR = output rows (M-tiles) per wave: brick height TY = 2*MR.  MR = 4: 32x8x2 brick, 1360-voxel halo;
// MR = 2: 32x4x2 brick, 816-voxel halo -> 39 KB of LDS (TERMS = 3) and 64 accumulator registers, i.e. 3-4
// resident workgroups per CU instead of 2.
constexpr int NSTEP = 14;          // tap pairs
constexpr int BF_TPB = 256;

// torch (Cout, Cin, 27) -> [nchunk][TERMS][nstep][2][CoutP][8] bf16 (zero padded); transposed = data gradient.
// zpair (logical Cout <= 16): the 32 columns are (co, pz) = (j & 15, j >> 4) -- the SAME 16 output channels for the
// two output planes z0, z0+1 of a brick, which share the 4-plane input window; taps run over kz' in 0..3 (36 taps,
// nstep = 18) and column (co, pz) carries w[kz' - pz] where that is a valid tap, 0 elsewhere.
constexpr int NSTEP_Z = 18;
template <int TERMS>
__global__ __launch_bounds__(256) void pack_weight_bf_kernel(const float* __restrict__ w, __bf16* __restrict__ out,
                                                             int Cout, int Cin, int CoutP, int nchunk,
                                                             int transposed, int zpair,
                                                             const float* __restrict__ wscale /* {S, 1/S} | NULL */) {
  // logical filter L[co][ci][tap] with (Co, Ci) = transposed ? (Cin, Cout) : (Cout, Cin)
  const int Co = transposed ? Cin : Cout, Ci = transposed ? Cout : Cin;
  const int nstep = zpair ? NSTEP_Z : NSTEP;
  const long long total = (long long)nchunk * nstep * 2 * CoutP * 8;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int c = (int)(e & 7);
    long long r = e >> 3;
    const int col = (int)(r % CoutP); r /= CoutP;
    const int h = (int)(r & 1); r >>= 1;
    const int s = (int)(r % nstep);
    const int chunk = (int)(r / nstep);
    const int ci = chunk * 8 + c;
    int tap = 2 * s + h, co = col;
    bool ok = tap < 27;
    if (zpair) {
      const int kz = tap / 9 - (col >> 4);          // tap = kz' * 9 + ky * 3 + kx
      co = col & 15;
      ok = (col < 32) && kz >= 0 && kz <= 2;
      tap = kz * 9 + tap % 9;
    }
    float v = 0.f;
    if (ok && ci < Ci && co < Co)
      v = transposed ? w[((long long)ci * Cin + co) * 27 + (26 - tap)] : w[((long long)co * Cin + ci) * 27 + tap];
    float rem = wscale ? v * wscale[0] : v;
#pragma unroll
    for (int t = 0; t < TERMS; ++t) {
      float back;
      const unsigned short hb = to16<TERMS>(rem, back);
      reinterpret_cast<unsigned short*>(out)[((((long long)chunk * TERMS + t) * nstep + s) * 2 + h) * CoutP * 8 +
                                             (long long)col * 8 + c] = hb;
      rem -= back;
    }
  }
}

// ZT = output-plane pairs per brick: 1 -> 32 x TY x 2 bricks (4 input planes per 2 output planes), 2 -> 32 x TY x 4
// bricks (6 per 4: the halo re-read factor drops from 2.66 to 1.99 and every B fragment feeds twice the MFMAs) for
// the low-channel layers of the full-resolution level, which are bound by input traffic, not by the matrix pipe.
template <int NT, int TERMS, int MR, bool ZP = false, int ZT = 1>
__global__ __launch_bounds__(BF_TPB, ((MR == 2 && NT == 2 && TERMS == 3) ? 3 : 2)) void conv3_fwd_bf_kernel(
    const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ mask, const bf16x8* __restrict__ wp, const float* __restrict__ bias,
    float* __restrict__ y, int D, int H, int W, int Cin, int Cout, int CoutP, int relu_in, int relu_out,
    int tiles_x, int tiles_y, int tiles_z, int tiles_zp, const float* __restrict__ ascale /* {S, 1/S} of the input | NULL */,
    const float* __restrict__ wscale /* of the packed weights | NULL */,
    double* __restrict__ stats_partial /* (N, bricks, Cout, 2) per-brick (sum y, sum y^2) | NULL */,
    int in_blocked /* x is (N, Cin/8, D, H, W, 8): a chunk's voxels are contiguous 32-byte records */,
    const float* __restrict__ addend /* like y | NULL: added before the activation (not for the z-paired variant) */) {
  // ZP: the 4 waves split the brick's y rows (MR each) and every wave produces BOTH z planes in its N tile
  constexpr int TZv = 2 * ZT, HZv = TZv + 2;
  constexpr int TY = (ZP ? 4 : 2) * MR, HY = TY + 2, PL = HX * HY * HZv;
  constexpr int NST = ZP ? NSTEP_Z : NSTEP;
  static_assert(!ZP || NT == 1, "z-paired tiles are for Cout <= 16");
  __shared__ bf16x8 sIn[TERMS][PL];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int n = blockIdx.z;
  // work item = (brick, cout group) with the cout group fastest, XCD-remapped (common.h)
  const int ncog = ZP ? 1 : (Cout + 32 * NT - 1) / (32 * NT);
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  const int cog = item % ncog, brick = item / ncog;
  // Brick order: the ~64 bricks an XCD has in flight form an 8 x 8 patch in (y, z) -- the directions in which
  // neighbouring halos overlap most (2 of 4 planes in z, 2 of 10 rows in y, only 2 of 34 columns in x) -- so the
  // shared planes are fetched into that XCD's L2 once instead of once per brick.  Patches are padded to 8 x 8;
  // workgroups of the padding exit here (before any barrier).
  const int tyz = (tiles_y + 7) >> 3;
  const int lz8 = brick & 7, ly8 = (brick >> 3) & 7, patch = brick >> 6;
  const int pyi = patch % tyz, rest = patch / tyz;
  const int pzi = rest % tiles_zp, bx = rest / tiles_zp;
  const int by = pyi * 8 + ly8, bz = pzi * 8 + lz8;
  if (by >= tiles_y || bz >= tiles_z) return;
  const int x0 = bx * TX, y0 = by * TY, z0 = bz * TZv;
  const int co0 = cog * (32 * NT);
  const int wz = ZP ? 0 : wv >> 1, wy = (ZP ? wv : (wv & 1)) * MR;

  f32x16 acc[ZT][MR][NT];
#pragma unroll
  for (int p = 0; p < ZT; ++p)
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[p][m][t][r] = 0.f;

  const float sA = ascale ? ascale[0] : 1.f;                                   // power of two: folding it into the
  const float desc = (ascale ? ascale[1] : 1.f) * (wscale ? wscale[1] : 1.f);   // coefficients and the epilogue is exact
  const bool vec4 = (Cin & 3) == 0;
  const int nchunk = (Cin + KC - 1) / KC;
  const int vrow = (wz * HY + wy) * HX + li;    // this lane's voxel in the wave's first row, tap (0,0,0)

  // staging descriptors: this thread's (up to 6) halo voxels are the same for every channel chunk
  constexpr int NV = (PL + BF_TPB - 1) / BF_TPB;      // 6
  int sv_rel[NV];                                     // element offset of the voxel relative to the brick origin
  bool sv_in[NV];                                     // inside the volume?
  const long long origin = ((((long long)n * D + z0) * H + y0) * W + x0) * Cin;   // may address the halo "before" it
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = tid + i * BF_TPB;
    const int lx = v % HX, ly = (v / HX) % HY, lz = v / (HX * HY);
    const int gx = x0 + lx - 1, gy = y0 + ly - 1, gz = z0 + lz - 1;
    sv_in[i] = (v < PL) && ((unsigned)gx < (unsigned)W) && ((unsigned)gy < (unsigned)H) && ((unsigned)gz < (unsigned)D);
    sv_rel[i] = (((lz - 1) * H + (ly - 1)) * W + (lx - 1)) * (in_blocked ? KC : Cin);
  }
  // channel-blocked input: chunk ch of sample n starts at ((n * nchunk + ch) * D*H*W) * 8 floats
  const long long chunk_stride = in_blocked ? (long long)D * H * W * KC : KC;
  const float* xb = in_blocked ? x + ((long long)n * nchunk * D * H * W + (((long long)z0 * H + y0) * W + x0)) * KC : x + origin;
  const float* mb = mask ? mask + origin : nullptr;
  // per-lane B offset (in bf16x8 units) of step 0; step s adds 2*CoutP, term q adds NSTEP*2*CoutP
  const int boff = lh * CoutP + co0 + li;

  // staging = fetch (global -> registers, raw) + commit (mask, normalise, ReLU, zero padding, split, LDS).
  // PF (z-paired variant: 32 accumulator registers, short MFMA phase per chunk): the fetch of chunk ch+1 is in
  // flight during the MFMAs of chunk ch; otherwise fetch and commit run back to back, one voxel at a time.
  constexpr bool PF = false;   // measured: no gain for the z-paired variant (its exposed latency is the B loads)
  constexpr int NPRE = PF ? NV : 1;
  float pv[NPRE][8], pm[NPRE][8];
  auto fetch_one = [&](int ch, int i, float (&v8)[8], float (&m8)[8]) {
    const int c0 = ch * KC;
#pragma unroll
    for (int j = 0; j < 8; ++j) { v8[j] = 0.f; m8[j] = 1.f; }
    if (sv_in[i]) {
      const float* p = xb + sv_rel[i] + ch * chunk_stride;
      if (vec4) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          if (c0 + 4 * q < Cin) {
            const float4 t4 = *reinterpret_cast<const float4*>(p + 4 * q);
            v8[4 * q] = t4.x; v8[4 * q + 1] = t4.y; v8[4 * q + 2] = t4.z; v8[4 * q + 3] = t4.w;
            if (mb) {
              const float4 m4 = *reinterpret_cast<const float4*>(mb + sv_rel[i] + c0 + 4 * q);
              m8[4 * q] = m4.x; m8[4 * q + 1] = m4.y; m8[4 * q + 2] = m4.z; m8[4 * q + 3] = m4.w;
            }
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (c0 + j < Cin) {
            v8[j] = p[j];
            if (mb) m8[j] = mb[sv_rel[i] + c0 + j];
          }
      }
    }
  };
  auto commit_one = [&](int ch, int i, const float (&v8)[8], const float (&m8)[8], const float (&csc)[8],
                        const float (&csh)[8]) {
    const int c0 = ch * KC;
    const int v = tid + i * BF_TPB;
    if (v < PL) {
      float val[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float t = (m8[j] > 0.f) ? v8[j] : 0.f;              // fused ReLU-backward mask
        t = t * csc[j] + csh[j];                            // identity when scale == NULL
        if (relu_in) t = fmaxf(t, 0.f);
        val[j] = (sv_in[i] && c0 + j < Cin) ? t : 0.f;      // zero padding AFTER the normalisation
      }
      bf16x8 parts[TERMS];
      split8<TERMS>(val, parts);
#pragma unroll
      for (int t = 0; t < TERMS; ++t) sIn[t][v] = parts[t];
    }
  };

  if (PF) {
#pragma unroll
    for (int i = 0; i < NV; ++i) fetch_one(0, i, pv[PF ? i : 0], pm[PF ? i : 0]);
  }
  for (int ch = 0; ch < nchunk; ++ch) {
    // normalisation coefficients of this chunk's 8 channels (wave-uniform)
    float csc[8], csh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool ok = scale && (ch * KC + j < Cin);
      csc[j] = (ok ? scale[n * Cin + ch * KC + j] : 1.f) * sA;
      csh[j] = (ok ? shift[n * Cin + ch * KC + j] : 0.f) * sA;
    }
    // B fragments come straight from L2 through a register ring BD steps deep: a step of the big-layer variant
    // has 48 MFMAs (1536 cycles) of cover, a z-paired step only 12, so it looks 4 steps ahead
    // (measured for NT = 2 on f16x3: depth 4 is 1 % faster than 2, depth 6 is 3 % slower).  The ring is filled
    // BEFORE the staging phase (its registers are idle there), so the first MFMA of the chunk does not wait for L2.
    const bf16x8* wc = wp + (long long)ch * TERMS * NST * 2 * CoutP + boff;
    constexpr int BD = NT == 4 ? 1 : NT == 3 ? 2 : (ZP ? 4 : (TERMS == 2 ? 4 : (NT == 1 ? 2 : 1))) / ZT;
    constexpr int BPRE = BD >= 2 ? BD / 2 : BD;      // slots filled ahead of the staging (all of them would spill)
    bf16x8 bq[BD][NT][TERMS];
#pragma unroll
    for (int d = 0; d < BPRE; ++d)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < TERMS; ++q) bq[d][t][q] = wc[(q * NST + d) * 2 * CoutP + 32 * t];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (!PF) fetch_one(ch, i, pv[0], pm[0]);
      commit_one(ch, i, pv[PF ? i : 0], pm[PF ? i : 0], csc, csh);
    }
    __syncthreads();
    if (PF && ch + 1 < nchunk) {
#pragma unroll
      for (int i = 0; i < NV; ++i) fetch_one(ch + 1, i, pv[PF ? i : 0], pm[PF ? i : 0]);
    }
#pragma unroll
    for (int d = BPRE; d < BD; ++d)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < TERMS; ++q) bq[d][t][q] = wc[(q * NST + d) * 2 * CoutP + 32 * t];
    // ---- 14 tap-pair steps, fully unrolled (tap offsets are compile-time constants per lane half)
#pragma unroll
    for (int s = 0; s < NST; ++s) {
      bf16x8 b[NT][TERMS];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < TERMS; ++q) b[t][q] = bq[s % BD][t][q];
      if (s + BD < NST) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int q = 0; q < TERMS; ++q) bq[s % BD][t][q] = wc[(q * NST + s + BD) * 2 * CoutP + 32 * t];
      }
      constexpr int last_tap = ZP ? 35 : 26;
      const int tapA = 2 * s, tapB = (2 * s + 1 > last_tap) ? last_tap : 2 * s + 1;   // padded half-step: zero weights
      const int offA = ((tapA / 9) * HY + (tapA / 3) % 3) * HX + tapA % 3;
      const int offB = ((tapB / 9) * HY + (tapB / 3) % 3) * HX + tapB % 3;
      const int abase = vrow + (lh ? offB : offA);
#pragma unroll
      for (int p = 0; p < ZT; ++p) {     // the z-pairs of the brick share the B fragments of the step
        bf16x8 a[MR][TERMS];
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
          for (int q = 0; q < TERMS; ++q) a[m][q] = sIn[q][abase + p * (2 * HY * HX) + m * HX];
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            // smallest terms first
            if (TERMS == 3) {
              acc[p][m][t] = mfma16<TERMS>(a[m][2], b[t][0], acc[p][m][t]);
              acc[p][m][t] = mfma16<TERMS>(a[m][1], b[t][1], acc[p][m][t]);
              acc[p][m][t] = mfma16<TERMS>(a[m][0], b[t][2], acc[p][m][t]);
            }
            acc[p][m][t] = mfma16<TERMS>(a[m][1], b[t][0], acc[p][m][t]);
            acc[p][m][t] = mfma16<TERMS>(a[m][0], b[t][1], acc[p][m][t]);
            acc[p][m][t] = mfma16<TERMS>(a[m][0], b[t][0], acc[p][m][t]);
          }
      }
    }
  }
  // ---- epilogue (identical to the fp32 kernel): col = lane&31 (channel), row = voxel along x
  // GroupNorm statistics of the OUTPUT (the next layer's normalisation) ride in the epilogue: per-lane fp32 sums
  // of <= 64 values, then fp64 across the lanes / waves that share a channel, one (sum, sum^2) pair per brick.
  float st1[NT], st2[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) st1[t] = st2[t] = 0.f;
  const long long sbrick = ((long long)n * tiles_z * tiles_y * tiles_x + ((long long)bz * tiles_y + by) * tiles_x + bx);
  if (ZP) {
    const int co = li & 15;                            // column = (channel, output plane)
#pragma unroll
    for (int p = 0; p < ZT; ++p) {
      const int gz = z0 + 2 * p + (li >> 4);
      if (gz < D && co < Cout) {
        const float bv = bias ? bias[co] : 0.f;
#pragma unroll
        for (int m = 0; m < MR; ++m) {
          const int gy = y0 + wy + m;
          if (gy >= H) continue;
          float* yp = y + ((((long long)n * D + gz) * H + gy) * W) * Cout + co;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int gx = x0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (gx < W) {
              float v = acc[p][m][0][r] * desc + bv;
              if (relu_out) v = fmaxf(v, 0.f);
              yp[(long long)gx * Cout] = v;
              st1[0] += v; st2[0] += v * v;
            }
          }
        }
      }
    }
    if (stats_partial) {
      double d1 = (double)st1[0], d2 = (double)st2[0];
      d1 += __shfl_xor(d1, 16); d2 += __shfl_xor(d2, 16);
      d1 += __shfl_xor(d1, 32); d2 += __shfl_xor(d2, 32);
      __syncthreads();                                   // every wave is done with the LDS images
      double* sred = reinterpret_cast<double*>(&sIn[0][0]);
      if (lane < 16) { sred[(wv * 16 + lane) * 2] = d1; sred[(wv * 16 + lane) * 2 + 1] = d2; }
      __syncthreads();
      if (tid < 32 && (tid >> 1) < Cout) {
        const int c = tid >> 1, k = tid & 1;
        stats_partial[(sbrick * Cout + c) * 2 + k] =
            (sred[(0 * 16 + c) * 2 + k] + sred[(1 * 16 + c) * 2 + k]) + (sred[(2 * 16 + c) * 2 + k] + sred[(3 * 16 + c) * 2 + k]);
      }
    }
    return;
  }
#pragma unroll
  for (int p = 0; p < ZT; ++p) {
    const int gz = z0 + 2 * p + wz;
    if (gz >= D) continue;
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const int gy = y0 + wy + m;
      if (gy >= H) continue;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int co = co0 + 32 * t + li;
        if (co >= Cout) continue;
        const float bv = bias ? bias[co] : 0.f;
        const long long rowoff = ((((long long)n * D + gz) * H + gy) * W) * Cout + co;
        float* yp = y + rowoff;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int gx = x0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (gx < W) {
            float v = acc[p][m][t][r] * desc + bv;
            if (addend) v += addend[rowoff + (long long)gx * Cout];
            if (relu_out) v = fmaxf(v, 0.f);
            yp[(long long)gx * Cout] = v;
            st1[t] += v; st2[t] += v * v;
          }
        }
      }
    }
  }
  if (stats_partial) {
    __syncthreads();                                     // every wave is done with the LDS images
    double* sred = reinterpret_cast<double*>(&sIn[0][0]);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      double d1 = (double)st1[t], d2 = (double)st2[t];
      d1 += __shfl_xor(d1, 32); d2 += __shfl_xor(d2, 32);
      if (lh == 0) { sred[((wv * NT + t) * 32 + li) * 2] = d1; sred[((wv * NT + t) * 32 + li) * 2 + 1] = d2; }
    }
    __syncthreads();
    if (tid < 64 * NT) {
      const int k = tid & 1, c = tid >> 1;               // c = t * 32 + li
      const int co = co0 + c;
      if (co < Cout)
        stats_partial[(sbrick * Cout + co) * 2 + k] = (sred[((0 * NT) * 32 + c) * 2 + k] + sred[((1 * NT) * 32 + c) * 2 + k]) +
                                                      (sred[((2 * NT) * 32 + c) * 2 + k] + sred[((3 * NT) * 32 + c) * 2 + k]);
    }
  }
}

// =============================================================================================
// conv3_fwd_g_kernel -- the same implicit GEMM with the staging taken off the critical path (round 2).
// What bounded conv3_fwd_bf_kernel was its staging: per chunk every thread ran six serial load -> wait -> normalise ->
// split -> ds_write chains through registers, 0.7 of an MFMA phase long, while the matrix pipe idled (SQ: 46 % busy).
// Here ONE persistent 512-thread workgroup per CU walks a list of 32 x 8 x 4 output bricks (halo 34 x 10 x 6 = 2040
// voxels) as one pipeline of (brick, 8-channel chunk) stages:
//   * the raw fp32 halo of the NEXT stage -- the next chunk, or chunk 0 of the next brick -- is copied HBM -> LDS by
//     global_load_lds_dwordx4 (16 bytes per lane, no staging registers, no VALU) while the MFMAs of this stage run, so
//     neither a chunk nor a brick starts with an exposed HBM round trip, and a brick's output stores drain under the
//     next brick's first chunk;
//   * a short LDS -> LDS conversion phase (GroupNorm scale/shift, ReLU, zero padding, range scale, fp16 hi/lo split: the
//     same arithmetic, so results are bit-identical to conv3_fwd_bf_kernel) turns it into the two fragment images;
//   * eight waves = 4 output planes x 2 row halves, 4 rows x NT cout tiles each (128 accumulator registers for NT = 2):
//     two waves per SIMD keep the matrix pipe fed, every B fragment is reused by 4 rows, the halo re-read factor is
//     1.99 instead of 2.66.  ZP (Cout <= 16, z-paired weights): waves = 2 plane pairs x 4 row quarters, the N tile is
//     (16 couts x 2 planes) over the pair's 4-plane input window, 18 tap-pair steps.
// LDS: raw stage 2040 x 32 B + two fragment images 2040 x 16 B (reused as 8 x 8 KB epilogue tiles) + the DMA offset
// table 16 KB = 147 200 B.
constexpr int GTY = 8, GTZ = 4;
constexpr int GHY = GTY + 2, GHZ = GTZ + 2, GPL = HX * GHY * GHZ;      // 2040 halo voxels
constexpr int G_TPB = 512;
constexpr int G_SLOTS = 2 * GPL;                                       // 16-byte slots of the raw stage
constexpr int G_AUX = 0;     // (nt, aux = 2, measured 12 % slower: neighbouring bricks share halo lines through L2)
constexpr int G_NLD = (G_SLOTS + G_TPB - 1) / G_TPB;                   // 8 LDS-DMA instructions per thread and chunk
constexpr int G_NCV = (GPL + G_TPB - 1) / G_TPB;                       // 4 voxels converted per thread and chunk
constexpr int G_OFF_BYTES = G_NLD * G_TPB * 4;                         // the DMA source offsets live in LDS, not in VGPRs
constexpr int G_IMG_BYTES = 8 * 32 * 64 * 4;                           // fragment images (65 280 B) / epilogue tiles (8 x 8 KB)
constexpr int G_LDS_BYTES = G_SLOTS * 16 + G_IMG_BYTES + G_OFF_BYTES;  // 65 280 + 65 536 + 16 384 = 147 200


// POOL (NT = 1, not z-paired: 16 < Cout <= 32): the epilogue applies MaxPool3d(2) (floor mode, ATen's first-max rule)
// to the brick it just computed -- a 32 x 8 x 4 brick at an even origin holds 16 x 4 x 2 whole windows -- and writes
// ONLY the pooled tensor (N, D/2, H/2, W/2, Cout), the winners' window indices (1 byte per pooled element, the format of
// kmh_maxpool3d_fwd) and the pooled tensor's (sum, sum^2) statistics: the full-resolution output of an encoder block that
// feeds nothing but the next level's pooling is never written (8.6 GB per step at 256^3) nor re-read by a pooling pass.
template <int NT, bool ZP, bool POOL = false>
__global__ __launch_bounds__(G_TPB, 2) void conv3_fwd_g_kernel(
    const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
    const bf16x8* __restrict__ wp, const float* __restrict__ bias, float* __restrict__ y, int D, int H, int W, int Cin,
    int Cout, int CoutP, int relu_in, int relu_out, int tiles_x, int tiles_y, int tiles_z, int tiles_zp,
    const float* __restrict__ ascale, const float* __restrict__ wscale, double* __restrict__ stats_partial,
    int in_blocked, const float* __restrict__ addend, int total_items, int N, long long* __restrict__ trace,
    unsigned* __restrict__ pool_arg = nullptr) {
  static_assert(!POOL || (NT == 1 && !ZP), "the pooling epilogue is built for the 32-wide tile");
  constexpr int TERMS = 2, MR = ZP ? 2 : 4;
  constexpr int NST = ZP ? NSTEP_Z : NSTEP;
  static_assert(!ZP || NT == 1, "z-paired tiles are for Cout <= 16");
  extern __shared__ __attribute__((aligned(16))) unsigned char gsm[];
  float4* sRaw = reinterpret_cast<float4*>(gsm);                        // [GPL][2]: 8 fp32 channels per halo voxel
  bf16x8* sIn = reinterpret_cast<bf16x8*>(gsm + G_SLOTS * 16);          // [TERMS][GPL]
  int* sOff = reinterpret_cast<int*>(gsm + G_SLOTS * 16 + G_IMG_BYTES);     // [G_NLD][512] DMA source offsets (elements)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);     // wave-uniform by construction: keep it (and wz, wy, the
  const int li = lane & 31, lh = lane >> 5;                    // DMA's LDS bases, the per-wave step tests) in SGPRs
  const int ncog = ZP ? 1 : (Cout + 32 * NT - 1) / (32 * NT);
  const int tyz = (tiles_y + 7) >> 3;
  // work list of this workgroup: virtual block ids blockIdx.x, + gridDim.x, ... of a launch with N * total_items
  // blocks (sample-major), mapped like conv3_fwd_bf_kernel maps its blocks (cout groups adjacent, 8 x 8 (y, z) brick
  // patches per XCD; gridDim.x is a multiple of 8, so every id of the list lands on this workgroup's XCD).  The
  // workgroups of an XCD thus work on ~32 consecutive bricks of ONE sample at a time and share their halos through its
  // L2 (per-sample work lists, 8 consecutive bricks per XCD and sample, fetched 32 % more: PMC r2f vs r2c).
  struct Item { int n, cog, bx, by, bz; };
  const int total_all = N * total_items;
  auto decode = [&](int vb, Item& it) -> bool {
    const int gitem = xcd_remap(vb, total_all);
    it.n = gitem / total_items;
    const int item = gitem - it.n * total_items;
    it.cog = item % ncog;
    const int brick = item / ncog;
    const int lz8 = brick & 7, ly8 = (brick >> 3) & 7, patch = brick >> 6;
    const int pyi = patch % tyz, rest = patch / tyz;
    const int pzi = rest % tiles_zp;
    it.bx = rest / tiles_zp; it.by = pyi * 8 + ly8; it.bz = pzi * 8 + lz8;
    return it.by < tiles_y && it.bz < tiles_z;             // patches are padded to 8 x 8
  };
  auto next_item = [&](int& vb, Item& it) -> bool {        // advance to the next real brick of the list
    for (vb += gridDim.x; vb < total_all; vb += gridDim.x)
      if (decode(vb, it)) return true;
    return false;
  };
  int vb = (int)blockIdx.x - (int)gridDim.x;
  Item cur, nxt;
  if (!next_item(vb, cur)) return;

  const int wz = ZP ? 2 * (wv >> 2) : wv >> 1;             // first output plane of the wave
  const int wy = ZP ? (wv & 3) * MR : (wv & 1) * MR;
  const float sA = ascale ? ascale[0] : 1.f;
  const float desc = (ascale ? ascale[1] : 1.f) * (wscale ? wscale[1] : 1.f);
  const int nchunk = Cin / KC;
  const int vrow = (wz * GHY + wy) * HX + li;
  const long long vox = (long long)D * H * W;
  const long long chunk_stride = in_blocked ? vox * KC : KC;
  auto sample_base = [&](int n) { return in_blocked ? x + (long long)n * nchunk * vox * KC : x + (long long)n * vox * Cin; };

  // LDS-DMA descriptors of a brick: 16-byte slot e = r * 512 + tid holds half (e & 1) of halo voxel e >> 1; padding
  // voxels fetch the clamped in-volume voxel (any valid address: the conversion writes zeros for them)
  auto fill_offsets = [&](const Item& it) {
    const int x0 = it.bx * TX, y0 = it.by * GTY, z0 = it.bz * GTZ;
    int t_ = tid;                     // opaque: the 24 halo coordinates of this thread's slots are recomputed per brick
    asm volatile("" : "+v"(t_));      // instead of living in (spilled) registers across the whole pipeline
#pragma unroll
    for (int r = 0; r < G_NLD; ++r) {
      const int e = r * G_TPB + t_, v = (e >> 1) < GPL ? (e >> 1) : GPL - 1;
      const int lx = v % HX, ly = (v / HX) % GHY, lz = v / (HX * GHY);
      int gx = x0 + lx - 1, gy = y0 + ly - 1, gz = z0 + lz - 1;
      gx = gx < 0 ? 0 : (gx > W - 1 ? W - 1 : gx);
      gy = gy < 0 ? 0 : (gy > H - 1 ? H - 1 : gy);
      gz = gz < 0 ? 0 : (gz > D - 1 ? D - 1 : gz);
      sOff[e] = ((gz * H + gy) * W + gx) * (in_blocked ? KC : Cin) + 4 * (e & 1);      // read back by this thread only
    }
  };
  auto inside_bits = [&](const Item& it) -> unsigned {     // bit i: voxel tid + 512 i of the halo is inside the volume
    const int x0 = it.bx * TX, y0 = it.by * GTY, z0 = it.bz * GTZ;
    unsigned bits = 0;
    int t_ = tid;
    asm volatile("" : "+v"(t_));
#pragma unroll
    for (int i = 0; i < G_NCV; ++i) {
      const int v = t_ + i * G_TPB;
      const int lx = v % HX, ly = (v / HX) % GHY, lz = v / (HX * GHY);
      const int gx = x0 + lx - 1, gy = y0 + ly - 1, gz = z0 + lz - 1;
      const bool in = (v < GPL) && ((unsigned)gx < (unsigned)W) && ((unsigned)gy < (unsigned)H) && ((unsigned)gz < (unsigned)D);
      bits |= (in ? 1u : 0u) << i;
    }
    return bits;
  };
  auto dma_chunk = [&](int n, int ch) {             // this wave's 8 KB of a chunk's halo (offsets of the brick in sOff)
    const float* base = sample_base(n) + ch * chunk_stride;
#pragma unroll
    for (int r = 0; r < G_NLD; ++r) {
      if (r * G_TPB + tid < G_SLOTS)
        __builtin_amdgcn_global_load_lds((kmh_glb_ptr)(base + sOff[r * G_TPB + tid]),
                                         (kmh_lds_ptr)(sRaw + r * G_TPB + wv * 64), 16, 0, G_AUX);
    }
  };

  // ---- B fragments straight from L2 through a register ring BD tap-pair steps deep.  Measured facts that shape the loop:
  //   * loads and LDS-DMA of one wave share ONE vmcnt queue, and hipcc drains it completely at every use of a loaded
  //     register while a DMA is in flight: the B loads are therefore inline asm with hand-counted waits;
  //   * a count may only rely on the order of the B loads among themselves (an LDS-DMA can complete before an older
  //     load: counting DMAs as "younger, still in flight" gave wrong results): "vmcnt(number of B loads issued after
  //     the needed one)" is exact without a DMA in flight and merely stricter with one;
  //   * each wave issues its share of a DMA (8 x 1 KB) in ONE step, wave w in step w: its own next B loads queue
  //     behind 8 KB only, the two waves of a SIMD never stall in the same step, and the last piece has 6+ steps to land;
  //   * SQ counters put the matrix pipe at 55 % busy at an effective 1.93 GHz for the first (non-persistent) version of
  //     this kernel (46 % for conv3_fwd_bf_kernel), i.e. 1.12 PF of fp16 MFMA under the power cap.
  constexpr int BD = 4;
  constexpr int BL = 2 * NT;                                         // B loads per step
  const long long step_stride = 2ll * CoutP, term_stride = (long long)NST * step_stride;
  bf16x8 bq[BD][NT][TERMS];
  long long o0 = 0;
  auto b_issue = [&](int slot) {
    const bf16x8* p0 = wp + o0;
    const bf16x8* p1 = p0 + term_stride;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(bq[slot][0][0]) : "v"(p0) : "memory");
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(bq[slot][0][1]) : "v"(p1) : "memory");
    if (NT == 2) {
      asm volatile("global_load_dwordx4 %0, %1, off offset:512" : "=v"(bq[slot][NT - 1][0]) : "v"(p0) : "memory");
      asm volatile("global_load_dwordx4 %0, %1, off offset:512" : "=v"(bq[slot][NT - 1][1]) : "v"(p1) : "memory");
    }
    o0 += step_stride;
  };

  // static priority for the second-dispatched half: the two waves of a SIMD (w, w + 4) are arbitrated by priority, then
  // AGE, and at equal priority the older wave finished every chunk ~7k cycles ahead of its partner and idled at the
  // barrier (cycle stamps, KMH_G_TRACE); MI355X_MICROARCH.md "Two waves per SIMD", item 4
  if (wv >= 4) __builtin_amdgcn_s_setprio(1);
  fill_offsets(cur);
  dma_chunk(cur.n, 0);
  unsigned cv_in = inside_bits(cur);
  int tr_n = 0;                                            // KMH_G_TRACE: s_memtime stamps of workgroup 0, wave 0
  auto stamp = [&]() {
    if (trace && blockIdx.x == 0 && tid == 0 && tr_n < 240) trace[tr_n++] = __builtin_readcyclecounter();
  };
  for (;;) {
    stamp();                                               // brick start
    const bool more = next_item(vb, nxt);
    const int co0 = cur.cog * (32 * NT);
    const int n = cur.n;
    const int boff = lh * CoutP + co0 + li;
    f32x16 acc[MR][NT];
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][t][r] = 0.f;

    for (int ch = 0; ch < nchunk; ++ch) {
      float csc[8], csh[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        csc[j] = (scale ? scale[n * Cin + ch * KC + j] : 1.f) * sA;
        csh[j] = (scale ? shift[n * Cin + ch * KC + j] : 0.f) * sA;
      }
      // this wave's DMAs of the stage have landed (and its output stores of the previous brick have drained); after the
      // barrier everybody's have -- and every wave is done with the MFMAs of the previous stage: the fragment images
      // may be overwritten
      stamp();                                             // chunk top
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      stamp();                                             // own DMA landed / stores drained
      __builtin_amdgcn_s_barrier();
      stamp();                                             // barrier 1 passed
      // first BD steps of B fragments: in flight during the conversion
      o0 = (long long)ch * TERMS * term_stride + boff;
#pragma unroll
      for (int d = 0; d < BD; ++d) b_issue(d);
#pragma unroll
      for (int i = 0; i < G_NCV; ++i) {
        const int v = tid + i * G_TPB;
        if (v < GPL) {
          const float4 r0 = sRaw[2 * v], r1 = sRaw[2 * v + 1];
          const float raw[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
          const bool in = (cv_in >> i) & 1u;
          float val[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float t = raw[j] * csc[j] + csh[j];
            if (relu_in) t = fmaxf(t, 0.f);
            val[j] = in ? t : 0.f;                         // zero padding AFTER the normalisation
          }
          bf16x8 parts[TERMS];
          split8<TERMS>(val, parts);
#pragma unroll
          for (int t = 0; t < TERMS; ++t) sIn[t * GPL + v] = parts[t];
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      stamp();                                             // conversion done
      __builtin_amdgcn_s_barrier();      // the fragment images are complete; the raw stage may be overwritten
      stamp();                                             // barrier 2 passed
      // the next stage's halo: the next chunk of this brick, or chunk 0 of the next brick (whose offsets replace this
      // brick's in the table: every DMA of this brick has been issued by now)
      const bool last_ch = ch + 1 == nchunk;
      const bool have_next = !last_ch || more;
      if (last_ch && more) fill_offsets(nxt);
      // (opaque copies: keep the per-step fragment addresses from being hoisted out of the loops into 14 + 14 VGPRs)
      int vr = vrow, lhv = lh;
      asm volatile("" : "+v"(vr), "+v"(lhv));
      // (Reading the A fragments of step s+1 into a second register set at the start of step s was measured and dropped:
      // NT = 2: 4 % slower (and 11 spilled registers); NT = 1 / z-paired tiles, 12 / 6 MFMAs per wave and step: the
      // tap-pair phase went from 14.5-17k to 16-18k cycles (KMH_G_TRACE).  hipcc's own placement -- each ds_read a few
      // MFMAs ahead of its first use -- stays.)
#pragma unroll
      for (int s = 0; s < NST; ++s) {
        if (s < 8 && s == wv && have_next) dma_chunk(last_ch ? nxt.n : n, last_ch ? 0 : ch + 1);
        {   // this step's B fragments: leave only the B loads issued after them in flight
          const int ahead = (s + BD - 1 < NST - 1 ? s + BD - 1 : NST - 1) - s;      // steps already issued beyond s
          switch (ahead * BL) {
            case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
            case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
            case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
            case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
            case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
            case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
            default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        constexpr int last_tap = ZP ? 35 : 26;
        const int tapA = 2 * s, tapB = (2 * s + 1 > last_tap) ? last_tap : 2 * s + 1;      // padded half-step: zero weights
        const int offA = ((tapA / 9) * GHY + (tapA / 3) % 3) * HX + tapA % 3;
        const int offB = ((tapB / 9) * GHY + (tapB / 3) % 3) * HX + tapB % 3;
        const int abase = vr + (lhv ? offB : offA);
        bf16x8 a[MR][TERMS];
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
          for (int q = 0; q < TERMS; ++q) a[m][q] = sIn[q * GPL + abase + m * HX];
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            acc[m][t] = mfma16<TERMS>(a[m][1], bq[s % BD][t][0], acc[m][t]);      // smallest terms first, as conv3_fwd_bf_kernel
            acc[m][t] = mfma16<TERMS>(a[m][0], bq[s % BD][t][1], acc[m][t]);
            acc[m][t] = mfma16<TERMS>(a[m][0], bq[s % BD][t][0], acc[m][t]);
          }
        __builtin_amdgcn_sched_barrier(0);
        if (s + BD < NST) b_issue(s % BD);     // refill the slot just consumed
        __builtin_amdgcn_sched_barrier(0);
      }
      stamp();                                             // steps done
    }

    // ---- epilogue of the brick (the stores drain under the next brick's first stage).  The accumulators hold one
    // CHANNEL per lane (32 consecutive channels of a voxel across 32 lanes): stored as they are that is 128 four-byte
    // store instructions per lane and brick, which cost 56k cycles per brick -- two whole chunks (cycle stamps: the
    // store path is issue-bound, MI355X_MICROARCH.md "epilogue store tail").  So every wave transposes its tile row by
    // row through its own 8 KB of the (now idle) fragment-image region and stores 16 bytes per lane: 4x fewer
    // instructions, whole 64-byte channel runs per 4 lanes.
    const int x0 = cur.bx * TX, y0 = cur.by * GTY, z0 = cur.bz * GTZ;
    constexpr int CH = 32 * NT;                                // columns of the wave's tile
    constexpr int L4 = CH / 4;                                 // lanes per voxel in the transposed view (8 or 16)
    constexpr int VPI = 64 / L4;                               // voxels per read instruction (8 or 4)
    const long long sbrick = ((long long)n * tiles_z * tiles_y * tiles_x + ((long long)cur.bz * tiles_y + cur.by) * tiles_x + cur.bx);
    float* tile = reinterpret_cast<float*>(sIn) + wv * (32 * CH);
    const int c4 = lane % L4, vx = lane / L4;                  // this lane's column quad and first voxel in the view
    const int col = 4 * c4;
    const int pl = ZP ? col >> 4 : 0;                          // ZP: column = (channel, output plane of the pair)
    const int co = ZP ? (col & 15) : co0 + col;
    const bool co_ok = co < Cout;                              // Cout % 4 == 0 (launcher)
    float4 bv = {0.f, 0.f, 0.f, 0.f};
    if (bias && co_ok) bv = *reinterpret_cast<const float4*>(bias + co);
    float st1[4] = {0.f, 0.f, 0.f, 0.f}, st2[4] = {0.f, 0.f, 0.f, 0.f};
    __syncthreads();                                           // every wave is done with the fragment images
    const int gz = z0 + wz + pl;
    if constexpr (POOL) {
      // lane = (channel quad c4, x-pair group j): the wave's row tile is read back as voxel PAIRS (2 j + 16 kk, + 1), so
      // the x children of a window meet in one lane, its y children in consecutive rows of this wave, and its z
      // children in the wave two up (same rows, next plane): odd planes hand their (x, y)-pooled partials over through
      // LDS.  Scan order of the reference (z, y, x; a later value wins only if strictly greater, or NaN) is kept by
      // combining lower-index halves first.
      const int j = lane >> 3;
      float4 pm[2][2];
      unsigned pa[2][2];
      auto pick = [](float a, float b, unsigned ca, unsigned cb, float& m_, unsigned& c_) {
        const bool tb = (b > a) || (b != b);
        m_ = tb ? b : a; c_ = tb ? cb : ca;
      };
#pragma unroll
      for (int m = 0; m < MR; ++m) {
#pragma unroll
        for (int r = 0; r < 16; ++r) tile[((r & 3) + 8 * (r >> 2) + 4 * lh) * CH + li] = acc[m][0][r];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int xe = 2 * j + 16 * kk;
          const float4 a = *reinterpret_cast<const float4*>(tile + xe * CH + col);
          const float4 b = *reinterpret_cast<const float4*>(tile + (xe + 1) * CH + col);
          float va[4] = {a.x * desc + bv.x, a.y * desc + bv.y, a.z * desc + bv.z, a.w * desc + bv.w};
          float vb[4] = {b.x * desc + bv.x, b.y * desc + bv.y, b.z * desc + bv.z, b.w * desc + bv.w};
          float mx[4];
          unsigned cx[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (relu_out) { va[q] = fmaxf(va[q], 0.f); vb[q] = fmaxf(vb[q], 0.f); }
            pick(va[q], vb[q], 0u, 1u, mx[q], cx[q]);                      // x children: codes 0 / 1
          }
          if ((m & 1) == 0) {
            pm[m >> 1][kk] = float4{mx[0], mx[1], mx[2], mx[3]};
            pa[m >> 1][kk] = cx[0] | (cx[1] << 8) | (cx[2] << 16) | (cx[3] << 24);
          } else {                                                         // y children: + 2 for the second row
            float4& P = pm[m >> 1][kk];
            const unsigned A = pa[m >> 1][kk];
            float o0, o1, o2, o3;
            unsigned c0, c1, c2, c3;
            pick(P.x, mx[0], A & 255u, cx[0] + 2u, o0, c0);
            pick(P.y, mx[1], (A >> 8) & 255u, cx[1] + 2u, o1, c1);
            pick(P.z, mx[2], (A >> 16) & 255u, cx[2] + 2u, o2, c2);
            pick(P.w, mx[3], A >> 24, cx[3] + 2u, o3, c3);
            P = float4{o0, o1, o2, o3};
            pa[m >> 1][kk] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
          }
        }
      }
      // z children: waves 2, 3, 6, 7 (odd planes) publish, waves 0, 1, 4, 5 (even planes) combine and store
      float4* xv = reinterpret_cast<float4*>(reinterpret_cast<unsigned char*>(sIn) + 8 * (32 * CH * 4));   // behind the 8 tiles
      unsigned* xa = reinterpret_cast<unsigned*>(xv + 4 * 4 * 64);
      const bool odd_plane = (wz & 1) != 0;
      const int slot = ((wv >> 2) * 2 + (wv & 1)) * 4 * 64;              // (plane pair, row half)
      if (odd_plane) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) { xv[slot + (2 * p + kk) * 64 + lane] = pm[p][kk]; xa[slot + (2 * p + kk) * 64 + lane] = pa[p][kk]; }
      }
      __syncthreads();
      if (!odd_plane) {
        const int Do = D >> 1, Ho = H >> 1, Wo = W >> 1;
        const int oz = (z0 + wz) >> 1;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const int oy = (y0 + wy + 2 * p) >> 1;
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const int ox = (x0 >> 1) + j + 8 * kk;
            const float4 Q = xv[slot + (2 * p + kk) * 64 + lane];
            const unsigned B = xa[slot + (2 * p + kk) * 64 + lane];
            const float4 P = pm[p][kk];
            const unsigned A = pa[p][kk];
            float o0, o1, o2, o3;
            unsigned c0, c1, c2, c3;
            pick(P.x, Q.x, A & 255u, (B & 255u) + 4u, o0, c0);
            pick(P.y, Q.y, (A >> 8) & 255u, ((B >> 8) & 255u) + 4u, o1, c1);
            pick(P.z, Q.z, (A >> 16) & 255u, ((B >> 16) & 255u) + 4u, o2, c2);
            pick(P.w, Q.w, A >> 24, (B >> 24) + 4u, o3, c3);
            if (oz < Do && oy < Ho && ox < Wo && co_ok) {
              const long long e = ((((long long)n * Do + oz) * Ho + oy) * Wo + ox) * Cout + co;
              *reinterpret_cast<float4*>(y + e) = float4{o0, o1, o2, o3};
              pool_arg[e >> 2] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
              st1[0] += o0; st2[0] += o0 * o0; st1[1] += o1; st2[1] += o1 * o1;
              st1[2] += o2; st2[2] += o2 * o2; st1[3] += o3; st2[3] += o3 * o3;
            }
          }
        }
      }
    } else {
#pragma unroll
    for (int m = 0; m < MR; ++m) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) tile[((r & 3) + 8 * (r >> 2) + 4 * lh) * CH + 32 * t + li] = acc[m][t][r];
      const int gy = y0 + wy + m;
      const bool row_ok = gz < D && gy < H && co_ok;
      const long long rowoff = ((((long long)n * D + gz) * H + gy) * W) * Cout + co;
      float4 v4[32 / VPI], ad[32 / VPI];
#pragma unroll
      for (int k = 0; k < 32 / VPI; ++k) {
        const int xx = vx + VPI * k;
        v4[k] = *reinterpret_cast<const float4*>(tile + xx * CH + col);
        ad[k] = float4{0.f, 0.f, 0.f, 0.f};
        if (addend && row_ok && x0 + xx < W) ad[k] = *reinterpret_cast<const float4*>(addend + rowoff + (long long)(x0 + xx) * Cout);
      }
#pragma unroll
      for (int k = 0; k < 32 / VPI; ++k) {
        const int gx = x0 + vx + VPI * k;
        if (row_ok && gx < W) {
          float4 o;
          o.x = v4[k].x * desc + bv.x + ad[k].x; o.y = v4[k].y * desc + bv.y + ad[k].y;
          o.z = v4[k].z * desc + bv.z + ad[k].z; o.w = v4[k].w * desc + bv.w + ad[k].w;
          if (relu_out) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
          *reinterpret_cast<float4*>(y + rowoff + (long long)gx * Cout) = o;
          st1[0] += o.x; st2[0] += o.x * o.x; st1[1] += o.y; st2[1] += o.y * o.y;
          st1[2] += o.z; st2[2] += o.z * o.z; st1[3] += o.w; st2[3] += o.w * o.w;
        }
      }
    }
    }   // !POOL
    if (stats_partial) {
      // per (wave, column) sums -> LDS -> one (sum, sum^2) pair per channel and brick, fixed order (deterministic)
      double d1[4], d2[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        d1[j] = (double)st1[j]; d2[j] = (double)st2[j];
#pragma unroll
        for (int o = L4; o < 64; o <<= 1) { d1[j] += __shfl_xor(d1[j], o); d2[j] += __shfl_xor(d2[j], o); }
      }
      __syncthreads();                                         // the tiles have been read back
      double* sred = reinterpret_cast<double*>(sIn);           // [wave][CH][2]  (NOT the raw stage: the next halo lands there)
      if (lane < L4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { sred[((wv * CH) + col + j) * 2] = d1[j]; sred[((wv * CH) + col + j) * 2 + 1] = d2[j]; }
      }
      __syncthreads();
      const int ncol = ZP ? 16 : CH;
      if (tid < 2 * ncol) {
        const int k = tid & 1, c = tid >> 1;
        const int cch = ZP ? c : co0 + c;
        if (cch < Cout) {
          double sum = 0.0;
#pragma unroll
          for (int w8 = 0; w8 < 8; ++w8) {
            sum += sred[(w8 * CH + c) * 2 + k];
            if (ZP) sum += sred[(w8 * CH + 16 + c) * 2 + k];   // the second plane of the pair
          }
          stats_partial[(sbrick * Cout + cch) * 2 + k] = sum;
        }
      }
    }
    stamp();                                               // epilogue issued
    if (!more) break;
    cur = nxt;
    cv_in = inside_bits(cur);
  }
}


// =============================================================================================
// conv3_fwd_s_kernel -- ONE wave per SIMD (round 4).  What the cycle stamps of conv3_fwd_g_kernel say: a chunk is
// ~31.3k cycles = tap-pair steps 26.0k (two waves per SIMD share the matrix pipe: 77 cycles per MFMA and wave, 83 % of the
// pipe) + a conversion phase of 4.2k + two barriers, and with two waves per SIMD nothing can be moved into the MFMA shadow:
// their issue streams are zero-sum (MI355X_MICROARCH.md "Two waves per SIMD", item 3; measured here too: DESIGN.md section 8).
// A SINGLE wave per SIMD with the whole register file does hide up to ~5 single-issue instructions per MFMA gap (same
// guide, constants table).  So: 256 threads = 4 waves, wave = one plane of the 32 x 8 x 4 brick = 8 rows x NT cout tiles
// (256 accumulator registers for NT = 2, every B fragment reused by 8 rows), and per step the wave's stream is
//   wait for this step's B fragments | two LDS-DMA pieces of the NEXT stage's halo (steps 0-7) | the A fragments of the
//   NEXT step into a second register set | 48 MFMAs with, from step 8 on, the in-place conversion of the next stage's
//   voxels (the lane's own: it fetched both 16-byte halves itself) scheduled between them | the B loads of step s + 4.
// Two stage buffers of 2 x 2048 16-byte slots (fp32 halves in, fp16 hi / lo planes out, in place), ONE barrier per stage.
// Bit-identical to conv3_fwd_g_kernel / conv3_fwd_bf_kernel: per accumulator the three products keep their order (the loop
// runs term-major over the 16 accumulators, so back-to-back MFMAs never hit the same one).
constexpr int S_TPB = 256, S_MR = 8;
constexpr int S_PLANE = 2048;                                         // 16-byte slots per plane of a stage buffer (>= GPL)
constexpr int S_NLD = 2 * S_PLANE / S_TPB;                            // 16 LDS-DMA instructions per thread and chunk
constexpr int S_NCV = S_PLANE / S_TPB;                                // 8 voxels converted per thread and chunk
constexpr int S_BUF_BYTES = 2 * S_PLANE * 16;                         // 65 536
constexpr int S_OFF_BYTES = S_NLD * S_TPB * 4;                        // 16 384
constexpr int S_COEF = 1024;                                          // channels of one sample's (scale, shift) table
constexpr int S_LDS_BYTES = 2 * S_BUF_BYTES + S_OFF_BYTES + 2 * S_COEF * 4;      // 155 648
static_assert(GPL <= S_PLANE && GTZ == 4 && GTY == S_MR, "wave = plane, 8 rows");
// the step's issue plan, swept and settled:
constexpr int S_ILR = 12, S_ILRN = 2;                                 // gaps that take LDS reads, reads per such gap
constexpr int S_ILV0 = 3, S_ILV1 = 3, S_ILV2 = 2;                     // first gap that takes conversion VALU; VALU per gap on the 32-wide / 64-wide tile
constexpr int SPS_BA = 6;                                             // SPARSE: drains at steps 0, 6, 12; cell c is expanded in steps 6 + 6 c .. + 5
constexpr int SP_BA = 9, SP_PS = 5;                                   // SPLIT: request distance = drain period; the stage's 16 DMA pieces go out in
                                                                      // steps 0 .. SP_PS - 1 (flat over the valid range: profiles/r5g_zp_split_ring_sweep.txt)
// What is still a compile-time switch is built by something: KMH_S_CW=0 KMH_S_DEEP=0 is the library's fall-back when the ISA audit
// fails (keymorph_amd/build.py), KMH_S_DEEP_RING_V=1 KMH_S_IL=0 the audit's positive control (tests/test_asm_audit_cpu.py),
// KMH_S_STAMPALL an instrument.
#ifndef KMH_S_DEEP
#define KMH_S_DEEP 1
#endif
#ifndef KMH_S_CW               // 1 = hand-counted waits in the kernels that convert their operand (0: full drains)
#define KMH_S_CW 1
#endif
#ifndef KMH_S_STAMPALL
#define KMH_S_STAMPALL 0
#endif
#ifndef KMH_S_IL               // 1 = LDS reads / conversion VALU dealt over the MFMA gaps of the whole step (0: reads first)
#define KMH_S_IL 1
#endif
#ifndef KMH_S_DEEP_RING_V      // 1 = the DEEP ring in "=v" registers: the variant that CRASHED (kept as the positive control of
#define KMH_S_DEEP_RING_V 0    // tests/test_asm_audit_cpu.py; never built into the library)
#endif

// ZP (Cout <= 16, z-paired weights, NT = 1): wave = (plane pair, row half) -- 4 rows, the N tile is (16 couts x 2 planes) over the
// pair's 4-plane input window, 18 tap-pair steps of 12 MFMAs (the eight-wave kernel: 6 per wave and step, the most
// overhead-bound launch of the step).
// SPLIT (round 5): the input arrives ALREADY range-scaled and split -- x is (N, Cin/8, V + 1) records of 32 bytes, 8 fp16 hi
// then 8 fp16 lo of one voxel's chunk, record V of every (sample, chunk) plane all zeros (the source of every padding slot) --
// written so by its producer (kmh_maxpool3d_bwd_split: a pooling backward knows its output's range scale before it writes).
// A stage's fragment images are then 16 LDS-DMA pieces per lane (global_load_lds_dwordx4, hi -> plane 0, lo -> plane 1), one
// or two per step, and NO conversion: no staging registers, no VALU, no coefficient table.  What that buys where the
// conversion cannot hide: the z-paired 32 -> 16 data gradient at 256^3 has 18 x 12 MFMAs per chunk (6.9k cycles) against a
// conversion of the same length (cycle stamps, profiles/r5a): 1300-1800 cycles per conversion step against 384 of MFMA time.
// Bit-identical to the fp32 input: the producer applies the same fmaf(x, S, 0) and split8<2>.
// POOL (round 5; NT = 1, not z-paired: 16 < Cout <= 32): the pooling epilogue of conv3_fwd_g_kernel on this kernel's waves -- a
// wave holds four rows of BOTH planes of a plane pair, so the x children of a window meet in one lane's accumulator registers,
// its y children in consecutive rows and its z children in rows m / m + 4 of the same wave: nothing crosses waves; ATen's
// first-max rule, the same winners, the same outputs bit for bit.  What it buys:
// the plain one-wave kernel spends 38 % of a two-chunk 16 -> 32 brick in its epilogue storing 128 KB (cycle stamps, r5a); the
// pooled tensor is 16 KB.
// SPARSE (round 7; with SPLIT, z-paired): the operand is the gradient of a tensor that feeds only a 2 x 2 x 2 max-pool, handed over
// as the POOLED gradient x = (N, D/2, H/2, W/2, Cin) fp32 with its winner bytes (`pool_arg`: one per pooled element, 0..7 =
// (dz, dy, dx)) -- one non-zero per window and channel, so the dense record tensor (7/8 zeros) and the pass that writes it are
// gone.  With even brick origins the 34 x 10 x 6 halo is covered by 18 x 6 x 4 = 432 pooled cells per chunk: a lane owns two
// (lanes 176 .. 255 own one and the 8 slots past the halo).  Per stage it loads each cell's 32 bytes of gradient and 8 winner
// bytes in step 0 (landed by the drain at the head of step BA), forms fmaf(v, S, 0) and split8<2> ONCE per cell, writes zero
// records to the cell's children and then each channel's hi / lo term, 2 bytes each, into the record of the child its winner byte
// names -- six steps per cell from step BA on, dealt over the MFMA gaps.  A child outside the halo (border cells keep >= 1 child inside per axis)
// is redirected to a sibling inside and its value zeroed; so are the children of cells outside the volume.  The winner byte
// enters an address only as (byte & 7) through a per-lane table of the cell's OWN eight record offsets (two v_perm_b32 look-ups
// serve four channels), so no byte value can write outside the cell's records; a byte > 7 cannot come from the pooling kernels.
// Same words in the same slots as SPLIT: bit-identical.  The table (sOff) holds per lane and cell the eight record offsets, the
// validity bytes, the cell's base slot and its global element offset.
template <int NT, bool ZP = false, bool SPLIT = false, bool POOL = false, bool AMP = false, bool SPARSE = false>
__global__ __launch_bounds__(S_TPB, 1) void conv3_fwd_s_kernel(
    const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
    const bf16x8* __restrict__ wp, const float* __restrict__ bias, float* __restrict__ y, int D, int H, int W, int Cin,
    int Cout, int CoutP, int relu_in, int relu_out, int tiles_x, int tiles_y, int tiles_z, int tiles_zp,
    const float* __restrict__ ascale, const float* __restrict__ wscale, double* __restrict__ stats_partial,
    int in_blocked, const float* __restrict__ addend, int total_items, int N, long long* __restrict__ trace,
    unsigned* __restrict__ pool_arg = nullptr) {
  constexpr int TERMS = 2, MR = ZP ? 4 : S_MR, NST = ZP ? NSTEP_Z : NSTEP;
  static_assert(!ZP || NT == 1, "z-paired tiles are for Cout <= 16");
  static_assert(ZP == SPLIT, "the z-paired tile is launched on pre-split operands only (fp32 operands: conv3_fwd_g_kernel<1, true>)");
  static_assert(!POOL || (NT == 1 && !ZP), "the pooling epilogue is built for the 32-wide tile");
  static_assert(!SPARSE || (SPLIT && ZP && !AMP && TX % 2 == 0 && GTY % 2 == 0 && GTZ % 2 == 0), "pooled operand: the pre-split arm, even brick origins");
  extern __shared__ __attribute__((aligned(16))) unsigned char gsm[];
  int* sOff = reinterpret_cast<int*>(gsm + 2 * S_BUF_BYTES);
  float* sCoef = reinterpret_cast<float*>(gsm + 2 * S_BUF_BYTES + S_OFF_BYTES);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int ncog = ZP ? 1 : (Cout + 32 * NT - 1) / (32 * NT);
  const int tyz = (tiles_y + 7) >> 3;
  struct Item { int n, cog, bx, by, bz; };
  const int total_all = N * total_items;
  auto decode = [&](int vb, Item& it) -> bool {      // the work list of conv3_fwd_g_kernel
    const int gitem = xcd_remap(vb, total_all);
    it.n = gitem / total_items;
    const int item = gitem - it.n * total_items;
    it.cog = item % ncog;
    const int brick = item / ncog;
    const int lz8 = brick & 7, ly8 = (brick >> 3) & 7, patch = brick >> 6;
    const int pyi = patch % tyz, rest = patch / tyz;
    const int pzi = rest % tiles_zp;
    it.bx = rest / tiles_zp; it.by = pyi * 8 + ly8; it.bz = pzi * 8 + lz8;
    return it.by < tiles_y && it.bz < tiles_z;
  };
  auto next_item = [&](int& vb, Item& it) -> bool {
    for (vb += gridDim.x; vb < total_all; vb += gridDim.x)
      if (decode(vb, it)) return true;
    return false;
  };
  int vb = (int)blockIdx.x - (int)gridDim.x;
  Item cur, nxt;
  if (!next_item(vb, cur)) return;

  const float sA = ascale ? ascale[0] : 1.f;
  const float desc = (ascale ? ascale[1] : 1.f) * (wscale ? wscale[1] : 1.f);
  const int nchunk = Cin / KC;
  // POOL (round 5): a wave owns rows 4 (wv & 1) .. + 3 of BOTH planes of a plane pair (accumulator rows 0-3 /
  // 4-7) instead of 8 rows of one plane, so the 2 x 2 x 2 pooling window -- x: a register pair, y: two rows, z: rows m / m + 4 --
  // lies inside ONE wave: no exchange through LDS, no idle odd-plane waves, every wave transposes and stores 16 values per lane
  // (- 4.7 % against a plane per wave: profiles/r5z_pool_epilogue_in_wave_z_pooling.txt)
  const int wz = (ZP || POOL) ? 2 * (wv >> 1) : wv, wy = ZP ? (wv & 1) * MR : (POOL ? (wv & 1) * (MR / 2) : 0);      // first output plane / row of the wave
  const int vrow = (wz * GHY + wy) * HX + li;
  auto arow = [](int m) -> int { return POOL ? (m & 3) * HX + (m >> 2) * (GHY * HX) : m * HX; };      // A-image offset of accumulator row m
  const long long vox = (long long)D * H * W;
  const long long plane = SPLIT ? (vox + 1) * KC : vox * KC;      // floats per (sample, chunk) plane of a channel-blocked input
  const long long chunk_stride = (in_blocked || SPLIT) ? plane : KC;
  auto sample_base = [&](int n) {
    return (in_blocked || SPLIT) ? x + (long long)n * nchunk * plane : x + (long long)n * vox * Cin;
  };

  // LDS-DMA descriptors of a brick: 16-byte slot e = r * 256 + tid holds half (r >> 3) of halo voxel (r & 7) * 256 + tid
  auto fill_offsets = [&](const Item& it) -> unsigned {      // -> bit i: voxel tid + 256 i of the halo is inside the volume
    const int x0 = it.bx * TX, y0 = it.by * GTY, z0 = it.bz * GTZ;
    int t_ = tid;
    asm volatile("" : "+v"(t_));
    if constexpr (SPARSE) {
      // per cell c of the lane: row 2 c = the 16-bit byte offsets of its 8 children's records from the cell's base slot (children
      // outside the halo: a sibling's), row 2 c + 1 = {validity bytes of children 0-3, 4-7, base slot (bytes), global element offset}
      typedef unsigned sp_u4 __attribute__((ext_vector_type(4)));
      sp_u4* tab = reinterpret_cast<sp_u4*>(sOff);
      constexpr int CX = HX / 2 + 1, CY = GHY / 2 + 1, CZ = GHZ / 2 + 1;      // 18 x 6 x 4 cells
      static_assert(2 * S_TPB >= CX * CY * CZ && 4 * S_TPB * 16 <= S_OFF_BYTES, "two cells per lane, four table rows");
      const int Wp = W >> 1, Hp = H >> 1, Dp = D >> 1;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int cell = c * S_TPB + t_;
        const bool real = cell < CX * CY * CZ;
        const int cl = real ? cell : 0;
        const int cxl = cl % CX, cyl = (cl / CX) % CY, czl = cl / (CX * CY);
        const int cgx = (x0 >> 1) - 1 + cxl, cgy = (y0 >> 1) - 1 + cyl, cgz = (z0 >> 1) - 1 + czl;
        const bool in = real && ((unsigned)cgx < (unsigned)Wp) && ((unsigned)cgy < (unsigned)Hp) && ((unsigned)cgz < (unsigned)Dp);
        const unsigned goff = in ? (unsigned)(((cgz * Hp + cgy) * Wp + cgx) * Cin) : 0u;
        const bool ex = cxl == 0 || cxl == CX - 1, ey = cyl == 0 || cyl == CY - 1, ez = czl == 0 || czl == CZ - 1;
        const int bx = cxl == 0 ? 0 : 2 * cxl - 1, by = cyl == 0 ? 0 : 2 * cyl - 1, bz = czl == 0 ? 0 : 2 * czl - 1;
        unsigned B = (unsigned)(((bz * GHY + by) * HX + bx) * 16);
        unsigned sx = ex ? 0u : 16u, sy = ey ? 0u : (unsigned)(HX * 16), sz = ez ? 0u : (unsigned)(GHY * HX * 16);
        if (!real) { B = (unsigned)((GPL + (t_ & 7)) * 16); sx = sy = sz = 0u; }      // the slots past the halo: zeros
        unsigned d[8], vl[2] = {0u, 0u};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
          d[k] = dx * sx + dy * sy + dz * sz;
          // the child outside the halo of a border cell: dx = 0 of the first column, dx = 1 of the last one (y, z alike)
          const bool ok = in && !(ex && dx == (cxl == 0 ? 0 : 1)) && !(ey && dy == (cyl == 0 ? 0 : 1)) && !(ez && dz == (czl == 0 ? 0 : 1));
          vl[k >> 2] |= (ok ? 0xffu : 0u) << (8 * (k & 3));
        }
        const sp_u4 r0 = {d[0] | (d[1] << 16), d[2] | (d[3] << 16), d[4] | (d[5] << 16), d[6] | (d[7] << 16)};
        const sp_u4 r1 = {vl[0], vl[1], B, goff};
        tab[(2 * c) * S_TPB + t_] = r0;                     // read back by this thread only
        tab[(2 * c + 1) * S_TPB + t_] = r1;
      }
      return 0u;
    } else if constexpr (SPLIT) {
      // one record offset (floats) per halo voxel of this lane: slot r * 256 + tid; padding voxels and the 8 slots past the
      // halo point at the plane's zero record
#pragma unroll
      for (int r = 0; r < S_NCV; ++r) {
        const int v = r * S_TPB + t_;
        const int lx = v % HX, ly = (v / HX) % GHY, lz = v / (HX * GHY);
        const int gx = x0 + lx - 1, gy = y0 + ly - 1, gz = z0 + lz - 1;
        const bool in = (v < GPL) && ((unsigned)gx < (unsigned)W) && ((unsigned)gy < (unsigned)H) && ((unsigned)gz < (unsigned)D);
        sOff[r * S_TPB + t_] = in ? ((gz * H + gy) * W + gx) * KC : (int)vox * KC;      // read back by this thread only
      }
      return 0u;
    }
    // ONE coordinate decode per halo voxel of the lane: both 16-byte halves' offsets and the voxel's inside bit (round 5: the
    // table and inside_bits() used to decode the same voxels twice over, ~3k cycles of a brick's last stage and ~2k more
    // after its epilogue)
    unsigned bits = 0;
#pragma unroll
    for (int r = 0; r < S_NCV; ++r) {
      const int v0_ = r * S_TPB + t_, v = v0_ < GPL ? v0_ : GPL - 1;
      const int lx = v % HX, ly = (v / HX) % GHY, lz = v / (HX * GHY);
      int gx = x0 + lx - 1, gy = y0 + ly - 1, gz = z0 + lz - 1;
      const bool in = (v0_ < GPL) && ((unsigned)gx < (unsigned)W) && ((unsigned)gy < (unsigned)H) && ((unsigned)gz < (unsigned)D);
      bits |= (in ? 1u : 0u) << r;
      gx = gx < 0 ? 0 : (gx > W - 1 ? W - 1 : gx);
      gy = gy < 0 ? 0 : (gy > H - 1 ? H - 1 : gy);
      gz = gz < 0 ? 0 : (gz > D - 1 ? D - 1 : gz);
      const int off = ((gz * H + gy) * W + gx) * (in_blocked ? KC : Cin);
      sOff[r * S_TPB + t_] = off;                 // read back by this thread only
      sOff[(8 + r) * S_TPB + t_] = off + 4;
    }
    return bits;
  };
  // the lane's voxel j of the next stage: its two 16-byte halves into a register ring (two voxels: loaded in step j, landed
  // by the drain at the head of step j + 1, converted there).  (LDS-DMA pieces -- no staging registers -- cost this single wave 100+ cycles of issue
  // each, 16 per chunk: steps with two pieces ran 1.8k cycles against the 1.54k of their 48 MFMAs.)
  typedef float kmh_f4 __attribute__((ext_vector_type(4)));      // (a native vector: the asm's "=v" operand)
  // DEEP (round 5, the 32-wide tile without a pre-split operand; KMH_S_DEEP=0: the fall-back build): its 24 MFMAs per step (768 cycles)
  // do not cover an HBM round trip, and a `vmcnt(0)` at every step head made every raw load issued in step s a wait at step
  // s + 1 (conversion steps 1200 cycles against 910 without a conversion).  As for SPLIT, the B ring holds a whole stage (in
  // AGPRs) and fragments are requested 7 steps ahead; the raw voxels are requested THREE steps before their conversion instead
  // of one.  (First with two drains per stage and compiler-visible raw loads: - 1-2 %; then with the counted waits below.)
  constexpr bool DEEP = (NT == 1) && !ZP && !SPLIT && (KMH_S_DEEP != 0);
  // CW (round 5, every kernel that converts its operand): COUNTED waits.  Loads return in issue order, so `vmcnt(K)` with K =
  // the number of loads issued after the one a step needs says exactly "that one has landed" -- and leaves the younger ones in
  // flight: a raw voxel requested CD steps before its conversion gets CD steps of MFMAs to come in from HBM (a full drain at the
  // next step head gave it one: 1.7-1.9k cycles against 0.9k idle and 2-4k loaded HBM latency; the conversion steps of the
  // 64-wide tile ran 2.1-2.6k cycles against 1.93k for plain ones).  The raw loads are inline asm as the fragment loads are
  // (the compiler's own waits for visible loads do not count the asm ones, i.e. wait for too much), every wait is followed by
  // empty asm statements that re-define the registers it covers (so no use can move above it), and tools/scan_asm_inflight.py
  // checks in the ISA that no destination is copied or spilled between its load and the wait that covers it -- the root of
  // round 4's "counted waits give run-to-run different results".  Output stores of an epilogue are OLDER than every load that
  // is waited for with a count (the fragments requested before an epilogue are drained / waited for with vmcnt(0)), so their
  // completion order does not matter: pending stores only make a counted wait stricter.
  constexpr bool CW = !SPLIT && (KMH_S_CW != 0);
  constexpr int CD = DEEP ? 3 : (CW ? 2 : 1);              // steps between a voxel's request and its conversion
  constexpr int RQ = CD + 1;                               // raw ring slots
  kmh_f4 rawq[RQ][2];
  auto raw_issue = [&](int n, int ch, int slot, int off0, int off1) {
    const float* base = sample_base(n) + ch * chunk_stride;
    const float* p0 = base + off0;
    const float* p1 = base + off1;
    if constexpr (CW) {
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(rawq[slot][0]) : "v"(p0) : "memory");
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(rawq[slot][1]) : "v"(p1) : "memory");
    } else {
      // (compiler-visible loads: its own waits for them are merely stricter than needed)
      rawq[slot][0] = *reinterpret_cast<const kmh_f4*>(p0);
      rawq[slot][1] = *reinterpret_cast<const kmh_f4*>(p1);
    }
  };
  auto raw_tie = [&](int slot) {                           // (after a wait: the slot's registers are defined HERE)
    asm volatile("" : "+v"(rawq[slot][0]));
    asm volatile("" : "+v"(rawq[slot][1]));
  };
  auto vm_wait = [](int K) {                               // s_waitcnt vmcnt(K), K a constant after unrolling
    switch (K) {
      case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
      case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
      case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
      case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
      case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
      case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
      case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
      case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
      case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
      default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
  };
  int coef_n = -1;
  auto fill_coef = [&](int n_) {                      // (the caller's barrier publishes it)
    for (int e = tid; e < Cin; e += S_TPB) {
      sCoef[e] = (scale ? scale[n_ * Cin + e] : 1.f) * sA;
      sCoef[S_COEF + e] = (scale ? shift[n_ * Cin + e] : 0.f) * sA;
    }
    coef_n = n_;
  };
  // conversion of the lane's voxel i (raw halves r0, r1 in registers) into the fragment images of stage buffer pb (sample
  // coef_n): branch-free, scheduled INTO a step's MFMA block; slots past the halo hold a clamped voxel's data and become zeros
  const float relu_floor = relu_in ? 0.f : -__builtin_inff();
  auto convert1 = [&](int ch, unsigned bits, int pb, int i, const kmh_f4 r0, const kmh_f4 r1) {
    const float4 a0 = *reinterpret_cast<const float4*>(sCoef + ch * KC), a1 = *reinterpret_cast<const float4*>(sCoef + ch * KC + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(sCoef + S_COEF + ch * KC), b1 = *reinterpret_cast<const float4*>(sCoef + S_COEF + ch * KC + 4);
    const float csc[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    const float csh[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    bf16x8* B8 = reinterpret_cast<bf16x8*>(gsm + pb * S_BUF_BYTES);
    const int v = tid + i * S_TPB;
    const float raw[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    const bool in = (bits >> i) & 1u;
    // ReLU and the zero padding (AFTER the normalisation) as ONE median per value: inside the volume the bounds are
    // (0 or -inf, +inf), outside (0, 0) -- 2 selects + 8 v_med3 per voxel instead of 8 maxima + 16 selects
    const float lo = in ? relu_floor : 0.f, hi = in ? __builtin_inff() : 0.f;
    float val[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) val[j] = __builtin_amdgcn_fmed3f(raw[j] * csc[j] + csh[j], lo, hi);
    bf16x8 parts[TERMS];
    split8<TERMS>(val, parts);
#pragma unroll
    for (int t = 0; t < TERMS; ++t) B8[t * S_PLANE + v] = parts[t];
  };

  // SPLIT: piece p (0..15) of a stage = plane (p & 1) of the lane's voxel p >> 1: 16 bytes per lane straight into the
  // fragment image of stage buffer `buf` (wave-uniform LDS base + 16 x lane), source = the voxel's record (+ 16 bytes for lo)
  auto dma_piece = [&](int n, int ch, int buf, int p, int off) {
    const float* src = sample_base(n) + ch * chunk_stride + off + 4 * (p & 1);
    unsigned char* dst = gsm + buf * S_BUF_BYTES + ((p & 1) * S_PLANE + (p >> 1) * S_TPB + wv * 64) * 16;
    __builtin_amdgcn_global_load_lds((kmh_glb_ptr)src, (kmh_lds_ptr)dst, 16, 0, 0);
  };
  // SPARSE: the loads of a stage's two cells and the four parts of one cell's expansion into stage buffer `buf`, one part per
  // step.  The loads are inline asm like the fragment loads (for compiler-visible ones hipcc adds counted waits of its own that do
  // not count the asm loads queued behind them: vmcnt(1) / vmcnt(0) in the middle of the expansion steps, i.e. a wait for the
  // fragments requested at that step's head); they are consumed behind the FULL drain at the head of step BA, followed by sp_tie
  // (no hand-counted wait), and the ISA audit covers their destinations like every other asm load's.  The 8 winner bytes are a
  // plain load whose first use is sp_tie: the compiler's own wait for it falls on the drain.
  typedef unsigned sp_u4 __attribute__((ext_vector_type(4)));
  const sp_u4* const spTab = reinterpret_cast<const sp_u4*>(sOff);
  kmh_f4 spg[2][2];                                        // [cell][half]: 8 gradient values
  typedef unsigned sp_u2 __attribute__((ext_vector_type(2)));
  sp_u2 spw[2];                                            // [cell]: 8 winner bytes
  unsigned sph[4], spl[4], spP[4], spM[4], spB = 0;        // the cell in expansion: hi / lo words, record offsets, masks (per channel pair)
  auto sp_issue = [&](int n, int ch) {
    const long long cells = vox >> 3;
    const float* gb = x + ((long long)n * cells) * Cin + ch * KC;
    const unsigned char* wb = reinterpret_cast<const unsigned char*>(pool_arg) + ((long long)n * cells) * Cin + ch * KC;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const unsigned goff = spTab[(2 * c + 1) * S_TPB + tid].w;
      const float* gp = gb + goff;
      const unsigned char* wq = wb + goff;
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(spg[c][0]) : "v"(gp) : "memory");
      asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=v"(spg[c][1]) : "v"(gp) : "memory");
      spw[c] = *reinterpret_cast<const sp_u2*>(wq);      // (compiler-visible: its first use is sp_tie, right behind the drain)
    }
  };
  auto sp_tie = [&]() {                                    // (after a full drain: the registers are defined HERE)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      asm volatile("" : "+v"(spg[c][0]));
      asm volatile("" : "+v"(spg[c][1]));
      asm volatile("" : "+v"(spw[c]));
    }
  };
  constexpr int SP_PARTS = 6;
  auto sp_part = [&](int c, int part, int buf) {
    unsigned char* const img = gsm + buf * S_BUF_BYTES;
    constexpr int LO = S_PLANE * 16;                       // the lo plane of a stage buffer
    if (part == 0) {
      // split once per cell; zero records to all children (a redirected child's lands on its sibling's), the hi plane
      const sp_u4 r0 = spTab[(2 * c) * S_TPB + tid], r1 = spTab[(2 * c + 1) * S_TPB + tid];
      const float raw[8] = {spg[c][0].x, spg[c][0].y, spg[c][0].z, spg[c][0].w, spg[c][1].x, spg[c][1].y, spg[c][1].z, spg[c][1].w};
      float val[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) val[j] = fmaf(raw[j], sA, 0.f);
      bf16x8 parts[TERMS];
      split8<TERMS>(val, parts);
      const sp_u4 hb = __builtin_bit_cast(sp_u4, parts[0]), lb = __builtin_bit_cast(sp_u4, parts[1]);
#pragma unroll
      for (int q = 0; q < 4; ++q) { sph[q] = hb[q]; spl[q] = lb[q]; }
      spB = r1.z;
      const sp_u4 z4 = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const unsigned dk = (k & 1) ? r0[k >> 1] >> 16 : r0[k >> 1] & 0xffffu;
        *reinterpret_cast<sp_u4*>(img + spB + dk) = z4;
      }
    } else if (part == 1) {
      // the lo plane's zero records; record offsets and validity of every channel's winner: byte tables of the 8 children, looked
      // up four channels at a time
      const sp_u4 r0 = spTab[(2 * c) * S_TPB + tid], r1 = spTab[(2 * c + 1) * S_TPB + tid];
      const sp_u4 z4 = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const unsigned dk = (k & 1) ? r0[k >> 1] >> 16 : r0[k >> 1] & 0xffffu;
        *reinterpret_cast<sp_u4*>(img + spB + dk + LO) = z4;
      }
      const unsigned tl0 = __builtin_amdgcn_perm(r0[1], r0[0], 0x06040200u), th0 = __builtin_amdgcn_perm(r0[1], r0[0], 0x07050301u);
      const unsigned tl1 = __builtin_amdgcn_perm(r0[3], r0[2], 0x06040200u), th1 = __builtin_amdgcn_perm(r0[3], r0[2], 0x07050301u);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const unsigned k4 = spw[c][h] & 0x07070707u;      // selector bytes 0..7: children 0-3 from the first table word, 4-7 from the second
        const unsigned lo4 = __builtin_amdgcn_perm(tl1, tl0, k4), hi4 = __builtin_amdgcn_perm(th1, th0, k4);
        const unsigned m4 = __builtin_amdgcn_perm(r1.y, r1.x, k4);
        spP[2 * h] = __builtin_amdgcn_perm(hi4, lo4, 0x05010400u);          // channels 4 h, 4 h + 1: 16-bit offsets
        spP[2 * h + 1] = __builtin_amdgcn_perm(hi4, lo4, 0x07030602u);      // channels 4 h + 2, 4 h + 3
        spM[2 * h] = __builtin_amdgcn_perm(0u, m4, 0x01010000u);            // 16-bit masks
        spM[2 * h + 1] = __builtin_amdgcn_perm(0u, m4, 0x03030202u);
      }
    } else {
      // two channels: each one's hi / lo term into the record of its winner (zero where that child or the cell is outside)
      {
        const int q = part - 2;
        const unsigned hv = sph[q] & spM[q], lv = spl[q] & spM[q];
        unsigned char* const p0 = img + spB + (spP[q] & 0xffffu) + 4 * q;
        unsigned char* const p1 = img + spB + (spP[q] >> 16) + 4 * q + 2;
        *reinterpret_cast<unsigned short*>(p0) = (unsigned short)hv;
        *reinterpret_cast<unsigned short*>(p0 + LO) = (unsigned short)lv;
        *reinterpret_cast<unsigned short*>(p1) = (unsigned short)(hv >> 16);
        *reinterpret_cast<unsigned short*>(p1 + LO) = (unsigned short)(lv >> 16);
      }
    }
  };
  // B fragments straight from L2 through a two-slot register ring that runs THROUGH the stage boundaries: the fragments of step
  // s + 1 are requested at the HEAD of step s (into the slot step s - 1 has just finished issuing from), so they have a whole
  // step -- ~1.5k cycles, several L2 round trips -- to land.  Without CW (KMH_S_CW=0, round 4) every step opens with a plain
  // `s_waitcnt vmcnt(0)`; round 4's counted waits gave run-to-run different results here -- the compiler was moving in-flight
  // destinations (see CW above and b_issue below), which the tied waits and the ISA audit now exclude.
  // SPLIT: the ring holds a whole stage's fragments (one slot per step) and the fragments of step s + BA are requested in step
  // s, so that the wave drains its memory queue only at the head of every BA-th step: the LDS-DMA pieces of the next stage's
  // halo, issued in the steps right after a drain, then have BA - SP_PS + 1 or more steps (thousands of cycles) to come in
  // from HBM before anything waits for them -- a drain at every step head would expose that latency 18 times per chunk.
  constexpr int BD = (SPLIT || DEEP) ? NST : 2;        // ring slots
  // (SPARSE: no DMA pieces whose HBM latency the drain period must cover; a shorter period leaves 12 steps behind the first drain
  // after the cells' loads to deal the expansion over)
  constexpr int BA = SPARSE ? SPS_BA : (SPLIT ? SP_BA : (DEEP ? 7 : 1));     // request distance = drain period (steps)
  static_assert(NST % BD == 0 && (SPLIT || DEEP || BD == 2), "the ring slot of a step must not depend on the stage");
  static_assert(!SPLIT || (NST % BA == 0 && SP_PS < BA && NT == 1), "drains at steps 0, BA, ...; pieces land before the next one");
  auto piece_beg = [](int s) -> int { return s >= SP_PS ? S_NLD : (S_NLD * s) / SP_PS; };      // pieces of steps 0 .. SP_PS - 1
  constexpr int BL = 2 * NT;
  const long long step_stride = 2ll * CoutP, term_stride = (long long)NST * step_stride;
  bf16x8 bq[BD][NT][TERMS];
  long long o0 = 0;
  // (AMP: the lo fragments are never multiplied and must not even be requested -- an asm load whose destination the compiler
  // sees as dead lands LATER in a register it has meanwhile given to something else)
  auto b_issue = [&](int slot) {
    const bf16x8* p0 = wp + o0;
    const bf16x8* p1 = p0 + term_stride;
    // The stage-deep ring of the 32-wide tile lives in the ACCUMULATOR half of the register file.  With "=v" destinations the
    // kernel needs 256 VGPRs + 218 AGPRs and the compiler, for which an asm load's destination is defined as soon as the
    // statement ends, moved 11 of the ring's registers into AGPRs (v_accvgpr_write) while their loads were still in flight: the
    // copies held stale data, the loads landed in registers since given to something else, the GPU faulted.  "=a" destinations
    // leave it nothing to move (MFMA reads its B operand from AGPRs directly); tools/scan_asm_inflight.py audits the ISA of
    // every instance for such copies and runs in the CPU test suite.
    if constexpr (DEEP && !KMH_S_DEEP_RING_V) {
      asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(bq[slot][0][0]) : "v"(p0) : "memory");
      if (!AMP) asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(bq[slot][0][1]) : "v"(p1) : "memory");
      o0 += step_stride;
      return;
    }
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(bq[slot][0][0]) : "v"(p0) : "memory");
    if (!AMP) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(bq[slot][0][1]) : "v"(p1) : "memory");
    if (NT == 2) {
      asm volatile("global_load_dwordx4 %0, %1, off offset:512" : "=v"(bq[slot][NT - 1][0]) : "v"(p0) : "memory");
      if (!AMP) asm volatile("global_load_dwordx4 %0, %1, off offset:512" : "=v"(bq[slot][NT - 1][1]) : "v"(p1) : "memory");
    }
    o0 += step_stride;
  };
  auto b_tie = [&](int slot) {                           // (after a wait: the slot's registers are defined HERE)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q = AMP ? 0 : 1; q >= 0; --q) {
        if constexpr (DEEP && !KMH_S_DEEP_RING_V) asm volatile("" : "+a"(bq[slot][t][q]));
        else asm volatile("" : "+v"(bq[slot][t][q]));
      }
  };
  // CW: loads issued after the youngest one step s needs, up to the wait at its head (a step issues its fragments, then, in
  // steps 1 .. 8, a raw voxel's two halves): the fragments of step s were requested BA steps earlier, the voxel it converts CD
  constexpr int NBL = NT * (AMP ? 1 : 2);                // loads of one b_issue
  auto cw_count = [&](int s_) -> int {
    auto nr = [&](int t) -> int { t = ((t % NST) + NST) % NST; return (t >= 1 && t < 9) ? 2 : 0; };
    int yr = 0, yb = nr(s_ - BA);
    for (int t = s_ - CD + 1; t < s_; ++t) yr += NBL + nr(t);
    for (int t = s_ - BA + 1; t < s_; ++t) yb += NBL + nr(t);
    return yr < yb ? yr : yb;
  };
  auto a_offset = [&](int s) -> int {                    // LDS slot offset of this lane's A fragment of step s, row 0
    constexpr int last_tap = ZP ? 35 : 26;
    const int tapA = 2 * s, tapB = (2 * s + 1 > last_tap) ? last_tap : 2 * s + 1;      // padded half-step: zero weights
    const int offA = ((tapA / 9) * GHY + (tapA / 3) % 3) * HX + tapA % 3;
    const int offB = ((tapB / 9) * GHY + (tapB / 3) % 3) * HX + tapB % 3;
    return lh ? offB : offA;
  };

  int tr_n = 0;                                            // KMH_G_TRACE: cycle stamps of workgroup 0, wave 0
  auto stamp = [&]() {
    if (trace && blockIdx.x == 0 && tid == 0 && tr_n < 240) trace[tr_n++] = __builtin_readcyclecounter();
  };
  // prologue: the first stage's halo, fetched and converted with nothing to hide behind
  unsigned cv_in = fill_offsets(cur);
  unsigned cv_brick_next = 0u;                             // the NEXT brick's bits, formed with its table in its predecessor's last stage
  if constexpr (SPARSE) {
    sp_issue(cur.n, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    sp_tie();
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int part = 0; part < SP_PARTS; ++part) sp_part(c, part, 0);
  } else if constexpr (SPLIT) {
#pragma unroll
    for (int p = 0; p < S_NLD; ++p) dma_piece(cur.n, 0, 0, p, sOff[(p >> 1) * S_TPB + tid]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    fill_coef(cur.n);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < S_NCV; ++i) {
      raw_issue(cur.n, 0, 0, sOff[i * S_TPB + tid], sOff[(8 + i) * S_TPB + tid]);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (CW) raw_tie(0);
      convert1(0, cv_in, 0, i, rawq[0][0], rawq[0][1]);
    }
  }
  o0 = lh * CoutP + cur.cog * (32 * NT) + li;             // chunk 0 of the first brick: the fragments of steps 0 .. BA - 1
#pragma unroll
  for (int d = 0; d < BA; ++d) b_issue(d);
  if (SPLIT || DEEP) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  int pb = 0;                                              // stage buffer holding the CURRENT stage's fragment images
  for (;;) {
    const bool more = next_item(vb, nxt);
    const int co0 = cur.cog * (32 * NT);
    const int n = cur.n;
    const int boff = lh * CoutP + co0 + li;
    f32x16 acc[MR][NT];
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][t][r] = 0.f;

    for (int ch = 0; ch < nchunk; ++ch) {
      // stage top: this wave's conversion writes are out; after the barrier everybody's are -- and every wave is done with
      // the MFMAs (and the epilogue tiles) of the previous stage: the other buffer may be overwritten by the next DMA
      stamp();                                             // stage top
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      stamp();                                             // barrier passed
      const bf16x8* sIn = reinterpret_cast<const bf16x8*>(gsm + pb * S_BUF_BYTES);      // [TERMS][S_PLANE]
      const bool last_ch = ch + 1 == nchunk;
      // The step loop requests the "next stage's" fragments / voxels / pieces even when there is no next stage (the addresses
      // stay valid: stage 0 of the current pair): no branch inside a step, one scheduling region per step, and the same loads in
      // every stage, which the counted waits need.  (With a branch around them the ISA audit flags the pooling instances of the
      // full-drain build: profiles/ab_arms_retired_kernel_identity.md.)
      const int nn = (last_ch && more) ? nxt.n : n, nch = last_ch ? 0 : ch + 1;
      unsigned cv_next = last_ch ? 0u : cv_in;             // (the next BRICK's table and bits: inside step 0, below)
      if (!SPLIT && nn != coef_n) {                        // uniform, rare: the work list moves on to another sample
        fill_coef(nn);
        __syncthreads();
      }
      const int co0n = ((last_ch && more) ? nxt.cog : cur.cog) * (32 * NT);      // the next stage's cout group
      int vr = vrow;
      asm volatile("" : "+v"(vr));
      int dof0 = 0, dof1 = 0;                              // the next raw voxel's source offsets (read one step ahead)
      bf16x8 a[2][MR][TERMS];                              // this step's A fragments and the next step's
      {
        const int ab = vr + a_offset(0);
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
          for (int q = 0; q < TERMS; ++q) a[0][m][q] = sIn[q * S_PLANE + ab + arow(m)];
      }
#pragma unroll
      for (int s = 0; s < NST; ++s) {
        // everything requested so far has landed: this step's B fragments (requested at the head of the last step), the raw
        // voxel s - 1, a previous brick's output stores
        // (SPLIT: only every BA-th step drains; step 0 of a brick's first stage does not either -- its fragments were waited
        // for ahead of the previous brick's epilogue, whose output stores thus stay in flight under BA steps of MFMAs)
        // (CW: counted -- the fragments of this step and the voxel it converts have landed, younger requests stay in flight;
        // DEEP: the first steps of a brick's first stage need nothing that was not waited for ahead of the previous epilogue)
        if constexpr (CW) {
          if (!(DEEP && ch == 0 && s <= CD)) vm_wait(cw_count(s));
          b_tie(s % BD);
          if (s >= 1 + CD && s < 9 + CD) raw_tie((s - 1 - CD) % RQ);
        } else if (!(SPLIT || DEEP) || (s % BA == 0 && !(s == 0 && ch == 0))) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (SPARSE) { if (s == BA) sp_tie(); }      // the two cells requested in step 0 have landed
        if (s + BA < NST) b_issue((s + BA) % BD);             // the fragments of step s + BA ...
        else {                                                // ... or of step s + BA - NST of the next stage
          if (s + BA == NST) o0 = (long long)nch * TERMS * term_stride + lh * CoutP + co0n + li;
          b_issue((s + BA - NST) % BD);
        }
        if (CW && s >= 1 && s < 9) raw_issue(nn, nch, (s - 1) % RQ, dof0, dof1);      // (CW: a fixed place in the load order)
        __builtin_amdgcn_sched_barrier(0);
        // the next stage's voxel s - 1 is requested in step s (1..8) and converted in step s + 1.  Step 0 of a brick's last stage
        // first replaces the offset table and the inside bits by the next brick's (~400 VALU: fillers here, 3k cycles at the
        // stage top before)
        if (s == 0 && last_ch && more) { cv_brick_next = fill_offsets(nxt); cv_next = cv_brick_next; }
        if constexpr (SPARSE) {
          // the next stage's two cells: requested in step 0 (after the table has been replaced), landed by the drain at the head
          // of step BA, expanded one part per step after it
          if (s == 0) sp_issue(nn, nch);
        } else if constexpr (SPLIT) {
          // this step's share of the next stage's 16 pieces (step 0: after the offset table has been replaced)
#pragma unroll
          for (int p = piece_beg(s); p < piece_beg(s + 1); ++p) dma_piece(nn, nch, pb ^ 1, p, sOff[(p >> 1) * S_TPB + tid]);
        } else {
        if (!CW && s >= 1 && s < 9) raw_issue(nn, nch, (s - 1) % RQ, dof0, dof1);
        if (s < 8) { dof0 = sOff[s * S_TPB + tid]; dof1 = sOff[(8 + s) * S_TPB + tid]; }
        }
        if (s + 1 < NST) {
          const int ab = vr + a_offset(s + 1);
#pragma unroll
          for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int q = 0; q < TERMS; ++q) a[(s + 1) & 1][m][q] = sIn[q * S_PLANE + ab + arow(m)];
        }
        constexpr int SP0 = BA;                              // SPARSE: first expansion step
        static_assert(!SPARSE || SP0 + 2 * SP_PARTS <= NST, "two cells' expansion steps behind the drain");
        if (SPARSE && s >= SP0 && s < SP0 + 2 * SP_PARTS) sp_part((s - SP0) / SP_PARTS, (s - SP0) % SP_PARTS, pb ^ 1);
        // the next stage's voxel s - 2 (requested in the last step)
        if (!SPLIT && s >= 1 + CD && s < 9 + CD) convert1(nch, cv_next, pb ^ 1, s - 1 - CD, rawq[(s - 1 - CD) % RQ][0], rawq[(s - 1 - CD) % RQ][1]);
        // term-major over the 8 x NT accumulators: per accumulator the order of conv3_fwd_bf_kernel (smallest terms first)
#pragma unroll
        for (int q3 = AMP ? 2 : 0; q3 < 3; ++q3)       // (AMP: hi x hi only)
#pragma unroll
          for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int t = 0; t < NT; ++t)
              acc[m][t] = mfma16<TERMS>(a[s & 1][m][q3 == 0 ? 1 : 0], bq[s % BD][t][q3 == 1 ? 1 : 0], acc[m][t]);
        constexpr int NMF = MR * NT * (AMP ? 1 : 3);          // MFMAs of a step
        if constexpr (KMH_S_IL != 0) {
          // ONE scheduling region per step (no branch inside: the next stage's requests are unconditional), its single-issue
          // instructions dealt over the MFMA gaps: a wave alone on its SIMD hides about five of them beside a 32-cycle MFMA, and
          // whatever sits in front of the step's first MFMA runs with the matrix pipe idle (the "reads first" arrangement put
          // 30-60 instructions there).
          const bool conv_step = !SPLIT && s >= 1 + CD && s < 9 + CD;
#pragma unroll
          for (int k = 0; k < NMF; ++k) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                   // one MFMA
            if (k < S_ILR) __builtin_amdgcn_sched_group_barrier(0x100, S_ILRN, 0);              // LDS reads: early gaps
            if (k == 1) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);                       // the raw voxel's two loads
            if (SPARSE && s == 0 && k >= 2 && k < 5) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);      // the two cells' six loads
            if (SPARSE && s >= SP0 && s < SP0 + 2 * SP_PARTS) {      // an expansion part: its VALU over all gaps, its LDS writes behind the reads
              __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
              if (k >= 6) __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);
            }
            if (conv_step && k >= S_ILV0) __builtin_amdgcn_sched_group_barrier(0x002, NT == 2 ? S_ILV2 : S_ILV1, 0);
          }
        } else {      // the "reads first" arrangement the dealt one replaced: built only by the ISA audit's positive control
        if (SPLIT || !(s >= 1 + CD && s < 9 + CD)) __builtin_amdgcn_sched_group_barrier(0x100, 64, 0);      // plain steps: reads first too
        if (!SPLIT && s >= 1 + CD && s < 9 + CD) {
          // every LDS read of the block first (the next step's A fragments, the coefficients, the next offsets), then a few bare
          // MFMAs while they land -- a wait in the middle of the MFMA stream stalls it --, then the conversion's VALU a few per gap
          __builtin_amdgcn_sched_group_barrier(0x100, 64, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
#pragma unroll
          for (int k = 0; k < NMF - 6; ++k) {
            __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);             // a few of the conversion's VALU ...
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);             // ... one MFMA
          }
        }
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_sched_barrier(0);
        if (KMH_S_STAMPALL || s == 0 || s == 9 || s == NST - 1) stamp();      // steps 0 / .. 9 / .. NST - 1 done (debug builds: every step)
      }
      if (!last_ch) pb ^= 1;                               // (after a brick's last stage the epilogue still uses its buffer)
    }

    // ---- epilogue of the brick: the wave's rows go through its own 8 KB of the (now idle) stage buffer, row by row, and
    // are stored 16 bytes per lane (conv3_fwd_g_kernel's epilogue, 8 rows per wave).  (Forming the products transposed --
    // weights as the A operand, so that four accumulator registers are four channels of one voxel and no LDS transposition is
    // needed -- was measured: the 32-byte pieces those stores write cost 60-68k cycles per brick against 33k here.)
    // (SPLIT: the next stage's first fragments, requested in the last BA steps, land here -- L2 hits, long issued -- so that
    // step 0 of the next brick need not drain the queue the output stores below are about to fill)
    if (SPLIT || DEEP) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int x0 = cur.bx * TX, y0 = cur.by * GTY, z0 = cur.bz * GTZ;
    constexpr int CH = 32 * NT;
    constexpr int L4 = CH / 4;
    constexpr int VPI = 64 / L4;
    const long long sbrick = ((long long)n * tiles_z * tiles_y * tiles_x + ((long long)cur.bz * tiles_y + cur.by) * tiles_x + cur.bx);
    unsigned char* sEp = gsm + pb * S_BUF_BYTES;
    float* tile0 = reinterpret_cast<float*>(sEp) + wv * (2 * 32 * CH);      // two tiles per wave: row m + 1 is written while
                                                                          // row m's read-back and stores are in flight
    const int c4 = lane % L4, vx = lane / L4;
    const int col = 4 * c4;
    const int pl = ZP ? col >> 4 : 0;                          // ZP: column = (channel, output plane of the pair)
    const int co = ZP ? (col & 15) : co0 + col;
    const bool co_ok = co < Cout;
    float4 bv = {0.f, 0.f, 0.f, 0.f};
    if (bias && co_ok) bv = *reinterpret_cast<const float4*>(bias + co);
    float st1[4] = {0.f, 0.f, 0.f, 0.f}, st2[4] = {0.f, 0.f, 0.f, 0.f};
    __syncthreads();                                           // every wave is done with the fragment images
    const int gz = z0 + wz + pl;
    if (POOL) stamp();
    if constexpr (POOL) {
      // (x, y) pooling IN REGISTERS: a lane's accumulator registers (2 q, 2 q + 1) of row m are the two x children of pooled
      // column X = (q & 1) + 4 (q >> 1) + 2 lh for ONE channel (column li of the tile), rows 2 p / 2 p + 1 of the same wave its
      // y children: no LDS round trip per row (the row-tile version: 16 stores, a wait, 4 loads, a wait, eight times over --
      // this single wave per SIMD is latency-bound there).  Planes wz (even) and wz + 1, both this wave's, hold the z children.
      // Scan order of the reference (z, y, x; a later value wins only if strictly greater, or NaN): lower-index
      // halves are combined first -- the same winners as kmh_maxpool3d_fwd.
      // (after a ReLU no value is NaN -- v_max_f32 returns its other operand -- and ATen's "a NaN wins" test, one unordered compare
      // and one mask OR per comparison, 274 of the epilogue's ~ 2000 instructions, is compiled out: two instances of the block)
      auto pool_block = [&](auto nan_wins) {
      constexpr bool NANW = decltype(nan_wins)::value;
      auto pick = [](float a, float b, unsigned ca, unsigned cb, float& m_, unsigned& c_) {
        const bool tb = (b > a) || (NANW && (b != b));
        m_ = tb ? b : a; c_ = tb ? cb : ca;
      };
      const int cl = co0 + li;
      const float bch = (bias && cl < Cout) ? bias[cl] : 0.f;
      float pvv[MR / 2][8];
      unsigned pcc[MR / 2];                                                 // 8 window codes of 4 bits
#pragma unroll
      for (int p = 0; p < MR / 2; ++p) {
        pcc[p] = 0u;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          float a0 = acc[2 * p][0][2 * q] * desc + bch, a1 = acc[2 * p][0][2 * q + 1] * desc + bch;
          float b0 = acc[2 * p + 1][0][2 * q] * desc + bch, b1 = acc[2 * p + 1][0][2 * q + 1] * desc + bch;
          if (relu_out) { a0 = fmaxf(a0, 0.f); a1 = fmaxf(a1, 0.f); b0 = fmaxf(b0, 0.f); b1 = fmaxf(b1, 0.f); }
          float t0, t1, t;
          unsigned c0, c1, c;
          pick(a0, a1, 0u, 1u, t0, c0);                                      // x children of the first row: codes 0 / 1
          pick(b0, b1, 0u, 1u, t1, c1);                                      // ... of the second row
          pick(t0, t1, c0, c1 + 2u, t, c);                                   // y children: + 2 for the second row
          pvv[p][q] = t;
          pcc[p] |= c << (4 * q);
        }
      }
      stamp();
      // z children = rows m / m + 4 of THIS wave: pooled rows p = 0, 1 of the lower plane meet p + 2 of the upper one.  Then
      // the wave's pooled tile (2 rows x 16 columns x 32 channels) is transposed through its own 5 KB so that a lane stores 4
      // channels of one pooled voxel (16 bytes; a wave instruction = 8 voxels = 1 KB of contiguous output).
      float* tv = reinterpret_cast<float*>(sEp) + wv * (32 * 32 + 32 * 8);                                // [32 voxels][32]
      unsigned char* tc = reinterpret_cast<unsigned char*>(tv + 32 * 32);                                 // [32 voxels][32] bytes
#pragma unroll
      for (int p = 0; p < MR / 4; ++p) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          float o;
          unsigned c;
          pick(pvv[p][q], pvv[p + MR / 4][q], (pcc[p] >> (4 * q)) & 15u, ((pcc[p + MR / 4] >> (4 * q)) & 15u) + 4u, o, c);
          const int X = (q & 1) + 4 * (q >> 1) + 2 * lh;
          tv[(p * 16 + X) * 32 + li] = o;
          tc[(p * 16 + X) * 32 + li] = (unsigned char)c;
        }
      }
      // (the wave's own LDS writes are ordered before its reads)
      stamp();
      const int Do = D >> 1, Ho = H >> 1, Wo = W >> 1;
      const int oz = (z0 + wz) >> 1;
      const int jx = lane >> 3;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int vi = jx + 8 * k, pr = vi >> 4, X = vi & 15;
        const float4 o4 = *reinterpret_cast<const float4*>(tv + vi * 32 + col);
        const unsigned cw = *reinterpret_cast<const unsigned*>(tc + vi * 32 + col);
        const int oy = ((y0 + wy) >> 1) + pr, ox = (x0 >> 1) + X;
        if (oz < Do && oy < Ho && ox < Wo && co_ok) {
          const long long e = ((((long long)n * Do + oz) * Ho + oy) * Wo + ox) * Cout + co;
          *reinterpret_cast<float4*>(y + e) = o4;
          pool_arg[e >> 2] = cw;
          st1[0] += o4.x; st2[0] += o4.x * o4.x; st1[1] += o4.y; st2[1] += o4.y * o4.y;
          st1[2] += o4.z; st2[2] += o4.z * o4.z; st1[3] += o4.w; st2[3] += o4.w * o4.w;
        }
      }
      };
      if (relu_out) pool_block(std::false_type{});
      else pool_block(std::true_type{});
    } else {
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      float* tile = tile0 + (m & 1) * (32 * CH);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) tile[((r & 3) + 8 * (r >> 2) + 4 * lh) * CH + 32 * t + li] = acc[m][t][r];
      const int gy = y0 + wy + m;
      const bool row_ok = gz < D && gy < H && co_ok;
      const long long rowoff = ((((long long)n * D + gz) * H + gy) * W) * Cout + co;
      float4 v4[32 / VPI], ad[32 / VPI];
#pragma unroll
      for (int k = 0; k < 32 / VPI; ++k) {
        const int xx = vx + VPI * k;
        v4[k] = *reinterpret_cast<const float4*>(tile + xx * CH + col);
        ad[k] = float4{0.f, 0.f, 0.f, 0.f};
        if (addend && row_ok && x0 + xx < W) ad[k] = *reinterpret_cast<const float4*>(addend + rowoff + (long long)(x0 + xx) * Cout);
      }
#pragma unroll
      for (int k = 0; k < 32 / VPI; ++k) {
        const int gx = x0 + vx + VPI * k;
        if (row_ok && gx < W) {
          float4 o;
          o.x = v4[k].x * desc + bv.x + ad[k].x; o.y = v4[k].y * desc + bv.y + ad[k].y;
          o.z = v4[k].z * desc + bv.z + ad[k].z; o.w = v4[k].w * desc + bv.w + ad[k].w;
          if (relu_out) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
          *reinterpret_cast<float4*>(y + rowoff + (long long)gx * Cout) = o;
          st1[0] += o.x; st2[0] += o.x * o.x; st1[1] += o.y; st2[1] += o.y * o.y;
          st1[2] += o.z; st2[2] += o.z * o.z; st1[3] += o.w; st2[3] += o.w * o.w;
        }
      }
    }
    }   // !POOL
    if (POOL) stamp();
    if (stats_partial) {
      double d1[4], d2[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        d1[j] = (double)st1[j]; d2[j] = (double)st2[j];
#pragma unroll
        for (int o = L4; o < 64; o <<= 1) { d1[j] += __shfl_xor(d1[j], o); d2[j] += __shfl_xor(d2[j], o); }
      }
      if (POOL) stamp();
      __syncthreads();                                         // the tiles have been read back
      double* sred = reinterpret_cast<double*>(sEp);           // [wave][CH][2]
      if (lane < L4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { sred[((wv * CH) + col + j) * 2] = d1[j]; sred[((wv * CH) + col + j) * 2 + 1] = d2[j]; }
      }
      __syncthreads();
      const int ncol = ZP ? 16 : CH;
      if (tid < 2 * ncol) {
        const int k = tid & 1, c = tid >> 1;
        const int cch = ZP ? c : co0 + c;
        if (cch < Cout) {
          // (the outputs are bit-identical to conv3_fwd_g_kernel's; these sums group them by wave = plane (pair) instead of by
          // (plane, row half), so they agree with that kernel's to fp32 rounding of the per-lane partial sums, not bit for bit)
          double sum = 0.0;
#pragma unroll
          for (int w4 = 0; w4 < 4; ++w4) {
            sum += sred[(w4 * CH + c) * 2 + k];
            if (ZP) sum += sred[(w4 * CH + 16 + c) * 2 + k];   // the second plane of the pair
          }
          stats_partial[(sbrick * Cout + cch) * 2 + k] = sum;
        }
      }
    }
    stamp();                                               // epilogue issued
    if (!more) break;
    cur = nxt;
    cv_in = cv_brick_next;
    pb ^= 1;
  }
  // (the last stage requested a "next stage" that does not exist -- nothing may still be in flight to this wave's
  // registers or to the workgroup's LDS when they are handed to another workgroup)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace
static inline bool use_zpair(int Cout) { return Cout <= 16; }      // the z-paired N tile (and weight packing) serves these

KMH_API size_t kmh_conv3d_pack_bf_bytes(int Cout, int Cin, int transposed, int terms) {
  const int Co = transposed ? Cin : Cout, Ci = transposed ? Cout : Cin;
  return (size_t)((Ci + 7) / 8) * terms * (use_zpair(Co) ? NSTEP_Z : NSTEP) * 2 * cout_pad(Co) * 8 * sizeof(__bf16);
}

KMH_API int kmh_conv3d_pack_weight_bf(const float* w, void* packed, int Cout, int Cin, int transposed, int terms,
                                      const float* wscale, void* stream) {
  const int Co = transposed ? Cin : Cout, Ci = transposed ? Cout : Cin;
  const int nchunk = (Ci + 7) / 8, CoutP = cout_pad(Co), zp = use_zpair(Co);
  const long long total = (long long)nchunk * (zp ? NSTEP_Z : NSTEP) * 2 * CoutP * 8;
  int nb = ceil_div(total, 256);
  if (nb > 2048) nb = 2048;
  hipStream_t s = (hipStream_t)stream;
  if (terms == 2 && !wscale) return -22;
  if (terms == 2) pack_weight_bf_kernel<2><<<nb, 256, 0, s>>>(w, (__bf16*)packed, Cout, Cin, CoutP, nchunk, transposed, zp, wscale);
  else if (terms == 3) pack_weight_bf_kernel<3><<<nb, 256, 0, s>>>(w, (__bf16*)packed, Cout, Cin, CoutP, nchunk, transposed, zp, wscale);
  else return -22;
  return KMH_LAUNCH_CHECK();
}

// the epilogue statistics' last step (stats_out != NULL), then the launch status every launcher returns
static int finish_stats(double* stats_ws, int bricks, int Cout, int N, double* stats_out, hipStream_t s) {
  if (stats_out) kmh_stats::final_kernel<<<dim3(ceil_div(Cout * 2, 256 / kWave), N), 256, 0, s>>>(stats_ws, bricks, Cout, stats_out);
  return KMH_LAUNCH_CHECK();
}

/* x (N,D,H,W,Cin) -> y (N,D,H,W,Cout); `packed` from kmh_conv3d_pack_weight_bf for the SAME (Cin, Cout) view:
 * forward: pack(w, Cout, Cin, 0); data gradient: pack(w, Cout_w, Cin_w, 1) and call with Cin = Cout_w, Cout = Cin_w */
template <int NT, int TERMS, int MR, bool ZP = false, int ZT = 1>
static int launch_fwd_bf(const float* x, const float* scale, const float* shift, const float* mask, const bf16x8* wp,
                         const float* bias, float* y, int N, int D, int H, int W, int Cin, int Cout, int CoutP,
                         int relu_in, int relu_out, const float* ascale, const float* wscale, double* stats_ws,
                         double* stats_out, hipStream_t s, int in_blocked = 0, const float* addend = nullptr) {
  const int tx = ceil_div(W, TX), ty = ceil_div(H, (ZP ? 4 : 2) * MR), tz = ceil_div(D, 2 * ZT);
  const int typ = ceil_div(ty, 8), tzp = ceil_div(tz, 8);         // (y, z) patches of 8 x 8 bricks
  dim3 g(tx * typ * tzp * 64 * (ZP ? 1 : ceil_div(Cout, 32 * NT)), 1, N);
  conv3_fwd_bf_kernel<NT, TERMS, MR, ZP, ZT><<<g, BF_TPB, 0, s>>>(x, scale, shift, mask, wp, bias, y, D, H, W, Cin, Cout,
                                                             CoutP, relu_in, relu_out, tx, ty, tz, tzp, ascale, wscale,
                                                             stats_out ? stats_ws : nullptr, in_blocked, addend);
  return finish_stats(stats_ws, tx * ty * tz, Cout, N, stats_out, s);
}

// What the two persistent kernels' launchers share.  Their grid: `total` virtual blocks per sample (32 x 8 x 4 bricks in (y, z)
// patches of 8 x 8, x `groups` cout groups) and persistent workgroups, one per CU, over ONE work list of N * total bricks (a
// multiple of 8 workgroups, so that every id of a workgroup's list falls on its own XCD)
struct PersistentGrid { int tx, ty, tz, tzp, total, wgs; };
static PersistentGrid persistent_grid(int N, int D, int H, int W, int groups) {
  const int tx = ceil_div(W, TX), ty = ceil_div(H, GTY), tz = ceil_div(D, GTZ), tzp = ceil_div(tz, 8);
  const int total = tx * ceil_div(ty, 8) * tzp * 64 * groups;
  const long long all8 = ((long long)N * total + 7) / 8 * 8;
  return {tx, ty, tz, tzp, total, all8 < 256 ? (int)all8 : 256};
}
template <typename K>
static int allow_lds(K kernel, int bytes) {      // 0 or the hipError_t
  return (int)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}
// KMH_G_TRACE=1 (debug): cycle stamps of workgroup 0 to stderr.  trace_begin: the cleared buffer the kernel stamps into (NULL
// unless tracing); trace_end: waits for the stream, prints the label and the differences between consecutive stamps.
static long long* trace_begin(hipStream_t s) {
  static long long* trace = nullptr;
  static const bool tracing = getenv("KMH_G_TRACE") != nullptr;
  if (tracing && !trace && hipMalloc(&trace, 240 * sizeof(long long)) != hipSuccess) trace = nullptr;
  if (trace) (void)hipMemsetAsync(trace, 0, 240 * sizeof(long long), s);
  return trace;
}
template <typename... A>
static void trace_end(const long long* trace, hipStream_t s, const char* label, A... a) {
  if (!trace) return;
  long long h[240];
  (void)hipStreamSynchronize(s);
  (void)hipMemcpy(h, trace, sizeof(h), hipMemcpyDeviceToHost);
  fprintf(stderr, label, a...);
  for (int i = 1; i < 240 && h[i]; ++i) fprintf(stderr, " %lld", h[i] - h[i - 1]);
  fprintf(stderr, "\n");
}

template <int NT, bool ZP, bool POOL = false>
static int launch_fwd_g(const float* x, const float* scale, const float* shift, const bf16x8* wp, const float* bias,
                        float* y, int N, int D, int H, int W, int Cin, int Cout, int CoutP, int relu_in, int relu_out,
                        const float* ascale, const float* wscale, double* stats_ws, double* stats_out, hipStream_t s,
                        int in_blocked, const float* addend, unsigned* pool_arg = nullptr) {
  if (int e = allow_lds(conv3_fwd_g_kernel<NT, ZP, POOL>, G_LDS_BYTES)) return e;
  const PersistentGrid g = persistent_grid(N, D, H, W, ZP ? 1 : ceil_div(Cout, 32 * NT));
  long long* trace = trace_begin(s);
  conv3_fwd_g_kernel<NT, ZP, POOL><<<dim3(g.wgs), G_TPB, G_LDS_BYTES, s>>>(x, scale, shift, wp, bias, y, D, H, W, Cin, Cout, CoutP,
                                                                           relu_in, relu_out, g.tx, g.ty, g.tz, g.tzp, ascale, wscale,
                                                                           stats_out ? stats_ws : nullptr, in_blocked, addend,
                                                                           g.total, N, trace, pool_arg);
  trace_end(trace, s, "KMH_G_TRACE NT=%d ZP=%d Cin=%d Cout=%d D=%d:", NT, (int)ZP, Cin, Cout, D);
  return finish_stats(stats_ws, g.tx * g.ty * g.tz, Cout, N, stats_out, s);
}

// amp: the entry point's use_amp flag (common.h: kmh_take_amp) -- the hi x hi instance of the same tile
template <int NT, bool ZP = false, bool SPLIT = false, bool POOL = false>
static int launch_fwd_s(bool amp, const float* x, const float* scale, const float* shift, const bf16x8* wp, const float* bias, float* y,
                        int N, int D, int H, int W, int Cin, int Cout, int CoutP, int relu_in, int relu_out,
                        const float* ascale, const float* wscale, double* stats_ws, double* stats_out, hipStream_t s,
                        int in_blocked, const float* addend, unsigned* pool_arg = nullptr) {
  if (int e = allow_lds(conv3_fwd_s_kernel<NT, ZP, SPLIT, POOL>, S_LDS_BYTES)) return e;
  const PersistentGrid g = persistent_grid(N, D, H, W, ZP ? 1 : ceil_div(Cout, 32 * NT));
  long long* trace = trace_begin(s);
#define KMH_S_ARGS x, scale, shift, wp, bias, y, D, H, W, Cin, Cout, CoutP, relu_in, relu_out, g.tx, g.ty, g.tz, g.tzp, ascale, wscale, \
                   stats_out ? stats_ws : nullptr, in_blocked, addend, g.total, N, trace, pool_arg
  if (amp) {
    if (int e = allow_lds(conv3_fwd_s_kernel<NT, ZP, SPLIT, POOL, true>, S_LDS_BYTES)) return e;
    conv3_fwd_s_kernel<NT, ZP, SPLIT, POOL, true><<<dim3(g.wgs), S_TPB, S_LDS_BYTES, s>>>(KMH_S_ARGS);
  } else
    conv3_fwd_s_kernel<NT, ZP, SPLIT, POOL><<<dim3(g.wgs), S_TPB, S_LDS_BYTES, s>>>(KMH_S_ARGS);
#undef KMH_S_ARGS
  trace_end(trace, s, "KMH_G_TRACE fwd_s NT=%d ZP=%d SPLIT=%d POOL=%d Cin=%d Cout=%d D=%d:", NT, (int)ZP, (int)SPLIT, (int)POOL, Cin, Cout, D);
  return finish_stats(stats_ws, g.tx * g.ty * g.tz, Cout, N, stats_out, s);
}

// the LDS-DMA kernel's preconditions: fp16 split, whole 8-channel chunks, no fused mask operand, and enough bricks to
// give every CU several of them
// 0: never, 1: when the launch has >= 512 bricks (default), 2: whenever the preconditions hold (parity tests force the
// kernel onto small / ragged volumes this way).  Initialised from KEYMORPH_FWD_G, changed by kmh_conv3d_fwd_bf_set_dispatch.
static std::atomic<int> g_fwd_g_mode{-1};
static int fwd_g_mode() {
  int m = g_fwd_g_mode.load(std::memory_order_relaxed);
  if (m < 0) {
    m = getenv("KEYMORPH_FWD_G") ? atoi(getenv("KEYMORPH_FWD_G")) : 1;
    if (m < 0 || m > 2) m = 1;
    g_fwd_g_mode.store(m, std::memory_order_relaxed);
  }
  return m;
}

// KEYMORPH_FWD_S=0 (read once per process): conv3_fwd_g_kernel, the eight-wave kernel, also where conv3_fwd_s_kernel would
// serve the 64-wide and 32-wide tiles and the pooling epilogue -- bit-identical outputs, kept as the parity arm of
// tests/test_conv_dispatch_gpu.py.  Any other value, or none: the one-wave kernel.
static bool fwd_s_on() {
  static const bool on = !(getenv("KEYMORPH_FWD_S") && atoi(getenv("KEYMORPH_FWD_S")) == 0);
  return on;
}

static bool fwd_g_ok(bool mask, bool addend, int N, int D, int H, int W, int Cin, int Cout, int terms) {
  const int mode = fwd_g_mode();
  if (!mode || terms != 2 || mask || (Cin & 7) || (Cout & 3)) return false;
  if (use_zpair(Cout) && addend) return false;
  if ((long long)D * H * W * (Cin > Cout ? Cin : Cout) >= (1ll << 31)) return false;          // 32-bit element offsets
  const long long wgs = (long long)N * ceil_div(W, TX) * ceil_div(H, GTY) * ceil_div(D, GTZ) *
                        (use_zpair(Cout) ? 1 : ceil_div(Cout, 64));
  return wgs >= (mode == 2 ? 1 : 512);
}

/* Kernel selection of kmh_conv3d_fwd_bf, settable at run time: mode 0 = conv3_fwd_bf_kernel always, 1 = the LDS-DMA
 * kernel (conv3_fwd_g_kernel) for launches of >= 512 bricks (default), 2 = conv3_fwd_g_kernel whenever its
 * preconditions hold, whatever the size.  Returns the previous mode (-22 for a bad argument). */
KMH_API int kmh_conv3d_fwd_bf_set_dispatch(int mode) {
  if (mode < 0 || mode > 2) return -22;
  const int old = fwd_g_mode();
  g_fwd_g_mode.store(mode, std::memory_order_relaxed);
  return old;
}

/* Which kernel kmh_conv3d_fwd_bf launches for this call under the current dispatch mode:
 * 0 conv3_fwd_bf_kernel, 1 conv3_fwd_g_kernel<1,false>, 2 conv3_fwd_g_kernel<2,false>, 3 conv3_fwd_g_kernel<1,true>
 * (z-paired, Cout <= 16). */
KMH_API int kmh_conv3d_fwd_bf_variant(int N, int D, int H, int W, int Cin, int Cout, int terms, int has_mask,
                                      int has_addend) {
  if (!fwd_g_ok(has_mask != 0, has_addend != 0, N, D, H, W, Cin, Cout, terms)) return 0;
  return use_zpair(Cout) ? 3 : (Cout > 32 ? 2 : 1);
}

/* in_blocked == 2 of kmh_conv3d_fwd_bf: x is the PRE-SPLIT channel-blocked tensor a producer such as kmh_maxpool3d_bwd_split
 * writes -- (N, Cin/8, D*H*W + 1) records of 32 bytes = the 8 fp16 "hi" then the 8 fp16 "lo" terms of fmaf(value, S, 0) with
 * S = ascale[0], record D*H*W of every (sample, chunk) plane all zeros -- so that the kernel copies fragments instead of
 * converting them (conv3_fwd_s_kernel<1, true, true>).  Served: the z-paired tile (Cout <= 16) of the one-wave kernel under its
 * usual preconditions, no scale / shift / mask / relu_in / addend (a gradient operand).  1 = served. */
KMH_API int kmh_conv3d_fwd_bf_split_ok(int N, int D, int H, int W, int Cin, int Cout, int terms) {
  if (!use_zpair(Cout) || Cin > S_COEF) return 0;
  if (((long long)D * H * W + 1) * KC >= (1ll << 31)) return 0;
  // The shape's own preconditions only -- NOT the tunable dispatch threshold (kmh_conv3d_fwd_bf_set_dispatch / KEYMORPH_FWD_G):
  // in_blocked == 2 always launches conv3_fwd_s_kernel<1, true, true>, whatever the mode, and a producer that asked this
  // question at forward time must get the same answer at backward time.
  if (N <= 0 || terms != 2 || (Cin & 7) || (Cout & 3)) return 0;
  if ((long long)D * H * W * (Cin > Cout ? Cin : Cout) >= (1ll << 31)) return 0;          // 32-bit element offsets
  return 1;
}

/* The convolution of a tensor that is the backward of a 2 x 2 x 2 max-pool, WITHOUT forming it: xp (N, D/2, H/2, W/2, Cin) fp32 is
 * the pooled gradient, `winners` (same shape, one byte per element) the window index 0..7 = (dz, dy, dx) that
 * kmh_conv3d_fwd_bf_pool / kmh_maxpool3d_fwd record; the operand stands for the (N, D, H, W, Cin) tensor with xp at each window's
 * winner and zeros elsewhere (what kmh_maxpool3d_bwd_split writes as records, in_blocked == 2 of kmh_conv3d_fwd_bf).  y and
 * stats_out are bit-identical to that route.  Served (kmh_conv3d_fwd_bf_sparse_ok): where the pre-split operand is, with even
 * D, H, W, in the f16x3 arithmetic (terms == 2; not use_amp's terms == 1).  The answer is for the SHAPE: it does not depend on the
 * dispatch mode.  Other arguments as kmh_conv3d_fwd_bf. */
KMH_API int kmh_conv3d_fwd_bf_sparse_ok(int N, int D, int H, int W, int Cin, int Cout, int terms) {
  if (terms != 2 || ((D | H | W) & 1) || D < 2 || H < 2 || W < 2) return 0;
  return kmh_conv3d_fwd_bf_split_ok(N, D, H, W, Cin, Cout, terms);
}

KMH_API int kmh_conv3d_fwd_bf_sparse(const float* xp, const unsigned char* winners, const void* packed, const float* bias,
                                     float* y, int N, int D, int H, int W, int Cin, int Cout, int relu_out, int terms,
                                     const float* ascale, const float* wscale, void* stats_ws, double* stats_out, void* stream) {
  if (!kmh_conv3d_fwd_bf_sparse_ok(N, D, H, W, Cin, Cout, terms) || !xp || !winners || !ascale || !wscale) return -22;
  if (((uintptr_t)xp & 15) || ((uintptr_t)winners & 7)) return -22;
  hipStream_t s = (hipStream_t)stream;
  if (int e = allow_lds(conv3_fwd_s_kernel<1, true, true, false, false, true>, S_LDS_BYTES)) return e;
  const PersistentGrid g = persistent_grid(N, D, H, W, 1);
  long long* trace = trace_begin(s);
  conv3_fwd_s_kernel<1, true, true, false, false, true><<<dim3(g.wgs), S_TPB, S_LDS_BYTES, s>>>(
      xp, nullptr, nullptr, (const bf16x8*)packed, bias, y, D, H, W, Cin, Cout, cout_pad(Cout), 0, relu_out, g.tx, g.ty, g.tz, g.tzp,
      ascale, wscale, stats_out ? (double*)stats_ws : nullptr, 0, nullptr, g.total, N, trace,
      reinterpret_cast<unsigned*>(const_cast<unsigned char*>(winners)));
  trace_end(trace, s, "KMH_G_TRACE fwd_s SPARSE Cin=%d Cout=%d D=%d:", Cin, Cout, D);
  return finish_stats((double*)stats_ws, g.tx * g.ty * g.tz, Cout, N, stats_out, s);
}

/* Convolution + ReLU + MaxPool3d(2) in one launch, for an encoder block whose output feeds ONLY the next level's pooling
 * (keymorph/unet3d/buildingblocks.py:46-78 then :321-380 `self.pooling(x)`): yp (N, D/2, H/2, W/2, Cout) = the pooled
 * output, arg (same shape, 1 byte per element) = the winners' window indices exactly as kmh_maxpool3d_fwd records them
 * (first maximum in z, y, x order), stats_out (N, Cout, 2) = (sum, sum^2) of the POOLED tensor; the full-resolution
 * output is never written.  Same arguments otherwise as kmh_conv3d_fwd_bf (no mask, bias, addend).
 * kmh_conv3d_fwd_bf_pool_ok says whether a shape is served (split-fp16 mode, whole 8-channel input chunks, 16 < Cout <= 32,
 * and the LDS-DMA kernel selected by the current dispatch mode). */
KMH_API int kmh_conv3d_fwd_bf_pool_ok(int N, int D, int H, int W, int Cin, int Cout, int terms) {
  return (Cout > 16 && Cout <= 32 && D >= 2 && H >= 2 && W >= 2 && fwd_g_ok(false, false, N, D, H, W, Cin, Cout, terms)) ? 1 : 0;
}

KMH_API int kmh_conv3d_fwd_bf_pool(const float* x, const float* scale, const float* shift, const void* packed, float* yp,
                                   unsigned char* arg, int N, int D, int H, int W, int Cin, int Cout, int relu_in,
                                   int terms, const float* ascale, const float* wscale, void* stats_ws, double* stats_out,
                                   int in_blocked, void* stream) {
  const bool amp = kmh_take_amp(terms);      // terms == 1: the fp16 kernels with hi x hi only (use_amp), for this call
  if (!kmh_conv3d_fwd_bf_pool_ok(N, D, H, W, Cin, Cout, terms) || !ascale || !wscale || !yp || !arg) return -22;
  if (((uintptr_t)yp & 15) || ((uintptr_t)arg & 3)) return -22;
  // the one-wave kernel's pooling epilogue (KEYMORPH_FWD_S=0: the eight-wave kernel's; same pooled values and winners)
  if (fwd_s_on() && Cin <= S_COEF)
    return launch_fwd_s<1, false, false, true>(amp, x, scale, shift, (const bf16x8*)packed, nullptr, yp, N, D, H, W, Cin, Cout,
                                               cout_pad(Cout), relu_in, 1, ascale, wscale, (double*)stats_ws, stats_out,
                                               (hipStream_t)stream, in_blocked, nullptr, (unsigned*)arg);
  return launch_fwd_g<1, false, true>(x, scale, shift, (const bf16x8*)packed, nullptr, yp, N, D, H, W, Cin, Cout,
                                      cout_pad(Cout), relu_in, 1, ascale, wscale, (double*)stats_ws, stats_out,
                                      (hipStream_t)stream, in_blocked, nullptr, (unsigned*)arg);
}

static inline int fwd_bf_rows(int Cout) {   // smallest brick height in y of the variants that may run
  return use_zpair(Cout) ? 8 : 4;
}

/* x (N,D,H,W,Cin) -> y (N,D,H,W,Cout); `packed` from kmh_conv3d_pack_weight_bf for the SAME (Cin, Cout) view:
 * forward: pack(w, Cout, Cin, 0); data gradient: pack(w, Cout_w, Cin_w, 1) and call with Cin = Cout_w, Cout = Cin_w.
 * rows_per_wave: 4 (32x8x2 brick) or 2 (32x4x2 brick, higher occupancy); 0 = library default. */
KMH_API size_t kmh_conv3d_fwd_bf_stats_ws_bytes(int N, int D, int H, int W, int Cout, int rows_per_wave) {
  return (size_t)N * ceil_div(W, TX) * ceil_div(H, fwd_bf_rows(Cout)) * ceil_div(D, TZ) * Cout * 2 *
         sizeof(double);
}

/* in_blocked != 0: x is stored channel-blocked, (N, Cin/8, D, H, W, 8) -- the 8 channels of a chunk of one voxel are
 * one 32-byte record and a chunk's voxels are contiguous, so the loader uses whole cache lines instead of a quarter of
 * each (Cin % 8 == 0, no mask; results are bit-identical; 8-13 % faster on the data-gradient launches).
 * stats_out (N,Cout,2) doubles | NULL: per-channel (sum y, sum y^2) of the OUTPUT, accumulated in the epilogue (what
 * kmh_channel_stats(y) would return: the next layer's GroupNorm statistics without another pass over y);
 * stats_ws: kmh_conv3d_fwd_bf_stats_ws_bytes. */
KMH_API int kmh_conv3d_fwd_bf(const float* x, const float* scale, const float* shift, const float* mask,
                              const void* packed, const float* bias, float* y, int N, int D, int H, int W, int Cin,
                              int Cout, int relu_in, int relu_out, int terms, int rows_per_wave, const float* ascale,
                              const float* wscale, void* stats_ws, double* stats_out, int in_blocked,
                              const float* addend, void* stream) {
  const bool amp = kmh_take_amp(terms);      // terms == 1: the fp16 kernels with hi x hi only (use_amp), for this call
  const int CoutP = cout_pad(Cout);
  hipStream_t s = (hipStream_t)stream;
  const bf16x8* wp = (const bf16x8*)packed;
  const int mr = rows_per_wave == 4 ? 4 : 2;
#define KMH_BF_CALL(NT_, T_, MR_) \
  return launch_fwd_bf<NT_, T_, MR_>(x, scale, shift, mask, wp, bias, y, N, D, H, W, Cin, Cout, CoutP, relu_in, relu_out, ascale, wscale, (double*)stats_ws, stats_out, s, in_blocked, addend)
  if (terms != 2 && terms != 3) return -22;
  if (addend && use_zpair(Cout)) return -22;
  if (in_blocked && ((Cin & 7) || mask)) return -22;
  if (in_blocked == 2) {      // pre-split input: see kmh_conv3d_fwd_bf_split_ok
    if (!kmh_conv3d_fwd_bf_split_ok(N, D, H, W, Cin, Cout, terms) || scale || shift || relu_in || addend || !ascale || !wscale)
      return -22;
    return launch_fwd_s<1, true, true>(amp, x, nullptr, nullptr, wp, bias, y, N, D, H, W, Cin, Cout, CoutP, 0, relu_out, ascale, wscale,
                                       (double*)stats_ws, stats_out, s, 2, nullptr);
  }
  if (terms == 2 && (!ascale || !wscale)) return -22;       // fp16 split without range scaling is not accurate
  // deep (32 x 8 x 4) bricks for the z-paired (Cout <= 16) launches on big volumes: less halo traffic, twice the B
  // reuse: +5 % on the 256^3 32->16 data gradient.  (The NT = 1, 4-rows-per-wave variant spills with 128 accumulator
  // registers plus 8 staging descriptors and is 4 % slower: not instantiated.)
  const bool deep = terms == 2 && Cout <= 32 && D >= 16 && (long long)D * H * W >= (1ll << 21);
  if (fwd_g_ok(mask != nullptr, addend != nullptr, N, D, H, W, Cin, Cout, terms)) {
    // the one-wave-per-SIMD kernel takes the 64-wide tile and the plain 32-wide one, the eight-wave kernel the z-paired tile
    // (the one-wave z-paired tile on fp32 operands was bit-identical, 3.7 % faster alone at 2 x 256^3 and flat inside the step:
    // retired); KEYMORPH_FWD_S=0: conv3_fwd_g_kernel for all of them
    if (use_zpair(Cout)) return launch_fwd_g<1, true>(x, scale, shift, wp, bias, y, N, D, H, W, Cin, Cout, CoutP, relu_in, relu_out, ascale, wscale, (double*)stats_ws, stats_out, s, in_blocked, addend);
    if (fwd_s_on() && Cin <= S_COEF) {
      if (Cout > 32) return launch_fwd_s<2>(amp, x, scale, shift, wp, bias, y, N, D, H, W, Cin, Cout, CoutP, relu_in, relu_out, ascale, wscale, (double*)stats_ws, stats_out, s, in_blocked, addend);
      return launch_fwd_s<1>(amp, x, scale, shift, wp, bias, y, N, D, H, W, Cin, Cout, CoutP, relu_in, relu_out, ascale, wscale, (double*)stats_ws, stats_out, s, in_blocked, addend);
    }
    if (Cout > 32) return launch_fwd_g<2, false>(x, scale, shift, wp, bias, y, N, D, H, W, Cin, Cout, CoutP, relu_in, relu_out, ascale, wscale, (double*)stats_ws, stats_out, s, in_blocked, addend);
    return launch_fwd_g<1, false>(x, scale, shift, wp, bias, y, N, D, H, W, Cin, Cout, CoutP, relu_in, relu_out, ascale, wscale, (double*)stats_ws, stats_out, s, in_blocked, addend);
  }
  if (use_zpair(Cout)) {   // weights were packed z-paired by kmh_conv3d_pack_weight_bf for this Cout
    if (terms == 2 && deep) return launch_fwd_bf<1, 2, 2, true, 2>(x, scale, shift, mask, wp, bias, y, N, D, H, W, Cin, Cout, CoutP, relu_in, relu_out, ascale, wscale, (double*)stats_ws, stats_out, s, in_blocked);
    if (terms == 2) return launch_fwd_bf<1, 2, 2, true>(x, scale, shift, mask, wp, bias, y, N, D, H, W, Cin, Cout, CoutP, relu_in, relu_out, ascale, wscale, (double*)stats_ws, stats_out, s, in_blocked);
    return launch_fwd_bf<1, 3, 2, true>(x, scale, shift, mask, wp, bias, y, N, D, H, W, Cin, Cout, CoutP, relu_in, relu_out, ascale, wscale, (double*)stats_ws, stats_out, s, in_blocked);
  }
  // Small volumes (the 32^3 level): the 32x8x2-brick grid has only ~512 workgroups for 512 slots, so half-height
  // bricks (twice the workgroups) run 1.9x faster there; with Cout % 128 == 0 the 128-wide N tile (NT = 4) adds
  // up to 10 % (the halo is staged once for twice the output channels).  Large grids prefer the tall bricks.
  const long long wgs4 = (long long)N * ceil_div(W, TX) * ceil_div(H, 8) * ceil_div(D, 2) * ceil_div(Cout, 64);
  const bool small_grid = wgs4 < 2048;
  if (small_grid && terms == 2 && Cout % 128 == 0) KMH_BF_CALL(4, 2, 2);
  // 64 < Cout <= 96 (the 32 -> 96 data gradient at full resolution): one 96-wide N tile on half-height bricks instead
  // of two 64-wide channel groups, the second of them half empty and both staging the same halo
  // (measured for Cout = 192 / 384 as 2 / 4 groups of 96: 9 % slower than 64-wide groups on the tall bricks)
  if (terms == 2 && Cout > 64 && Cout <= 96) KMH_BF_CALL(3, 2, 2);
  if (Cout > 32) {
    if (terms == 2) { if (mr == 4 && !small_grid) KMH_BF_CALL(2, 2, 4); else KMH_BF_CALL(2, 2, 2); }
    else { if (mr == 4) KMH_BF_CALL(2, 3, 4); else KMH_BF_CALL(2, 3, 2); }
  } else {
    if (terms == 2) { if (mr == 4) KMH_BF_CALL(1, 2, 4); else KMH_BF_CALL(1, 2, 2); }
    else { if (mr == 4) KMH_BF_CALL(1, 3, 4); else KMH_BF_CALL(1, 3, 2); }
  }
#undef KMH_BF_CALL
}
