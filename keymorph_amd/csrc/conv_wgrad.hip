// Split-bf16 weight gradient: dW[tap][ci][co] = sum_v xn[v + tap][ci] * dz[v][co].
// K of the MFMA = 16 consecutive voxels of one brick row, so BOTH operands need, per lane, 8 consecutive
// voxels of ONE channel: the brick is transposed while it is staged into channel-major bf16 LDS images
//   sXT[term][ci (+1 zero plane)][halo row][24]   plane pitch 1168 B (= 73 x 16 B: lanes = channels hit 16
//   sDT[term][co][128 voxels]                     plane pitch  272 B (= 17 x 16 B)   distinct 16-B slots)
// A fragment = aligned ds_read_b128 + ds_read_b32 around the window, then a funnel shift by the tap's x
// offset (0 / 2 / 4 bytes: v_alignbyte for kx = 1, register renaming for kx = 2); B fragment = one aligned
// ds_read_b128.  M rows are packed (tap, ci) with ci tiles of <= 16 channels (2 taps per 32-row tile),
// tiles dealt to the 8 waves exactly like the fp32 kernel; per-wave partial slabs, deterministic reduce.
// Kernels in this file:
//   conv3_wgrad_ws_kernel<NT, TERMS, MASK, PW, DSPLIT, AMP, DSPARSE>   producer / consumer waves over a ring of z planes (the default)
//   conv3_wgrad_bf_kernel<NT, TERMS>                          single-role (bf16x6, odd channel counts, huge volumes)
//   wgrad_bf_reduce_kernel, wgrad_bf_reduce_fold_kernel
#include "conv_split.h"
#include <type_traits>

namespace {

constexpr int WX = 16, WY = 4, WZ = 2;
constexpr int WHY = WY + 2, WHZ = WZ + 2;
constexpr int XROWS = WHY * WHZ;           // 24 halo rows
constexpr int XPITCH = 24;                 // elements per halo row (18 used)
constexpr int XPLANE = 1168;               // bytes per channel plane (24 rows x 48 B = 1152, padded)
constexpr int DPLANE = 272;                // bytes per cout plane (128 voxels x 2 B = 256, padded)
constexpr int WV = WX * WY * WZ;           // 128
// Round 6, the wave-specialised kernel: the x image is a RING of z planes.  Bricks are walked z-fastest, so a brick's 4-plane
// halo window shares 2 planes with its predecessor's: only the 2 new planes (12 of 24 halo rows) are fetched, normalised and
// split per brick -- the operand was 3.4 x redundant (432 halo voxels per 128-voxel brick), now 1.7 x.  8 ring planes: 4 being
// multiplied, up to 4 being filled (the first brick of a z column fills all 4 and starts 4 planes further on, so it never
// touches what the previous column's last brick is still being read from).
constexpr int RZ = 8;                                  // ring planes
// Plane pitch of the ring image: 2312 bytes = 578 words, i.e. 2 mod 32.  The consumers' A fragments are five dwords per lane that
// the compiler reads with 4-byte instructions (ds_read2_b32: it scalarises a 16-byte load whose dwords feed the funnel shifts one by
// one), whose 32-lane groups are 16 channels x 2 taps: with the pitch at 4 mod 32 words (2320 B = 145 x 16 B, chosen in round 2 for
// 16-byte reads that the compiler never emitted) 32 lanes hit 8 banks -- 57 % of the LDS-active cycles were bank conflicts and the LDS
// was 86 % busy (profiles/r6i_sq_counters_wgrad_ring.txt).  At 2 mod 32 the channels take 16 distinct banks and the producers'
// 4-byte stores (channel quads 8 banks apart) stay conflict-free: -6 ... -11 % on every launch; 6, 10, 18 mod 32 the same, an ODD
// pitch twice as slow (profiles/r6k_wgrad_ring_pitch_ab.txt).
constexpr int WG_RPAD = 8;              // bytes added to the 2304 of the rows of a channel plane
constexpr int XPITCH_R = 24;            // elements (2 bytes) per halo row of the ring image (18 used; a lane reads 5 dwords from byte 0 or 16)
constexpr int ZSLOT = WHY * XPITCH_R * 2;                  // bytes per ring plane inside a channel plane
constexpr int XPLANE_R = RZ * ZSLOT + WG_RPAD;
static_assert(XPITCH_R * 2 >= 36 && (XPLANE_R & 3) == 0 && (ZSLOT & 3) == 0, "a row holds 18 elements; dword-aligned planes");
constexpr int WGB_TPB = 512;
constexpr int MTWB = 2;                    // M tiles per wave (14 tiles over 8 waves)

__device__ __forceinline__ unsigned pack2(__bf16 lo, __bf16 hi) {
  return (unsigned)__builtin_bit_cast(unsigned short, lo) | ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
}

// ---- pieces shared by the two weight-gradient kernels -----------------------------------------------------------
// Tile dealing.  M-tile m = (kx group, slot): all 32 rows of a tile share the tap's x offset kx = m / TPK (the funnel
// shift is then wave-uniform); within the kx group the 9 (kz, ky) taps are packed TPT = 32 / CP per tile.  The three
// kx tiles of one slot read the SAME 20 bytes per lane and differ only in the shift, so with 8 tile groups and 5
// slots (CP = 16: 15 tiles) waves 0-4 take (slot w, kx 0) and (slot w, kx 1) -- one LDS read feeds both fragments --
// and waves 5-7 share out the five kx = 2 tiles.  Other shapes: round robin.
struct WgradTiles {
  int TPT, TPK, tile[MTWB], abase[MTWB], akx[MTWB];
  int akz[MTWB];                                  // ring layout: the lane's tap kz (abase then holds no z term)
  bool share_a;                                   // wave-uniform: tile 1 reuses tile 0's LDS words
};
__device__ __forceinline__ WgradTiles wgrad_deal_tiles(int CP, int MT, int TG, int tg, int li, int lh, bool ring = false) {
  WgradTiles w;
  w.TPT = 32 / CP;
  w.TPK = (9 + w.TPT - 1) / w.TPT;
  const bool paired = (TG == 8 && MT == 15);
  w.share_a = paired && tg < 5;
#pragma unroll
  for (int j = 0; j < MTWB; ++j) {
    int m = tg + TG * j;
    if (paired) {
      if (tg < 5) m = j * w.TPK + tg;                        // (kx = j, slot = tg)
      else { const int k = (tg - 5) * 2 + j; m = k < 5 ? 2 * w.TPK + k : MT; }   // (kx = 2, slot = k); k = 5: none
    }
    w.tile[j] = m;
    const int kx = m / w.TPK, slot = m - kx * w.TPK;
    const int t9 = slot * w.TPT + li / CP, c = li % CP;
    const bool valid = (m < MT) && (t9 < 9);
    const int kz = t9 / 3, ky = t9 % 3;
    w.abase[j] = valid ? (c * XPLANE + (kz * WHY + ky) * (XPITCH * 2) + 16 * lh) : (CP * XPLANE + 16 * lh);
    w.akz[j] = 0;
    if (ring) {      // the z offset is added per brick: ((ring base + row plane + kz) mod RZ) planes (the zero plane: any)
      w.abase[j] = valid ? (c * XPLANE_R + ky * (XPITCH_R * 2) + 16 * lh) : (CP * XPLANE_R + 16 * lh);
      w.akz[j] = valid ? kz : 0;
    }
    w.akx[j] = __builtin_amdgcn_readfirstlane(m < MT ? kx : 0);
  }
  return w;
}

// MFMA phase of one brick: one K16 step per brick row (z, y), this wave's k-split share of the rows
// MODE (wave-uniform, fixed for the life of the wave) specialises the funnel shift of the A fragments:
//   0  generic: any kx per tile, branch-free selects (8 VALU per fragment)
//   1  the paired dealing's waves 0-4: tile 0 is kx = 0 (the words as read), tile 1 is kx = 1 of the SAME words
//      (4 alignbyte); one LDS read feeds both
//   2  the paired dealing's waves 5-7: both tiles are kx = 2, a pure register renaming (no VALU)
template <int NT, int TERMS, int MODE = 0, bool AMP = false, bool RING = false>
__device__ __forceinline__ void wgrad_mfma_brick(const unsigned char* sXT, const unsigned char* sDT, int xt_bytes,
                                                 const WgradTiles& w, int ks, int KS, int li, int lh,
                                                 f32x16 (&acc)[MTWB][NT], int ring_base = 0) {
  constexpr int CO = 32 * NT;
  // the paired dealing implies CP = 16 and no k-split (KS = 1): the row loop is unrolled and every LDS offset but the
  // per-lane base is an instruction immediate
  if (MODE != 0) xt_bytes = 17 * (RING ? XPLANE_R : XPLANE);
  const unsigned char* sDTl = sDT + li * DPLANE + 16 * lh;
  // RING: the byte offset of ring plane (base + zz + kz) mod RZ, per tile and output plane zz of the brick (per lane: kz is)
  int zo[MTWB][WZ];
#pragma unroll
  for (int j = 0; j < MTWB; ++j)
#pragma unroll
    for (int z = 0; z < WZ; ++z) zo[j][z] = RING ? ((ring_base + z + w.akz[j]) & (RZ - 1)) * ZSLOT : 0;
  auto one_row = [&](int row) {
    const int zz = row / WY, yy = row - zz * WY;
    const int arow = RING ? yy * (XPITCH_R * 2) : (zz * WHY + yy) * (XPITCH * 2);
    const int brow = row * WX * 2;
    bf16x8 b[NT][TERMS];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q = 0; q < TERMS; ++q)
        b[t][q] = *reinterpret_cast<const bf16x8*>(sDTl + (q * CO + 32 * t) * DPLANE + brow);
    bf16x8 a[MTWB][TERMS];
    uint4 wq[TERMS];
    unsigned w4q[TERMS];
#pragma unroll
    for (int j = 0; j < MTWB; ++j) {
#pragma unroll
      for (int q = 0; q < TERMS; ++q) {
        if (MODE == 1 ? j == 0 : (MODE == 2 || j == 0 || !w.share_a)) {
          const unsigned char* p = sXT + q * xt_bytes + w.abase[j] + (RING ? zo[j][zz] : 0) + arow;
          if constexpr (RING) {
            // five dwords, read AS dwords (the ring's plane pitch is a multiple of 8, not of 16 bytes: see XPLANE_R)
            const unsigned* p32 = reinterpret_cast<const unsigned*>(p);
            wq[q] = make_uint4(p32[0], p32[1], p32[2], p32[3]);
            w4q[q] = p32[4];
          } else {
            wq[q] = *reinterpret_cast<const uint4*>(p);
            w4q[q] = *reinterpret_cast<const unsigned*>(p + 16);
          }
        }
        const uint4 v = wq[q];
        const unsigned v4 = w4q[q];
        if (MODE == 1) {
          uint4 r = v;
          if (j == 1) {
            r.x = __builtin_amdgcn_alignbyte(v.y, v.x, 2u);
            r.y = __builtin_amdgcn_alignbyte(v.z, v.y, 2u);
            r.z = __builtin_amdgcn_alignbyte(v.w, v.z, 2u);
            r.w = __builtin_amdgcn_alignbyte(v4, v.w, 2u);
          }
          a[j][q] = __builtin_bit_cast(bf16x8, r);
          continue;
        }
        if (MODE == 2) {
          uint4 r;
          r.x = v.y; r.y = v.z; r.z = v.w; r.w = v4;
          a[j][q] = __builtin_bit_cast(bf16x8, r);
          continue;
        }
        // branch-free funnel shift by the tile's (wave-uniform) tap x offset kx in {0, 1, 2} elements: kx = 2
        // selects the next dword as source, kx = 1 shifts by two bytes -- no control flow between the LDS reads,
        // so all fragment loads of a row are in flight together
        const bool k2 = w.akx[j] == 2;
        const unsigned sh = w.akx[j] == 1 ? 2u : 0u;
        uint4 r;
        r.x = __builtin_amdgcn_alignbyte(v.y, k2 ? v.y : v.x, sh);
        r.y = __builtin_amdgcn_alignbyte(v.z, k2 ? v.z : v.y, sh);
        r.z = __builtin_amdgcn_alignbyte(v.w, k2 ? v.w : v.z, sh);
        r.w = __builtin_amdgcn_alignbyte(v4, k2 ? v4 : v.w, sh);
        a[j][q] = __builtin_bit_cast(bf16x8, r);
      }
    }
#pragma unroll
    for (int j = 0; j < MTWB; ++j)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (TERMS == 3) {
          acc[j][t] = mfma16<TERMS>(a[j][2], b[t][0], acc[j][t]);
          acc[j][t] = mfma16<TERMS>(a[j][1], b[t][1], acc[j][t]);
          acc[j][t] = mfma16<TERMS>(a[j][0], b[t][2], acc[j][t]);
        }
        if constexpr (!AMP) {
          acc[j][t] = mfma16<TERMS>(a[j][1], b[t][0], acc[j][t]);
          acc[j][t] = mfma16<TERMS>(a[j][0], b[t][1], acc[j][t]);
        }
        acc[j][t] = mfma16<TERMS>(a[j][0], b[t][0], acc[j][t]);
      }
  };
  // (Round 6, measured and removed: the fragments of row r + 1 read into a second register set before row r's MFMAs -- the
  // compiler's own order is "rrLM rrrrLM ...", 33 lgkmcnt waits per 48 MFMAs; with the read-ahead 14, all counted (lgkmcnt(10..12))
  // -- changed no launch: 3.435 / 3.400 ms with / without at 16 -> 32, 2 x 256^3; N = 64 spills.  profiles/r6d_wgrad_readahead_ab.txt)
  if (MODE != 0) {
#pragma unroll
    for (int row = 0; row < WY * WZ; ++row) one_row(row);
  } else {
    for (int row = ks; row < WY * WZ; row += KS) one_row(row);
  }
}

// this wave's accumulators -> its partial slab (tap, ci, co)
template <int NT>
__device__ __forceinline__ void wgrad_store_partial(float* out, const WgradTiles& w, int MT, int CP, int ci0, int co0,
                                                    int Cin, int Cout, int li, int lh, const f32x16 (&acc)[MTWB][NT]) {
#pragma unroll
  for (int j = 0; j < MTWB; ++j) {
    const int m = w.tile[j];
    if (m >= MT) continue;
    const int kx = m / w.TPK, slot = m - kx * w.TPK;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int co = co0 + 32 * t + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const int t9 = slot * w.TPT + rr / CP, c = ci0 + rr % CP;
        const int tap = t9 * 3 + kx;             // (kz*3 + ky)*3 + kx
        if (t9 < 9 && c < Cin && co < Cout) out[((long long)tap * Cin + c) * Cout + co] = acc[j][t][r];
      }
    }
  }
}

template <int NT, int TERMS>
__global__ __launch_bounds__(WGB_TPB, 2) void conv3_wgrad_bf_kernel(
    const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ dz, const float* __restrict__ dzmask, float* __restrict__ partial, int N, int D,
    int H, int W, int Cin, int Cout, int relu_in, int CP, int MT, int TG, int KS, int ci_tiles, int tiles_x,
    int tiles_y, int tiles_z, int bricks_per_slab, int nslab_total, int Cmem /* channel stride of x in memory */,
    int ones_ch /* logical channel that reads as 1 inside the volume (-1: none) */,
    const float* __restrict__ xscale /* {S, 1/S} of x | NULL */, const float* __restrict__ dscale /* of dz | NULL */) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smemb[];
  constexpr int CO = 32 * NT;
  const int xt_bytes = (CP + 1) * XPLANE;                 // one term of sXT
  unsigned char* sXT = smemb;                             // [TERMS][(CP+1)][XPLANE]
  unsigned char* sDT = smemb + TERMS * xt_bytes;          // [TERMS][CO][DPLANE]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  // work item = (slab, (ci tile, cout group)) with the tile index fastest, XCD-remapped: the workgroups that
  // re-read the same bricks for different channel tiles run on the same XCD at the same time
  const int ntile = gridDim.x / nslab_total;
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  const int tile = item % ntile, slab = item / ntile;
  const int cit = tile % ci_tiles, cog = tile / ci_tiles;
  const int ci0 = cit * CP, co0 = cog * CO;
  const int tg = wv % TG, ks = wv / TG;

  const WgradTiles wt = wgrad_deal_tiles(CP, MT, TG, tg, li, lh);
  f32x16 acc[MTWB][NT];
#pragma unroll
  for (int j = 0; j < MTWB; ++j)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][t][r] = 0.f;

  // zero plane (padded M rows) of every term
  for (int e = tid; e < TERMS * (XPLANE / 4); e += WGB_TPB) {
    const int t = e / (XPLANE / 4), o = e - t * (XPLANE / 4);
    reinterpret_cast<unsigned*>(sXT + t * xt_bytes + CP * XPLANE)[o] = 0u;
  }
  // slabs never straddle samples (nslab_total = N * slabs per sample): the reduce kernel can then give per-sample sums
  const int slabs_per_n = nslab_total / N, bricks_in_n = tiles_x * tiles_y * tiles_z;
  const long long b_base = (long long)(slab / slabs_per_n) * bricks_in_n;
  const long long b_beg = b_base + (long long)(slab % slabs_per_n) * bricks_per_slab;
  long long b_end = b_beg + bricks_per_slab;
  if (b_end > b_base + bricks_in_n) b_end = b_base + bricks_in_n;
  const bool xvec = (CP >= 4) && ((Cin & 3) == 0) && (Cmem == Cin);
  const bool dvec = (Cout & 3) == 0;
  const int cq = CP >> 2;                 // channel quads per voxel (xvec)

  // ---- software pipeline over bricks: the global loads of brick b+1 are issued into registers before the
  //      MFMA phase of brick b and converted / transposed into LDS after it (1 workgroup per CU: nothing
  //      else would hide the HBM latency).  Item = 2 voxels x (4 channels | 1 channel).
  constexpr int XI = 2;                         // input-halo items per thread (24 rows x 9 pairs x <=4 quads = 864)
  constexpr int DI = (WV / 2) * (CO / 4) / WGB_TPB;   // dz items per thread (vector path): 2 (NT=2) or 1
  const int x_per_row = 9 * (xvec ? cq : CP);
  const int x_items = XROWS * x_per_row;
  float4 px[XI][2];
  float4 pd[DI > 0 ? DI : 1][2], pm[DI > 0 ? DI : 1][2];
  int pn = 0;                                   // sample index of the prefetched brick

  // per-thread staging descriptors (identical for every brick): computed once.  Global addresses are
  // (per-brick base pointer) + (precomputed 32-bit element offset relative to the brick origin).
  int xi_dz[XI], xi_dy[XI], xi_dx[XI], xi_cb[XI], xi_lds[XI], xi_rel[XI];
  bool xi_on[XI];
  const int HWs = H * W;
#pragma unroll
  for (int i = 0; i < XI; ++i) {
    const int e = tid + i * WGB_TPB;
    const int rowh = e / x_per_row, rem = e - rowh * x_per_row;
    const int cpart = rem / 9, pr = rem - cpart * 9;
    const int lz = rowh / WHY, ly = rowh - lz * WHY;
    xi_cb[i] = xvec ? 4 * cpart : cpart;
    xi_on[i] = (e < x_items) && (ci0 + xi_cb[i] < Cin);
    xi_dz[i] = lz - 1; xi_dy[i] = ly - 1; xi_dx[i] = 2 * pr - 1;
    xi_lds[i] = xi_cb[i] * XPLANE + (rowh * XPITCH + 2 * pr) * 2;
    xi_rel[i] = ((xi_dz[i] * H + xi_dy[i]) * W + xi_dx[i]) * Cmem + xi_cb[i];
  }
  constexpr int DIR = DI > 0 ? DI : 1;
  int di_dz[DIR], di_dy[DIR], di_dx[DIR], di_lds[DIR], di_rel[DIR];
  bool di_on[DIR];
#pragma unroll
  for (int i = 0; i < DI; ++i) {
    const int e = tid + i * WGB_TPB;
    // lanes: 4 consecutive cout quads (one 64-B global segment), then 64 voxel pairs, then quad groups
    const int q = (e & 3) + 4 * (e >> 8), pv = (e >> 2) & 63;
    const int lx = (pv % (WX / 2)) * 2, ly = (pv / (WX / 2)) % WY, lz = pv / ((WX / 2) * WY);
    di_dz[i] = lz; di_dy[i] = ly; di_dx[i] = lx;
    di_on[i] = co0 + 4 * q < Cout;
    di_lds[i] = (4 * q) * DPLANE + ((lz * WY + ly) * WX + lx) * 2;
    di_rel[i] = ((lz * H + ly) * W + lx) * Cout + 4 * q;
  }
  const float sX = xscale ? xscale[0] : 1.f, sD = dscale ? dscale[0] : 1.f;
  // normalisation coefficients of this thread's channels, reloaded only when the sample index changes
  float xsc[XI][4], xsh[XI][4];
  int coef_n = -1;
  auto load_coefs = [&](int n) {
    if (n == coef_n) return;
    coef_n = n;
#pragma unroll
    for (int i = 0; i < XI; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = ci0 + xi_cb[i] + j;
        const bool ok = scale && xi_on[i] && c < Cin && (xvec || j == 0);
        xsc[i][j] = (ok ? scale[n * Cin + c] : 1.f) * sX;      // power-of-two range scale folded in (exact)
        xsh[i][j] = (ok ? shift[n * Cin + c] : 0.f) * sX;
      }
  };
  const int bricks_per_n = tiles_x * tiles_y * tiles_z, tiles_xy = tiles_x * tiles_y;
  auto brick_coords = [&](long long bi64, int& n, int& x0, int& y0, int& z0) {
    const int bi = (int)bi64;                    // < 2^31 bricks by construction
    n = bi / bricks_per_n;
    const int r = bi - n * bricks_per_n;
    const int bz = r / tiles_xy, r2 = r - bz * tiles_xy;
    const int by = r2 / tiles_x, bx = r2 - by * tiles_x;
    x0 = bx * WX; y0 = by * WY; z0 = bz * WZ;
  };
  auto prefetch = [&](long long bi) {
    int n, x0, y0, z0;
    brick_coords(bi, n, x0, y0, z0);
    pn = n;
    const long long origin = (((long long)n * D + z0) * H + y0) * W + x0;     // wave-uniform
    const float* xb = x + origin * Cmem + ci0;
    const float* db = dz + origin * Cout + co0;
    const float* mb = dzmask ? dzmask + origin * Cout + co0 : nullptr;
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      px[i][0] = px[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
      const int gy = y0 + xi_dy[i], gz = z0 + xi_dz[i];
      if (xi_on[i] && (unsigned)gy < (unsigned)H && (unsigned)gz < (unsigned)D) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int gx = x0 + xi_dx[i] + u;
          if ((unsigned)gx < (unsigned)W) {
            if (xvec) px[i][u] = *reinterpret_cast<const float4*>(xb + xi_rel[i] + u * Cin);
            else px[i][u].x = (ci0 + xi_cb[i] == ones_ch) ? 1.f : xb[xi_rel[i] + u * Cmem];
          }
        }
      }
    }
    if (dvec) {
#pragma unroll
      for (int i = 0; i < DI; ++i) {
        const int gy = y0 + di_dy[i], gz = z0 + di_dz[i];
        const bool rok = di_on[i] && (gy < H) && (gz < D);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int gx = x0 + di_dx[i] + u;
          pd[i][u] = make_float4(0.f, 0.f, 0.f, 0.f);
          pm[i][u] = make_float4(1.f, 1.f, 1.f, 1.f);
          if (rok && gx < W) {
            pd[i][u] = *reinterpret_cast<const float4*>(db + di_rel[i] + u * Cout);
            if (mb) pm[i][u] = *reinterpret_cast<const float4*>(mb + di_rel[i] + u * Cout);
          }
        }
      }
    }
  };
  auto commit = [&](long long bi) {   // registers -> normalise / mask -> split -> transposed LDS images
    int n, x0, y0, z0;
    brick_coords(bi, n, x0, y0, z0);
    load_coefs(n);
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      if (xi_on[i]) {
        const int gy = y0 + xi_dy[i], gz = z0 + xi_dz[i];
        const bool rowok = (unsigned)gy < (unsigned)H && (unsigned)gz < (unsigned)D;
        const int nch = xvec ? 4 : 1;
        float v[2][4] = {{px[i][0].x, px[i][0].y, px[i][0].z, px[i][0].w}, {px[i][1].x, px[i][1].y, px[i][1].z, px[i][1].w}};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const bool ok = rowok && (unsigned)(x0 + xi_dx[i] + u) < (unsigned)W;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j < nch) {
              float t = v[u][j] * xsc[i][j] + xsh[i][j];     // identity coefficients when scale == NULL
              if (relu_in) t = fmaxf(t, 0.f);
              v[u][j] = ok ? t : 0.f;                        // zero padding AFTER the normalisation
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < nch) {
            float r0 = v[0][j], r1 = v[1][j];
#pragma unroll
            for (int t = 0; t < TERMS; ++t) {
              float b0, b1;
              const unsigned h0 = to16<TERMS>(r0, b0), h1 = to16<TERMS>(r1, b1);
              *reinterpret_cast<unsigned*>(sXT + t * xt_bytes + xi_lds[i] + j * XPLANE) = h0 | (h1 << 16);
              r0 -= b0; r1 -= b1;
            }
          }
        }
      }
    }
    if (dvec) {
#pragma unroll
      for (int i = 0; i < DI; ++i) {
        float v[2][4] = {{pd[i][0].x, pd[i][0].y, pd[i][0].z, pd[i][0].w}, {pd[i][1].x, pd[i][1].y, pd[i][1].z, pd[i][1].w}};
        const float m[2][4] = {{pm[i][0].x, pm[i][0].y, pm[i][0].z, pm[i][0].w}, {pm[i][1].x, pm[i][1].y, pm[i][1].z, pm[i][1].w}};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float r0 = (m[0][j] > 0.f) ? v[0][j] * sD : 0.f, r1 = (m[1][j] > 0.f) ? v[1][j] * sD : 0.f;
#pragma unroll
          for (int t = 0; t < TERMS; ++t) {
            float b0, b1;
            const unsigned h0 = to16<TERMS>(r0, b0), h1 = to16<TERMS>(r1, b1);
            *reinterpret_cast<unsigned*>(sDT + t * CO * DPLANE + di_lds[i] + j * DPLANE) = h0 | (h1 << 16);
            r0 -= b0; r1 -= b1;
          }
        }
      }
    } else {   // odd Cout: direct (unpipelined) scalar staging
      for (int e = tid; e < (WV / 2) * CO; e += WGB_TPB) {
        const int c = e % CO, pv = e / CO;
        const int lx = (pv % (WX / 2)) * 2, ly = (pv / (WX / 2)) % WY, lz = pv / ((WX / 2) * WY);
        const int gy = y0 + ly, gz = z0 + lz;
        float r[2] = {0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int gx = x0 + lx + u;
          if ((gx < W) & (gy < H) & (gz < D) & (co0 + c < Cout)) {
            const long long off = ((((long long)n * D + gz) * H + gy) * W + gx) * Cout + co0 + c;
            r[u] = (dzmask && !(dzmask[off] > 0.f)) ? 0.f : dz[off] * sD;
          }
        }
        const int vox = (lz * WY + ly) * WX + lx;
#pragma unroll
        for (int t = 0; t < TERMS; ++t) {
          float b0, b1;
          const unsigned h0 = to16<TERMS>(r[0], b0), h1 = to16<TERMS>(r[1], b1);
          *reinterpret_cast<unsigned*>(sDT + (t * CO + c) * DPLANE + vox * 2) = h0 | (h1 << 16);
          r[0] -= b0; r[1] -= b1;
        }
      }
    }
  };

  if (b_beg < b_end) prefetch(b_beg);
  for (long long bi = b_beg; bi < b_end; ++bi) {
    __syncthreads();            // previous brick's MFMA phase is done with the LDS images
    commit(bi);
    __syncthreads();
    if (bi + 1 < b_end) prefetch(bi + 1);
    wgrad_mfma_brick<NT, TERMS>(sXT, sDT, xt_bytes, wt, ks, KS, li, lh, acc);
  }
  wgrad_store_partial<NT>(partial + (((long long)slab * KS + ks) * 27) * Cin * Cout, wt, MT, CP, ci0, co0, Cin, Cout, li,
                          lh, acc);
}

// =============================================================================================
// Wave-specialised weight gradient (the vector path: Cin % 4 == 0, Cout % 4 == 0).  The kernel above needs ~235
// registers per lane, i.e. ONE 512-thread workgroup per CU, so its staging (global -> normalise -> split -> transposed
// LDS images) and its MFMA phase run back to back.  Here a 768-thread workgroup has 8 CONSUMER waves (the same tile
// dealing and MFMA loop, no staging registers) and 4 PRODUCER waves (one per SIMD) that stage brick b+1 into the
// other half of a double-buffered LDS image while the consumers multiply brick b: one raw s_barrier per brick, the
// producers' global loads for brick b+2 stay in flight across it (only LDS traffic is drained at the barrier).
constexpr int WS_CONS = 8;
// PW producer waves: 4 (one per SIMD, 3 waves per SIMD in all: 168 registers) or 8 (two per SIMD, 128 registers: the
// consumers of the unmasked N = 64 variant fit, and the producers -- the pole with 4 -- get twice the issue slots)

__device__ __forceinline__ void ws_barrier() {
  // LDS writes / reads of this wave are complete, outstanding GLOBAL loads are not waited for
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// DSPLIT (round 5): dz is the pre-split record tensor of kmh_maxpool3d_bwd_split -- (N, Cout/8, V + 1) records of 8 fp16 hi +
// 8 fp16 lo terms of fmaf(dz, S, 0) -- so a producer item (4 channels of two x neighbours) is four 8-byte loads and eight
// 16-bit packs instead of two 16-byte loads, eight multiplies and four split_pair sequences: the same words in the same
// transposed image, bit-identical sums.
// DSPARSE (round 7): dz is the POOLED gradient (N, D/2, H/2, W/2, Cout) fp32 and `dzmask` its winner bytes (one per pooled element,
// 0..7 = (dz, dy, dx)) -- the gradient of a convolution whose output feeds only a 2 x 2 x 2 max-pool has one non-zero per window and
// channel, so the dense tensor (7/8 zeros) is never formed.  The same item (4 channels of two x neighbours = the two dx children of
// one pooled cell at the item's (dz, dy)) is one 16-byte load of the cell's channel quad, one 4-byte load of its winners,
// fmaf(v, S, 0) and split_pair on 4 values; a child gets the words when the winner byte names it (compare-select, never an
// address term) and zeros otherwise: the words DSPLIT builds, bit for bit.  Even D, H, W.
template <int NT, int TERMS, bool MASK, int PW, bool DSPLIT = false, bool AMP = false, bool DSPARSE = false>
__global__ __launch_bounds__(64 * (WS_CONS + PW), (PW == 8 ? 4 : 3)) void conv3_wgrad_ws_kernel(
    const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ dz, const float* __restrict__ dzmask, float* __restrict__ partial, int N, int D,
    int H, int W, int Cin, int Cout, int relu_in, int CP, int MT, int TG, int KS, int ci_tiles, int tiles_x,
    int tiles_y, int tiles_z, int bricks_per_slab, int nslab_total, const float* __restrict__ xscale,
    const float* __restrict__ dscale, int dz_blocked /* dz is (N, Cout/8, D, H, W, 8) */) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smemb[];
  constexpr int CO = 32 * NT;
  // LDS: sXT[TERMS][CP+1][XPLANE_R] -- ONE ring image of RZ z planes (see XPLANE_R) -- then two stages of sDT[TERMS][CO][DPLANE]
  const int xt_bytes = (CP + 1) * XPLANE_R;               // one term of sXT
  constexpr int dt_bytes = TERMS * CO * DPLANE;           // one stage of sDT
  unsigned char* const sXTr = smemb;
  unsigned char* const sDT0 = smemb + TERMS * xt_bytes;
  constexpr int WS_TPB = 64 * (WS_CONS + PW), WS_PT = 64 * PW;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int ntile = gridDim.x / nslab_total;
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  const int tile = item % ntile, slab = item / ntile;
  const int cit = tile % ci_tiles, cog = tile / ci_tiles;
  const int ci0 = cit * CP, co0 = cog * CO;

  // zero plane (padded M rows) of every term: all RZ ring planes of it
  for (int e = tid; e < TERMS * (XPLANE_R / 4); e += WS_TPB) {
    const int t = e / (XPLANE_R / 4), o = e - t * (XPLANE_R / 4);
    reinterpret_cast<unsigned*>(sXTr + t * xt_bytes + CP * XPLANE_R)[o] = 0u;
  }
  // slabs never straddle samples (nslab_total = N * slabs per sample): the reduce kernel can then give per-sample sums
  const int bricks_per_n = tiles_x * tiles_y * tiles_z;
  const int slabs_per_n = nslab_total / N;
  const long long b_base = (long long)(slab / slabs_per_n) * bricks_per_n;
  const long long b_beg = b_base + (long long)(slab % slabs_per_n) * bricks_per_slab;
  long long b_end = b_beg + bricks_per_slab;
  if (b_end > b_base + bricks_per_n) b_end = b_base + bricks_per_n;
  if (b_beg >= b_end) return;                             // uniform over the workgroup
  auto brick_coords = [&](long long bi64, int& n, int& x0, int& y0, int& z0) {
    const int bi = (int)bi64;
    n = bi / bricks_per_n;
    const int r = bi - n * bricks_per_n;                   // z fastest: consecutive bricks share two halo planes
    const int col = r / tiles_z, bz = r - col * tiles_z;
    const int by = col / tiles_x, bx = col - by * tiles_x;
    x0 = bx * WX; y0 = by * WY; z0 = bz * WZ;
  };
  // ring base of a brick: + 2 planes per brick inside a z column, + 4 at the first brick of a column (which fills all four
  // planes of its window); producers and consumers advance it by the same rule
  const int cz_first = (int)((b_beg - b_base) % tiles_z);

  // (Round 6, measured and removed -- profiles/r6e_wgrad_prio_order_ab.txt: s_setprio 2 on the consumer waves: flat; on the
  // producer waves: 1-10 % slower (the consumers' stream is the critical path); term-major MFMA order over a row's
  // accumulators instead of three products of one accumulator back to back: flat.)
  if (wv >= WS_CONS) {
    // ------------------------------------------------------------------------------ producers
    const int pt = tid - 64 * WS_CONS;
    const int cq = CP >> 2;                               // channel quads per voxel
    const int x_per_row = 9 * cq;
    // x items of HALF a halo window (2 planes = 12 rows): set 0 = planes 2, 3 (the NEW planes of every brick), set 1 = planes
    // 0, 1 (fetched only by the first brick of a z column).  Same (ly, pair, channels) in both sets: lz differs by 2.
    const int x_items = 2 * WHY * x_per_row;              // <= 432
    constexpr int XH = (432 + WS_PT - 1) / WS_PT;         // items per thread and half: 1 (PW = 8) or 2
    constexpr int XI = 2 * XH;                            // register sets: [0, XH) = set 0, [XH, 2 XH) = set 1
    constexpr int DI = (WV / 2) * (CO / 4) / WS_PT;       // 4 (NT = 2) or 2
    int xi_pk[XI], xi_lds[XI];                     // pk = lz | ly << 4 | (2 pr) << 8 | cb << 16 | on << 30 (halo coords)
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int e = pt + (i % XH) * WS_PT;
      const int rowh = e / x_per_row, rem = e - rowh * x_per_row;
      const int cpart = rem / 9, pr = rem - cpart * 9;
      const int lzh = rowh / WHY, ly = rowh - lzh * WHY;
      const int lz = lzh + (i < XH ? 2 : 0);
      const int cb = 4 * cpart;
      const bool on = (e < x_items) && (ci0 + cb < Cin);
      xi_pk[i] = on ? (lz | (ly << 4) | ((2 * pr) << 8) | (cb << 16) | (1 << 30)) : 0;   // off: loads a valid dummy
      xi_lds[i] = cb * XPLANE_R + (ly * XPITCH_R + 2 * pr) * 2;                               // + the ring plane's ZSLOT, per brick
    }
    int di_pk[DI], di_lds[DI], di_q4[DI];
#pragma unroll
    for (int i = 0; i < DI; ++i) {
      const int e = pt + i * WS_PT;
      const int q = (e & 3) + 4 * (e >> 8), pv = (e >> 2) & 63;
      const int lx = (pv % (WX / 2)) * 2, ly = (pv / (WX / 2)) % WY, lz = pv / ((WX / 2) * WY);
      const bool on = co0 + 4 * q < Cout;
      di_pk[i] = lz | (ly << 4) | (lx << 8) | (on ? (1 << 30) : 0);
      di_lds[i] = (4 * q) * DPLANE + ((lz * WY + ly) * WX + lx) * 2;
      di_q4[i] = on ? 4 * q : 0;                          // off: loads a valid dummy, writes zeros
      // channel-blocked dz: element offset of the quad inside the sample = (chunk plane) + voxel * 8 + (quad in chunk)
      if (dz_blocked) di_q4[i] = on ? ((co0 + 4 * q) >> 3) * (D * H * W * 8) + ((4 * q) & 7) : 0;
      // pre-split records: planes of V + 1 records of 8 floats; the quad's four fp16 hi terms are floats (quad in chunk) / 2 ..
      // + 1 of the record, its lo terms 4 floats further
      if (DSPLIT) di_q4[i] = on ? ((co0 + 4 * q) >> 3) * ((D * H * W + 1) * 8) + (((4 * q) & 7) >> 1) : 0;
      if (DSPARSE) di_q4[i] = on ? co0 + 4 * q : 0;        // pooled cells are (.., Cout): the quad inside the cell
    }
    static_assert(!(DSPLIT && DSPARSE), "one operand source");
    const int dstride = (dz_blocked || DSPLIT) ? 8 : Cout;      // floats between x neighbours of one dz quad
    const float sX = xscale ? xscale[0] : 1.f, sD = dscale ? dscale[0] : 1.f;
    float4 px[XI][2], pd[DI][2], pm[MASK ? DI : 1][2];

    // Loads are unconditional: halo coordinates are clamped into the volume (the value is zeroed at conversion time
    // when the true coordinate was outside), so a brick's 16 (+8 mask) 16-byte loads per thread go out back to back.
    // Element offsets inside one sample are 24-bit multiply-adds (the launcher checks D*H*W*C < 2^31).
    auto issue = [&](int n, int x0, int y0, int z0, bool col_start) {
      const int xn_sets = col_start ? XI : XH;             // uniform: a column's first brick fetches all four planes
      const float* xn = x + (long long)n * D * H * W * Cin + ci0;
      const float* dn = DSPARSE ? dz + (long long)n * (D >> 1) * (H >> 1) * (W >> 1) * Cout
                      : DSPLIT ? dz + (long long)n * (Cout >> 3) * ((long long)D * H * W + 1) * 8
                               : dz + (long long)n * D * H * W * Cout + (dz_blocked ? 0 : co0);
      const float* mn = MASK ? dzmask + (long long)n * D * H * W * Cout + co0 : nullptr;
      // all element offsets first, then the loads back to back
      unsigned xo[XI][2], dO[DI][2];
#pragma unroll
      for (int i = 0; i < XI; ++i) {
        if (i >= xn_sets) break;
        const int gz = min(max(z0 + (xi_pk[i] & 15) - 1, 0), D - 1), gy = min(max(y0 + ((xi_pk[i] >> 4) & 15) - 1, 0), H - 1);
        const int gx0 = x0 + ((xi_pk[i] >> 8) & 255) - 1, cb = (xi_pk[i] >> 16) & 255;
        const unsigned row = __umul24(__umul24(gz, H) + gy, W);
        xo[i][0] = __umul24(row + min(max(gx0, 0), W - 1), Cin) + cb;
        xo[i][1] = __umul24(row + min(max(gx0 + 1, 0), W - 1), Cin) + cb;
      }
#pragma unroll
      for (int i = 0; i < DI; ++i) {
        const int gz = min(z0 + (di_pk[i] & 15), D - 1), gy = min(y0 + ((di_pk[i] >> 4) & 15), H - 1);
        const int gx0 = x0 + ((di_pk[i] >> 8) & 255);
        const unsigned row = __umul24(__umul24(gz, H) + gy, W);
        dO[i][0] = __umul24(row + min(gx0, W - 1), dstride) + di_q4[i];
        dO[i][1] = __umul24(row + min(gx0 + 1, W - 1), dstride) + di_q4[i];
        if (DSPARSE)       // the pooled cell of the pair (clamped into the volume as above); [1] is not used
          dO[i][0] = __umul24(__umul24(__umul24(gz >> 1, H >> 1) + (gy >> 1), W >> 1) + (min(gx0, W - 1) >> 1), Cout) + di_q4[i];
      }
#pragma unroll
      for (int i = 0; i < XI; ++i) {
        if (i >= xn_sets) break;
        px[i][0] = *reinterpret_cast<const float4*>(xn + xo[i][0]);
        px[i][1] = *reinterpret_cast<const float4*>(xn + xo[i][1]);
      }
#pragma unroll
      for (int i = 0; i < DI; ++i) {
        if constexpr (DSPARSE) {       // the cell's channel quad and its four winner bytes (the same element offset, in bytes)
          pd[i][0] = *reinterpret_cast<const float4*>(dn + dO[i][0]);
          const unsigned char* wn = reinterpret_cast<const unsigned char*>(dzmask) + (long long)n * (D >> 1) * (H >> 1) * (W >> 1) * Cout;
          pd[i][1] = make_float4(__uint_as_float(*reinterpret_cast<const unsigned*>(wn + dO[i][0])), 0.f, 0.f, 0.f);
          continue;
        }
        if constexpr (DSPLIT) {        // (hi.x, hi.y, lo.x, lo.y): 4 + 4 fp16 terms of the voxel's channel quad
          const float2 h0 = *reinterpret_cast<const float2*>(dn + dO[i][0]), l0 = *reinterpret_cast<const float2*>(dn + dO[i][0] + 4);
          const float2 h1 = *reinterpret_cast<const float2*>(dn + dO[i][1]), l1 = *reinterpret_cast<const float2*>(dn + dO[i][1] + 4);
          pd[i][0] = make_float4(h0.x, h0.y, l0.x, l0.y);
          pd[i][1] = make_float4(h1.x, h1.y, l1.x, l1.y);
          continue;
        }
        pd[i][0] = *reinterpret_cast<const float4*>(dn + dO[i][0]);
        pd[i][1] = *reinterpret_cast<const float4*>(dn + dO[i][1]);
        if (MASK) {
          pm[i][0] = *reinterpret_cast<const float4*>(mn + dO[i][0]);
          pm[i][1] = *reinterpret_cast<const float4*>(mn + dO[i][1]);
        }
      }
    };
    // (n, channel) normalisation coefficients of this workgroup's CP channels, pre-multiplied by the range scale:
    // a small LDS table behind the two stages, rewritten (by every producer wave for itself: LDS operations of one
    // wave are ordered, and the waves write identical values) when the sample index changes
    float* ctab = reinterpret_cast<float*>(sDT0 + 2 * dt_bytes);
    int tab_n = -1;
    const float relu_lo = relu_in ? 0.f : -INFINITY;
    // Keeps every use of the staged registers behind the barrier: register-only work may otherwise be hoisted above
    // the (volatile, but not register-clobbering) barrier statement, and the wait for the loads with it.
    auto pin = [](float4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); };
    auto convert = [&](int n, int x0, int y0, int z0, unsigned char* sXT, unsigned char* sDT, int ring_base, bool col_start) {
      const int xn_sets = col_start ? XI : XH;
      if (n != tab_n) {
        tab_n = n;
        if (lane < 2 * CP) {
          const int c = ci0 + (lane % CP);
          float v = lane < CP ? sX : 0.f;
          if (scale && c < Cin) v = (lane < CP ? scale[(long long)n * Cin + c] : shift[(long long)n * Cin + c]) * sX;
          ctab[lane] = v;
        }
      }
#pragma unroll
      for (int i = 0; i < XI; ++i) {
        if (i >= xn_sets) break;
        const int zdst = ((ring_base + (xi_pk[i] & 15)) & (RZ - 1)) * ZSLOT;      // this halo plane's place in the ring
        const int gz = z0 + (xi_pk[i] & 15) - 1, gy = y0 + ((xi_pk[i] >> 4) & 15) - 1;
        const int gx0 = x0 + ((xi_pk[i] >> 8) & 255) - 1, cb = (xi_pk[i] >> 16) & 255;
        const bool rowok = (unsigned)gy < (unsigned)H && (unsigned)gz < (unsigned)D;
        const float4 sc4 = *reinterpret_cast<const float4*>(ctab + cb);
        const float4 sh4 = *reinterpret_cast<const float4*>(ctab + CP + cb);
        const float sc[4] = {sc4.x, sc4.y, sc4.z, sc4.w}, sh[4] = {sh4.x, sh4.y, sh4.z, sh4.w};
        float v[2][4] = {{px[i][0].x, px[i][0].y, px[i][0].z, px[i][0].w}, {px[i][1].x, px[i][1].y, px[i][1].z, px[i][1].w}};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const bool ok = rowok && (unsigned)(gx0 + u) < (unsigned)W;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float t = fmaxf(v[u][j] * sc[j] + sh[j], relu_lo);
            v[u][j] = ok ? t : 0.f;                        // zero padding AFTER the normalisation
          }
        }
        if (xi_pk[i] >> 30) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            unsigned w[TERMS];
            split_pair<TERMS>(v[0][j], v[1][j], w);
#pragma unroll
            for (int t = 0; t < TERMS; ++t)
              *reinterpret_cast<unsigned*>(sXT + t * xt_bytes + xi_lds[i] + zdst + j * XPLANE_R) = w[t];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < DI; ++i) {
        const int gz = z0 + (di_pk[i] & 15), gy = y0 + ((di_pk[i] >> 4) & 15), gx0 = x0 + ((di_pk[i] >> 8) & 255);
        const bool rok = (di_pk[i] >> 30) && gy < H && gz < D;
        if constexpr (DSPARSE) {
          static_assert(!DSPARSE || (TERMS == 2 && !MASK), "the pooled operand is split into fp16 hi / lo, already masked");
          const bool k0 = rok && gx0 < W;                    // even W: both x neighbours are inside, or neither
          const unsigned kk = ((di_pk[i] & 1) << 2) | (((di_pk[i] >> 4) & 1) << 1);      // window index of the dx = 0 child (even brick origins)
          const unsigned wb = __float_as_uint(pd[i][1].x);
          unsigned w01[2], w23[2];
          split_pair<2>(fmaf(pd[i][0].x, sD, 0.f), fmaf(pd[i][0].y, sD, 0.f), w01);
          split_pair<2>(fmaf(pd[i][0].z, sD, 0.f), fmaf(pd[i][0].w, sD, 0.f), w23);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const unsigned a = (wb >> (8 * j)) & 255u;
            const bool m0 = k0 && a == kk, m1 = k0 && a == kk + 1;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              const unsigned pr = j < 2 ? w01[t] : w23[t];
              const unsigned h16 = (j & 1) ? pr >> 16 : pr & 0xffffu;
              const unsigned wd = m0 ? h16 : (m1 ? h16 << 16 : 0u);
              *reinterpret_cast<unsigned*>(sDT + t * CO * DPLANE + di_lds[i] + j * DPLANE) = wd;
            }
          }
          continue;
        }
        if constexpr (DSPLIT) {
          // words of the transposed image: (voxel 0 | voxel 1 << 16) per channel and term
          static_assert(TERMS == 2 && !MASK, "pre-split records are fp16 hi / lo, already masked");
          const bool k0 = rok && gx0 < W, k1 = rok && gx0 + 1 < W;
          unsigned a[4] = {__float_as_uint(pd[i][0].x), __float_as_uint(pd[i][0].y), __float_as_uint(pd[i][0].z), __float_as_uint(pd[i][0].w)};
          unsigned b[4] = {__float_as_uint(pd[i][1].x), __float_as_uint(pd[i][1].y), __float_as_uint(pd[i][1].z), __float_as_uint(pd[i][1].w)};
#pragma unroll
          for (int u = 0; u < 4; ++u) { a[u] = k0 ? a[u] : 0u; b[u] = k1 ? b[u] : 0u; }
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const unsigned av = a[2 * t + (j >> 1)], bv = b[2 * t + (j >> 1)];
              const unsigned wd = (j & 1) ? ((av >> 16) | (bv & 0xffff0000u)) : ((av & 0xffffu) | (bv << 16));
              *reinterpret_cast<unsigned*>(sDT + t * CO * DPLANE + di_lds[i] + j * DPLANE) = wd;
            }
          continue;
        }
        float v[2][4] = {{pd[i][0].x, pd[i][0].y, pd[i][0].z, pd[i][0].w}, {pd[i][1].x, pd[i][1].y, pd[i][1].z, pd[i][1].w}};
        float m[2][4] = {{1.f, 1.f, 1.f, 1.f}, {1.f, 1.f, 1.f, 1.f}};
        if (MASK) {
          m[0][0] = pm[i][0].x; m[0][1] = pm[i][0].y; m[0][2] = pm[i][0].z; m[0][3] = pm[i][0].w;
          m[1][0] = pm[i][1].x; m[1][1] = pm[i][1].y; m[1][2] = pm[i][1].z; m[1][3] = pm[i][1].w;
        }
        const bool ok0 = rok && gx0 < W, ok1 = rok && gx0 + 1 < W;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float r0 = (ok0 && m[0][j] > 0.f) ? v[0][j] * sD : 0.f, r1 = (ok1 && m[1][j] > 0.f) ? v[1][j] * sD : 0.f;
          unsigned w[TERMS];
          split_pair<TERMS>(r0, r1, w);
#pragma unroll
          for (int t = 0; t < TERMS; ++t)
            *reinterpret_cast<unsigned*>(sDT + t * CO * DPLANE + di_lds[i] + j * DPLANE) = w[t];
        }
      }
    };

    // brick coordinates advance incrementally (z fastest, then x, y; a slab stays inside one sample): no divisions in the loop
    int cn, cx, cy, cz;
    {
      int x0, y0, z0;
      brick_coords(b_beg, cn, x0, y0, z0);
      cx = x0 / WX; cy = y0 / WY; cz = z0 / WZ;
    }
    int rbase = 0;                                        // ring base of the brick whose loads are in flight
    bool cstart = true;                                   // ... and whether it is the first of its column (here: of the slab)
    issue(cn, cx * WX, cy * WY, cz * WZ, true);
    for (long long bi = b_beg; bi < b_end; ++bi) {
      unsigned char* sDTs = sDT0 + ((bi - b_beg) & 1) * dt_bytes;
      const int pn = cn, px0 = cx * WX, py0 = cy * WY, pz0 = cz * WZ;      // the brick whose loads are in flight
      const int pbase = rbase;
      const bool pstart = cstart;
      cstart = false;
      if (++cz == tiles_z) { cz = 0; cstart = true; if (++cx == tiles_x) { cx = 0; if (++cy == tiles_y) { cy = 0; ++cn; } } }
      rbase = (rbase + (cstart ? 4 : 2)) & (RZ - 1);
#pragma unroll
      for (int i = 0; i < XI; ++i) { pin(px[i][0]); pin(px[i][1]); }
#pragma unroll
      for (int i = 0; i < DI; ++i) {
        pin(pd[i][0]); pin(pd[i][1]);
        if (MASK) { pin(pm[i][0]); pin(pm[i][1]); }
      }
      convert(pn, px0, py0, pz0, sXTr, sDTs, pbase, pstart);                 // waits for the loads of brick bi only
      if (bi + 1 < b_end) issue(cn, cx * WX, cy * WY, cz * WZ, cstart);      // in flight across the barrier
      ws_barrier();
    }
    return;
  }

  // -------------------------------------------------------------------------------- consumers
  const int tg = wv % TG, ks = wv / TG;
  const WgradTiles wt = wgrad_deal_tiles(CP, MT, TG, tg, li, lh, true);
  f32x16 acc[MTWB][NT];
#pragma unroll
  for (int j = 0; j < MTWB; ++j)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][t][r] = 0.f;

  ws_barrier();                                            // brick b_beg is staged (and the zero planes written)
  auto bricks = [&](auto mode) {
    int rbase = 0, cz = cz_first;                           // as the producers count them
    for (long long bi = b_beg; bi < b_end; ++bi) {
      const unsigned char* sDT = sDT0 + ((bi - b_beg) & 1) * dt_bytes;
      wgrad_mfma_brick<NT, TERMS, decltype(mode)::value, AMP, true>(sXTr, sDT, xt_bytes, wt, ks, KS, li, lh, acc, rbase);
      const bool nstart = ++cz == tiles_z;
      if (nstart) cz = 0;
      rbase = (rbase + (nstart ? 4 : 2)) & (RZ - 1);
      if (bi + 1 < b_end) ws_barrier();                    // brick bi+1 is staged: its ring planes and the other sDT stage
    }
  };
  // the paired dealing (CP = 16) fixes every wave's tap x offsets: waves 0-4 hold (kx 0, kx 1) of one slot, waves
  // 5-7 two kx = 2 tiles (an absent sixth one reads the zero plane, whatever its shift)
  if (TG == 8 && MT == 15) {
    if (tg < 5) bricks(std::integral_constant<int, 1>{});
    else bricks(std::integral_constant<int, 2>{});
  } else {
    bricks(std::integral_constant<int, 0>{});
  }
  wgrad_store_partial<NT>(partial + (((long long)slab * KS + ks) * 27) * Cin * Cout, wt, MT, CP, ci0, co0, Cin, Cout, li,
                          lh, acc);
}

__global__ __launch_bounds__(256) void wgrad_bf_reduce_kernel(const float* __restrict__ partial, int nslab, int Cin,
                                                              int Cout, float* __restrict__ dw, int accumulate,
                                                              const float* __restrict__ xscale,
                                                              const float* __restrict__ dscale) {
  const double desc = (double)(xscale ? xscale[1] : 1.f) * (double)(dscale ? dscale[1] : 1.f);
  const long long total = (long long)27 * Cin * Cout;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    double s = 0;
    for (int k = 0; k < nslab; ++k) s += partial[(long long)k * total + e];
    const int co = (int)(e % Cout), ci = (int)((e / Cout) % Cin), tap = (int)(e / ((long long)Cout * Cin));
    const long long o = ((long long)co * Cin + ci) * 27 + tap;
    dw[o] = accumulate ? dw[o] + (float)(s * desc) : (float)(s * desc);
  }
}

// Reduce + fold: dw as above, and, from the PER-SAMPLE sums the slab order allows,
//   bhat[n][ci] = sum_{tap, co} w[co][ci][tap] * dWn[n][tap][ci][co]  =  sum_v dxn[n][v][ci] * xhat[n][v][ci]
// (dxn = the data gradient of the same dz, xhat = the convolution's input): GroupNorm's second backward statistic
// without a pass over dxn and x.  Block = (ci, tap triple); bhat must be zero on entry.
// 1024 threads = LP columns (the next power of two >= 3 Cout, capped at 1024) x S = 1024 / LP slices of the slabs: the
// slab sums are strided reads 27 Cin Cout floats apart, and one thread walking all of them ran at 1.1 TB/s.
__global__ __launch_bounds__(1024) void wgrad_bf_reduce_fold_kernel(const float* __restrict__ partial, int N, int per_n,
                                                                    int Cin, int Cout, float* __restrict__ dw,
                                                                    int accumulate, const float* __restrict__ xscale,
                                                                    const float* __restrict__ dscale,
                                                                    const float* __restrict__ w,
                                                                    double* __restrict__ bhat, int LP) {
  const double desc = (double)(xscale ? xscale[1] : 1.f) * (double)(dscale ? dscale[1] : 1.f);
  const long long total = (long long)27 * Cin * Cout;
  const int ci = blockIdx.x, t3 = blockIdx.y;
  __shared__ double red[1024];
  __shared__ double wred[1024 / kWave];
  const int S = 1024 / LP, lcol = threadIdx.x % LP, sl = threadIdx.x / LP;
  const int L = 3 * Cout;
  for (int l0 = 0; l0 < L; l0 += LP) {                      // (one pass unless 3 Cout > 1024)
    const int l = l0 + lcol;
    const bool act = l < L;
    const int tap = 3 * t3 + (act ? l / Cout : 0), co = act ? l % Cout : 0;
    const long long e = ((long long)tap * Cin + ci) * Cout + co;
    const long long o = ((long long)co * Cin + ci) * 27 + tap;
    const double wv = act ? (double)w[o] : 0.0;
    double tot = 0;
    for (int n = 0; n < N; ++n) {
      double sn = 0;
      if (act)
        for (int k = sl; k < per_n; k += S) sn += partial[((long long)n * per_n + k) * total + e];
      __syncthreads();
      red[threadIdx.x] = sn;
      __syncthreads();
      double bn = 0;
      if (sl == 0 && act) {
        sn = 0;
        for (int q = 0; q < S; ++q) sn += red[q * LP + lcol];      // fixed order
        tot += sn;
        bn = wv * sn * desc;
      }
      const double r = block_sum<double>(bn, wred);
      if (threadIdx.x == 0) atomicAdd(bhat + (long long)n * Cin + ci, r);
    }
    if (sl == 0 && act) dw[o] = accumulate ? dw[o] + (float)(tot * desc) : (float)(tot * desc);
  }
}

struct WgradBfPlan {
  int CP, MT, TG, KS, ci_tiles, co_groups, NT, tiles_x, tiles_y, tiles_z, nslab, bricks_per_slab;
  long long nbricks;
  size_t lds;        // one stage of conv3_wgrad_bf_kernel
  size_t lds_ws;     // conv3_wgrad_ws_kernel: the ring x image + two dz stages + the coefficient table
};

static WgradBfPlan wgrad_bf_plan(int N, int D, int H, int W, int Cin, int Cout, int terms) {
  WgradBfPlan p;
  p.CP = 1;
  while (p.CP < Cin && p.CP < 16) p.CP <<= 1;
  p.ci_tiles = (Cin + p.CP - 1) / p.CP;
  {
    const int tpt = 32 / p.CP;
    p.MT = 3 * ((9 + tpt - 1) / tpt);            // uniform-kx tiles: 15 (CP=16), 9, 6, 3, 3
  }
  p.TG = 1;
  while (p.TG < 8 && p.TG < p.MT) p.TG <<= 1;
  p.KS = 8 / p.TG;
  p.NT = Cout > 32 ? 2 : 1;
  p.co_groups = (Cout + 32 * p.NT - 1) / (32 * p.NT);
  p.tiles_x = (W + WX - 1) / WX; p.tiles_y = (H + WY - 1) / WY; p.tiles_z = (D + WZ - 1) / WZ;
  p.nbricks = (long long)N * p.tiles_x * p.tiles_y * p.tiles_z;
  // ~768 workgroups in all; a slab is a run of bricks of ONE sample
  const long long bricks_per_n = (long long)p.tiles_x * p.tiles_y * p.tiles_z;
  long long want = 768 / ((long long)p.ci_tiles * p.co_groups * N);
  if (want < 1) want = 1;
  if (want > bricks_per_n) want = bricks_per_n;
  p.bricks_per_slab = (int)((bricks_per_n + want - 1) / want);
  p.nslab = N * (int)((bricks_per_n + p.bricks_per_slab - 1) / p.bricks_per_slab);
  p.lds = (size_t)terms * ((size_t)(p.CP + 1) * XPLANE + (size_t)32 * p.NT * DPLANE);
  p.lds_ws = (size_t)terms * ((size_t)(p.CP + 1) * XPLANE_R + 2 * (size_t)32 * p.NT * DPLANE) + 256;
  return p;
}

template <int NT, int TERMS>
static int launch_wgrad_bf(const WgradBfPlan& p, const float* x, const float* scale, const float* shift,
                           const float* dz, const float* dzmask, float* ws, int N, int D, int H, int W, int Cin,
                           int Cout, int relu_in, int Cmem, int ones_ch, const float* xscale, const float* dscale,
                           hipStream_t s) {
  hipError_t e = hipFuncSetAttribute((const void*)conv3_wgrad_bf_kernel<NT, TERMS>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
  if (e != hipSuccess) return (int)e;
  dim3 g(p.ci_tiles * p.co_groups * p.nslab);
  conv3_wgrad_bf_kernel<NT, TERMS><<<g, WGB_TPB, p.lds, s>>>(x, scale, shift, dz, dzmask, ws, N, D, H, W, Cin, Cout,
                                                            relu_in, p.CP, p.MT, p.TG, p.KS, p.ci_tiles, p.tiles_x,
                                                            p.tiles_y, p.tiles_z, p.bricks_per_slab, p.nslab, Cmem,
                                                            ones_ch, xscale, dscale);
  return KMH_LAUNCH_CHECK();
}

template <int NT, int TERMS, bool MASK, int PW, bool DSPLIT = false, bool DSPARSE = false>
static int launch_wgrad_ws(const WgradBfPlan& p, const float* x, const float* scale, const float* shift,
                           const float* dz, const float* dzmask, float* ws, int N, int D, int H, int W, int Cin,
                           int Cout, int relu_in, const float* xscale, const float* dscale, int dz_blocked, hipStream_t s,
                           bool amp) {
  const size_t lds = p.lds_ws;                             // ring x image, two dz stages, the coefficient table
  hipError_t e = hipFuncSetAttribute((const void*)conv3_wgrad_ws_kernel<NT, TERMS, MASK, PW, DSPLIT, false, DSPARSE>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return (int)e;
  dim3 g(p.ci_tiles * p.co_groups * p.nslab);
  if constexpr (!MASK && PW == 8 && !DSPARSE) {      // (the pooled operand is not served under use_amp)
    if (amp) {
      e = hipFuncSetAttribute((const void*)conv3_wgrad_ws_kernel<NT, TERMS, MASK, PW, DSPLIT, true>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
      conv3_wgrad_ws_kernel<NT, TERMS, MASK, PW, DSPLIT, true><<<g, 64 * (WS_CONS + PW), lds, s>>>(
          x, scale, shift, dz, dzmask, ws, N, D, H, W, Cin, Cout, relu_in, p.CP, p.MT, p.TG, p.KS, p.ci_tiles, p.tiles_x, p.tiles_y,
          p.tiles_z, p.bricks_per_slab, p.nslab, xscale, dscale, dz_blocked);
      return KMH_LAUNCH_CHECK();
    }
  }
  conv3_wgrad_ws_kernel<NT, TERMS, MASK, PW, DSPLIT, false, DSPARSE><<<g, 64 * (WS_CONS + PW), lds, s>>>(x, scale, shift, dz, dzmask, ws, N, D, H, W, Cin, Cout,
                                                               relu_in, p.CP, p.MT, p.TG, p.KS, p.ci_tiles, p.tiles_x,
                                                               p.tiles_y, p.tiles_z, p.bricks_per_slab, p.nslab, xscale,
                                                               dscale, dz_blocked);
  return KMH_LAUNCH_CHECK();
}

}  // namespace

// the wave-specialised kernel's preconditions (vector path of the f16x3 mode)
static bool wgrad_ws_ok(const WgradBfPlan& p, int D, int H, int W, int Cin, int Cout, int terms) {
  return terms == 2 && p.CP >= 4 && (Cin & 3) == 0 && (Cout & 3) == 0 && p.lds_ws <= 160 * 1024 &&
         (long long)D * H * W * (Cin > Cout ? Cin : Cout) < (1ll << 31) &&
         (long long)D * H * W <= (1ll << 24);   // 24-bit multiply-adds index the voxels of one sample
}

/* 1 when kmh_conv3d_wgrad_bf accepts a channel-blocked dz, (N, Cout/8, D, H, W, 8), for this shape */
KMH_API int kmh_conv3d_wgrad_bf_blocked_ok(int N, int D, int H, int W, int Cin, int Cout, int terms) {
  const WgradBfPlan p = wgrad_bf_plan(N, D, H, W, Cin, Cout, terms);
  return (Cout & 7) == 0 && wgrad_ws_ok(p, D, H, W, Cin, Cout, terms) ? 1 : 0;
}

KMH_API size_t kmh_conv3d_wgrad_bf_ws_bytes(int N, int D, int H, int W, int Cin, int Cout, int terms) {
  const WgradBfPlan p = wgrad_bf_plan(N, D, H, W, Cin, Cout, terms);
  return (size_t)p.nslab * p.KS * 27 * Cin * Cout * sizeof(float);
}

/* append_ones != 0: x has Cin-1 real channels in memory and a virtual last channel that reads 1 inside the volume
 * (0 in the zero padding); dw then has Cin logical input channels.  With scale == NULL this yields, per output
 * channel and tap, R = sum_v x[v+tap] dz[v] and S = sum_v [v+tap inside] dz[v] in ONE pass. */
/* 1 when kmh_conv3d_wgrad_bf_sparse serves this shape: the wave-specialised kernel's preconditions (as for a channel-blocked dz),
 * even D, H, W, the f16x3 arithmetic (terms == 2; not the one-product use_amp arithmetic, terms == 1). */
KMH_API int kmh_conv3d_wgrad_bf_sparse_ok(int N, int D, int H, int W, int Cin, int Cout, int terms) {
  if (N <= 0 || terms != 2 || ((D | H | W) & 1) || D < 2 || H < 2 || W < 2) return 0;
  return kmh_conv3d_wgrad_bf_blocked_ok(N, D, H, W, Cin, Cout, terms);
}

/* dz_kind: 0 dense, 1 channel-blocked, 2 pre-split records, 3 = dz is the POOLED gradient (N, D/2, H/2, W/2, Cout) and `winners`
 * its window indices (kmh_conv3d_wgrad_bf_sparse) */
static int wgrad_bf_impl(const float* x, const float* scale, const float* shift, const float* dz,
                         const float* dzmask, float* dw, int N, int D, int H, int W, int Cin, int Cout,
                         int relu_in, int accumulate, int terms, int append_ones, const float* xscale,
                         const float* dscale, int dz_blocked, const unsigned char* winners, const float* w_fold, double* bhat,
                         void* ws, void* stream) {
  const bool amp = kmh_take_amp(terms);      // terms == 1: the fp16 kernels with hi x hi only (use_amp), for this call
  hipStream_t s = (hipStream_t)stream;
  if ((w_fold == nullptr) != (bhat == nullptr)) return -22;
  const WgradBfPlan p = wgrad_bf_plan(N, D, H, W, Cin, Cout, terms);
  if (dz_blocked == 3 && (amp || dzmask || append_ones || !winners || !xscale || !dscale ||
                          ((uintptr_t)dz & 15) || ((uintptr_t)winners & 3) || !kmh_conv3d_wgrad_bf_sparse_ok(N, D, H, W, Cin, Cout, terms)))
    return -22;
  if (dz_blocked && (dzmask || !kmh_conv3d_wgrad_bf_blocked_ok(N, D, H, W, Cin, Cout, terms))) return -22;
  if (dz_blocked == 2 && (terms != 2 || ((long long)D * H * W + 1) * (Cout > Cin ? Cout : Cin) >= (1ll << 31))) return -22;
  if (p.MT > p.TG * MTWB || (terms != 2 && terms != 3)) return -22;
  const int Cmem = append_ones ? Cin - 1 : Cin, ones_ch = append_ones ? Cin - 1 : -1;
  if (append_ones && (scale || Cin > 4)) return -22;
  int rc;
  if (terms == 2 && (!xscale || !dscale)) return -22;      // fp16 split without range scaling is not accurate
#define KMH_WG_CALL(NT_, T_) launch_wgrad_bf<NT_, T_>(p, x, scale, shift, dz, dzmask, (float*)ws, N, D, H, W, Cin, Cout, relu_in, Cmem, ones_ch, xscale, dscale, s)
  // wave-specialised kernel (producer / consumer waves, double-buffered LDS): vector path of the f16x3 mode
  const bool ws_ok = wgrad_ws_ok(p, D, H, W, Cin, Cout, terms) && !append_ones;
  // (8 producer waves without a mask operand, 4 with one)
#define KMH_WS_CALL(NT_, M_, PW_) launch_wgrad_ws<NT_, 2, M_, PW_>(p, x, scale, shift, dz, dzmask, (float*)ws, N, D, H, W, Cin, Cout, relu_in, xscale, dscale, dz_blocked, s, amp)
  if (dz_blocked == 3) {               // the pooled gradient and its winner bytes (the winners travel in the mask operand's place)
    if (!ws_ok) return -22;
    const float* wn = reinterpret_cast<const float*>(winners);
    rc = p.NT == 2 ? launch_wgrad_ws<2, 2, false, 8, false, true>(p, x, scale, shift, dz, wn, (float*)ws, N, D, H, W, Cin, Cout, relu_in, xscale, dscale, 0, s, amp)
                   : launch_wgrad_ws<1, 2, false, 8, false, true>(p, x, scale, shift, dz, wn, (float*)ws, N, D, H, W, Cin, Cout, relu_in, xscale, dscale, 0, s, amp);
  } else if (ws_ok && dz_blocked == 2) {      // pre-split dz records (kmh_maxpool3d_bwd_split)
    rc = p.NT == 2 ? launch_wgrad_ws<2, 2, false, 8, true>(p, x, scale, shift, dz, nullptr, (float*)ws, N, D, H, W, Cin, Cout, relu_in, xscale, dscale, 0, s, amp)
                   : launch_wgrad_ws<1, 2, false, 8, true>(p, x, scale, shift, dz, nullptr, (float*)ws, N, D, H, W, Cin, Cout, relu_in, xscale, dscale, 0, s, amp);
  } else if (ws_ok) {
    if (p.NT == 2) rc = dzmask ? KMH_WS_CALL(2, true, 4) : KMH_WS_CALL(2, false, 8);
    else rc = dzmask ? KMH_WS_CALL(1, true, 4) : KMH_WS_CALL(1, false, 8);
  } else if (p.NT == 2) rc = terms == 2 ? KMH_WG_CALL(2, 2) : KMH_WG_CALL(2, 3);
  else rc = terms == 2 ? KMH_WG_CALL(1, 2) : KMH_WG_CALL(1, 3);
#undef KMH_WS_CALL
#undef KMH_WG_CALL
  if (rc) return rc;
  const long long total = (long long)27 * Cin * Cout;
  int nb = ceil_div(total, 256);
  if (nb > 2048) nb = 2048;
  if (bhat)
  {
    int LP = 64;
    while (LP < 3 * Cout && LP < 1024) LP <<= 1;
    wgrad_bf_reduce_fold_kernel<<<dim3(Cin, 9), 1024, 0, s>>>((const float*)ws, N, (p.nslab / N) * p.KS, Cin, Cout, dw,
                                                              accumulate, xscale, dscale, w_fold, bhat, LP);
  }
  else
    wgrad_bf_reduce_kernel<<<nb, 256, 0, s>>>((const float*)ws, p.nslab * p.KS, Cin, Cout, dw, accumulate, xscale, dscale);
  return KMH_LAUNCH_CHECK();
}

KMH_API int kmh_conv3d_wgrad_bf(const float* x, const float* scale, const float* shift, const float* dz,
                                const float* dzmask, float* dw, int N, int D, int H, int W, int Cin, int Cout,
                                int relu_in, int accumulate, int terms, int append_ones, const float* xscale,
                                const float* dscale, int dz_blocked, const float* w_fold, double* bhat, void* ws,
                                void* stream) {
  if (dz_blocked < 0 || dz_blocked > 2) return -22;
  return wgrad_bf_impl(x, scale, shift, dz, dzmask, dw, N, D, H, W, Cin, Cout, relu_in, accumulate, terms, append_ones, xscale,
                       dscale, dz_blocked, nullptr, w_fold, bhat, ws, stream);
}

/* The weight gradient of a convolution whose output feeds only a 2 x 2 x 2 max-pool, from the POOLED gradient: dzp (N, D/2, H/2,
 * W/2, Cout) fp32 and `winners` (same shape, one byte per element: the window index 0..7 = (dz, dy, dx) kmh_conv3d_fwd_bf_pool /
 * kmh_maxpool3d_fwd record) stand for the dense gradient with one non-zero per window and channel, which is never formed.
 * Bit-identical to kmh_conv3d_wgrad_bf on the scattered tensor (dz_blocked 1 or 2).  Other arguments as kmh_conv3d_wgrad_bf;
 * served where kmh_conv3d_wgrad_bf_sparse_ok says so, -22 elsewhere. */
KMH_API int kmh_conv3d_wgrad_bf_sparse(const float* x, const float* scale, const float* shift, const float* dzp,
                                       const unsigned char* winners, float* dw, int N, int D, int H, int W, int Cin, int Cout,
                                       int relu_in, int accumulate, int terms, const float* xscale, const float* dscale,
                                       const float* w_fold, double* bhat, void* ws, void* stream) {
  return wgrad_bf_impl(x, scale, shift, dzp, nullptr, dw, N, D, H, W, Cin, Cout, relu_in, accumulate, terms, 0, xscale, dscale, 3,
                       winners, w_fold, bhat, ws, stream);
}
