// Local normalised cross-correlation of two volumes (the squared form ANTs and VoxelMorph use), with its gradient.
//
// a, b: (N, D, H, W) float32, each sample on its own.  Window w (odd, 3 <= w <= 15), r = w / 2.  For voxel p the window O(p) is the
// IN-BOUNDS part of the w^3 cube around p (truncated at the border, not zero-padded), n = |O(p)| = the product of three per-axis
// counts, and with the window sums Sa, Sb, Saa, Sbb, Sab of a, b, a^2, b^2, ab
//   cross = Sab - Sa Sb / n    va = max(Saa - Sa^2 / n, 0)    vb = max(Sbb - Sb^2 / n, 0)
//   cc_p = cross^2 / (va vb + eps)      out[n] = mean_p cc_p                                 (in [0, 1]; higher is better)
// Every sample is RECENTRED by its first voxel before anything is squared (a' = a - a[n, 0], b likewise): subtracting a nearby
// fp32 value is exact, cross, va and vb do not change in real arithmetic (truncated windows make cc exactly invariant to an
// offset), and the cancellation of Saa - Sa^2 / n at CT-range offsets is gone.
// Gradient, with D = va vb + eps, A = 2 cross / D, B = 2 cross^2 vb / D^2, C = 2 cross^2 va / D^2, ua = Sa / n, ub = Sb / n and
// box() the same truncated window sum (self-adjoint), V = D H W voxels:
//   d out / d a_v = [ box(A)_v b_v - box(A ub)_v - box(B)_v a_v + box(B ua)_v ] / V        (b: a <-> b, B -> C)
// which holds for the recentred a', b', ua', ub' as well (box(A) pivot - box(A pivot) = 0), so the pivot never comes back in.
//
// One walk serves all three passes (box_walk): a workgroup of 256 owns an 8 x 32 (y, x) column of kTileZ = 16 output planes and
// walks the planes z0 - r .. z0 + 15 + r.  Per plane: the (8 + 2r) x (32 + 2r) halo of the raw fields goes to LDS (the next
// plane's loads are issued before this plane is summed), the x pass sums w taps of every row directly into (8 + 2r) x 32 per
// sum, the y pass sums w of those rows directly, one output voxel per lane, and the plane's sums enter a ring of w planes in
// the lane's registers; the z pass is the direct sum of the ring.  Every window is summed directly in ascending x, y, z: nothing
// runs along an axis, so the error does not grow with the volume.  With 32 outputs along x a half wave reads one row: both LDS
// passes are conflict-free at any row pitch.
//   lncc_walk_kernel<w, false>   forward: raw a', b'; sums Sa, Sb, Saa, Sbb, Sab; cc summed over the tile in a fixed order
//                                (lane: ascending z; then block_sum) -> one partial per tile; lncc_final_kernel adds a sample's
//                                partials in fp64 in a fixed order.  Nothing the size of the volume is written.
//   lncc_walk_kernel<w, true>    the backward's first pass: the same walk, but writes the five fields A, B, C, ua', ub' (20 B per
//                                voxel) to ws instead of summing cc.
//   lncc_box_kernel<w, mode>     the backward's second pass: raw = those fields, sums box(A), box(A ub), box(B), box(B ua) (and
//                                / or the b side), combined with a'_v, b'_v and gout[n] / V.  mode: both, da only, db only; each
//                                side's arithmetic is the same explicit fma chain in every mode, so one gradient alone equals the
//                                same gradient of a call for both, bit for bit.
// No floating-point atomics anywhere: two runs are bit-identical, and the tiling depends on (D, H, W) alone, so a batch equals
// its samples run one by one.
#include "common.h"

namespace {
constexpr int TPB = 256;
constexpr int kTileX = 32, kTileY = 8, kTileZ = 16;
constexpr int kMinWin = 3, kMaxWin = 15;
constexpr int kFields = 5;                                            // A, B, C, ua', ub'
static_assert(kTileX * kTileY == TPB, "one output voxel of a plane per lane");

// voxels of [i - r, i + r] inside [0, n)
__device__ __forceinline__ int win_count(int i, int r, int n) {
  const int lo = i - r < 0 ? 0 : i - r, hi = i + r > n - 1 ? n - 1 : i + r;
  return hi - lo + 1;
}

// The walk.  P: NRAW raw fields per voxel, NSUM window sums;
//   p.fetch(z, y, x, v[NRAW])         the raw fields of an in-bounds voxel (out of bounds counts as 0 in every sum)
//   P::add(raw[NRAW], s[NSUM])        s += the terms of one voxel
//   p.emit(z, y, x, S[NSUM])          the window sums of an in-bounds output voxel, planes in ascending z
// lds: NRAW * PLANE + NSUM * PY * kTileX floats.
template <int WIN, class P>
__device__ __forceinline__ void box_walk(P& p, int D, int H, int W, int z0, int y0, int x0, float* lds) {
  constexpr int R = WIN / 2, PY = kTileY + 2 * R, PX = kTileX + 2 * R, PLANE = PY * PX, ROWS = PY * kTileX;
  constexpr int NR = P::NRAW, NS = P::NSUM, PER = (PLANE + TPB - 1) / TPB;
  float* raw = lds;                                                   // [NR][PY][PX]
  float* xs = lds + NR * PLANE;                                       // [NS][PY][kTileX]
  const int tid = threadIdx.x, ty = tid / kTileX, tx = tid % kTileX;
  const int zend = z0 + kTileZ < D ? z0 + kTileZ : D;                 // output planes z0 .. zend - 1
  const int plast = zend - 1 + R;
  float ring[NS][WIN], pre[PER][NR];
#pragma unroll
  for (int f = 0; f < NS; ++f)
#pragma unroll
    for (int k = 0; k < WIN; ++k) ring[f][k] = 0.f;

  auto fetch_plane = [&](int z) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = tid + i * TPB, y = y0 - R + e / PX, x = x0 - R + e % PX;
#pragma unroll
      for (int f = 0; f < NR; ++f) pre[i][f] = 0.f;
      if (e < PLANE && z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W) p.fetch(z, y, x, pre[i]);
    }
  };
  fetch_plane(z0 - R);
  for (int pz = z0 - R; pz <= plast; ++pz) {
    const bool live = pz >= 0 && pz < D;                              // workgroup-uniform
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = tid + i * TPB;
      if (e < PLANE) {
#pragma unroll
        for (int f = 0; f < NR; ++f) raw[f * PLANE + e] = pre[i][f];
      }
    }
    __syncthreads();
    if (pz < plast) fetch_plane(pz + 1);
    if (live) {
      for (int it = tid; it < ROWS; it += TPB) {                      // x pass: row it / 32 of the halo, output column it % 32
        const float* src = raw + (it / kTileX) * PX + it % kTileX;
        float s[NS];
#pragma unroll
        for (int f = 0; f < NS; ++f) s[f] = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
          float v[NR];
#pragma unroll
          for (int f = 0; f < NR; ++f) v[f] = src[f * PLANE + k];
          P::add(v, s);
        }
#pragma unroll
        for (int f = 0; f < NS; ++f) xs[f * ROWS + it] = s[f];
      }
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < NS; ++f) {
#pragma unroll
      for (int k = 0; k + 1 < WIN; ++k) ring[f][k] = ring[f][k + 1];
      float s = 0.f;
      if (live) {
#pragma unroll
        for (int k = 0; k < WIN; ++k) s += xs[f * ROWS + (ty + k) * kTileX + tx];      // y pass
      }
      ring[f][WIN - 1] = s;
    }
    const int oz = pz - R, y = y0 + ty, x = x0 + tx;
    if (oz >= z0 && y < H && x < W) {                                 // oz < zend by the loop's end
      float S[NS];
#pragma unroll
      for (int f = 0; f < NS; ++f) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) s += ring[f][k];                // z pass
        S[f] = s;
      }
      p.emit(oz, y, x, S);
    }
  }
}

// tile -> its corner; tiles run x fastest, then y, then z
__device__ __forceinline__ void tile_corner(int t, int H, int W, int& z0, int& y0, int& x0) {
  const int nx = (W + kTileX - 1) / kTileX, ny = (H + kTileY - 1) / kTileY;
  x0 = (t % nx) * kTileX;
  y0 = (t / nx % ny) * kTileY;
  z0 = (t / nx / ny) * kTileZ;
}

template <int WIN, bool STORE>
struct PairWalk {
  static constexpr int NRAW = 2, NSUM = 5;                            // a', b' -> Sa, Sb, Saa, Sbb, Sab
  const float* a;
  const float* b;
  float* fields;                                                      // STORE: this sample's A; the others kFields-strided by `fs`
  long long fs;
  float pa, pb, eps, acc;
  int D, H, W;
  __device__ __forceinline__ void fetch(int z, int y, int x, float (&v)[2]) const {
    const long long i = ((long long)z * H + y) * W + x;
    v[0] = a[i] - pa;
    v[1] = b[i] - pb;
  }
  __device__ static __forceinline__ void add(const float (&v)[2], float (&s)[5]) {
    s[0] += v[0];
    s[1] += v[1];
    s[2] = fmaf(v[0], v[0], s[2]);
    s[3] = fmaf(v[1], v[1], s[3]);
    s[4] = fmaf(v[0], v[1], s[4]);
  }
  __device__ __forceinline__ void emit(int z, int y, int x, const float (&S)[5]) {
    constexpr int R = WIN / 2;
    const float n = (float)(win_count(z, R, D) * win_count(y, R, H) * win_count(x, R, W));
    const float cross = S[4] - S[0] * S[1] / n;
    const float va = fmaxf(S[2] - S[0] * S[0] / n, 0.f), vb = fmaxf(S[3] - S[1] * S[1] / n, 0.f);
    const float den = fmaf(va, vb, eps);
    if constexpr (STORE) {
      const long long i = ((long long)z * H + y) * W + x;
      const float q = 2.f * cross * cross / (den * den);
      fields[i] = 2.f * cross / den;
      fields[fs + i] = q * vb;
      fields[2 * fs + i] = q * va;
      fields[3 * fs + i] = S[0] / n;
      fields[4 * fs + i] = S[1] / n;
    } else {
      acc += cross * cross / den;
    }
  }
};

// grid (tiles, N).  STORE: fields (kFields, N, V); else partial (N, tiles)
template <int WIN, bool STORE>
__global__ __launch_bounds__(TPB) void lncc_walk_kernel(const float* __restrict__ a, const float* __restrict__ b, int D, int H,
                                                        int W, float eps, float* __restrict__ partial,
                                                        float* __restrict__ fields) {
  constexpr int R = WIN / 2, PY = kTileY + 2 * R, PX = kTileX + 2 * R;
  __shared__ float lds[2 * PY * PX + 5 * PY * kTileX];
  __shared__ float scratch[TPB / kWave];
  const int n = blockIdx.y;
  const long long V = (long long)D * H * W;
  PairWalk<WIN, STORE> p;
  p.a = a + n * V;
  p.b = b + n * V;
  p.pa = p.a[0];
  p.pb = p.b[0];
  p.eps = eps;
  p.acc = 0.f;
  p.D = D, p.H = H, p.W = W;
  p.fs = (long long)gridDim.y * V;
  p.fields = STORE ? fields + n * V : nullptr;
  int z0, y0, x0;
  tile_corner(blockIdx.x, H, W, z0, y0, x0);
  box_walk<WIN>(p, D, H, W, z0, y0, x0, lds);
  if constexpr (!STORE) {
    const float sum = block_sum(p.acc, scratch);
    if (threadIdx.x == 0) partial[(long long)n * gridDim.x + blockIdx.x] = sum;
  }
}

// one workgroup per sample: out[n] = sum of its partials / V, in fp64 in a fixed order
__global__ __launch_bounds__(TPB) void lncc_final_kernel(const float* __restrict__ partial, int tiles, long long V,
                                                         float* __restrict__ out) {
  __shared__ double scratch[TPB / kWave];
  const int n = blockIdx.x;
  double acc = 0.0;
  for (int t = threadIdx.x; t < tiles; t += TPB) acc += (double)partial[(long long)n * tiles + t];
  acc = block_sum(acc, scratch);
  if (threadIdx.x == 0) out[n] = (float)(acc / (double)V);
}

// one side of the gradient: box(A) y - box(A uy) - box(Q) x + box(Q ux)
__device__ __forceinline__ float lncc_side(float sA, float sAuy, float sQ, float sQux, float x, float y) {
  return fmaf(sA, y, -sAuy) + fmaf(-sQ, x, sQux);
}

constexpr int kBoth = 0, kOnlyA = 1, kOnlyB = 2;
template <int MODE>
struct FieldWalk {
  // both: raw A, B, C, ua, ub -> box(A), box(A ub), box(B), box(B ua), box(A ua), box(C), box(C ub)
  // one side: raw A, Q, ux, uy -> box(A), box(A uy), box(Q), box(Q ux)   (da: Q = B, x = a; db: Q = C, x = b)
  static constexpr int NRAW = MODE == kBoth ? 5 : 4, NSUM = MODE == kBoth ? 7 : 4;
  const float* a;
  const float* b;
  const float* fields;
  long long fs;
  float* da;
  float* db;
  float pa, pb, scale;
  int H, W;
  __device__ __forceinline__ void fetch(int z, int y, int x, float (&v)[NRAW]) const {
    const long long i = ((long long)z * H + y) * W + x;
    v[0] = fields[i];
    if constexpr (MODE == kBoth) {
      v[1] = fields[fs + i];
      v[2] = fields[2 * fs + i];
      v[3] = fields[3 * fs + i];
      v[4] = fields[4 * fs + i];
    } else {
      v[1] = fields[(MODE == kOnlyA ? 1 : 2) * fs + i];
      v[2] = fields[(MODE == kOnlyA ? 3 : 4) * fs + i];
      v[3] = fields[(MODE == kOnlyA ? 4 : 3) * fs + i];
    }
  }
  __device__ static __forceinline__ void add(const float (&v)[NRAW], float (&s)[NSUM]) {
    s[0] += v[0];
    if constexpr (MODE == kBoth) {
      s[1] = fmaf(v[0], v[4], s[1]);
      s[2] += v[1];
      s[3] = fmaf(v[1], v[3], s[3]);
      s[4] = fmaf(v[0], v[3], s[4]);
      s[5] += v[2];
      s[6] = fmaf(v[2], v[4], s[6]);
    } else {
      s[1] = fmaf(v[0], v[3], s[1]);
      s[2] += v[1];
      s[3] = fmaf(v[1], v[2], s[3]);
    }
  }
  __device__ __forceinline__ void emit(int z, int y, int x, const float (&S)[NSUM]) {
    const long long i = ((long long)z * H + y) * W + x;
    const float av = a[i] - pa, bv = b[i] - pb;
    if constexpr (MODE == kBoth) {
      da[i] = scale * lncc_side(S[0], S[1], S[2], S[3], av, bv);
      db[i] = scale * lncc_side(S[0], S[4], S[5], S[6], bv, av);
    } else if constexpr (MODE == kOnlyA) {
      da[i] = scale * lncc_side(S[0], S[1], S[2], S[3], av, bv);
    } else {
      db[i] = scale * lncc_side(S[0], S[1], S[2], S[3], bv, av);
    }
  }
};

template <int WIN, int MODE>
__global__ __launch_bounds__(TPB) void lncc_box_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       const float* __restrict__ fields, const float* __restrict__ gout, int D,
                                                       int H, int W, float* __restrict__ da, float* __restrict__ db) {
  constexpr int R = WIN / 2, PY = kTileY + 2 * R, PX = kTileX + 2 * R;
  __shared__ float lds[FieldWalk<MODE>::NRAW * PY * PX + FieldWalk<MODE>::NSUM * PY * kTileX];
  const int n = blockIdx.y;
  const long long V = (long long)D * H * W;
  FieldWalk<MODE> p;
  p.a = a + n * V;
  p.b = b + n * V;
  p.pa = p.a[0];
  p.pb = p.b[0];
  p.fields = fields + n * V;
  p.fs = (long long)gridDim.y * V;
  p.da = da ? da + n * V : nullptr;
  p.db = db ? db + n * V : nullptr;
  p.scale = gout[n] / (float)V;
  p.H = H, p.W = W;
  int z0, y0, x0;
  tile_corner(blockIdx.x, H, W, z0, y0, x0);
  box_walk<WIN>(p, D, H, W, z0, y0, x0, lds);
}

bool lncc_ok(int N, int D, int H, int W, int window) {
  return N >= 1 && N <= 65535 && D >= 1 && H >= 1 && W >= 1 && (long long)D * H * W < (1ll << 31) && window >= kMinWin &&
         window <= kMaxWin && (window & 1);
}
long long lncc_tiles(int D, int H, int W) {
  return (long long)ceil_div(D, kTileZ) * ceil_div(H, kTileY) * ceil_div(W, kTileX);
}
size_t lncc_partial_bytes(int N, int D, int H, int W) {
  return ((size_t)N * lncc_tiles(D, H, W) * sizeof(float) + 255) / 256 * 256;
}

template <int WIN>
void lncc_fwd_launch(const float* a, const float* b, int N, int D, int H, int W, float eps, float* out, float* partial,
                     hipStream_t s) {
  const int tiles = (int)lncc_tiles(D, H, W);
  lncc_walk_kernel<WIN, false><<<dim3((unsigned)tiles, (unsigned)N), TPB, 0, s>>>(a, b, D, H, W, eps, partial, nullptr);
  lncc_final_kernel<<<N, TPB, 0, s>>>(partial, tiles, (long long)D * H * W, out);
}

template <int WIN>
void lncc_bwd_launch(const float* a, const float* b, const float* gout, int N, int D, int H, int W, float eps, float* da,
                     float* db, float* fields, hipStream_t s) {
  const dim3 grid((unsigned)lncc_tiles(D, H, W), (unsigned)N);
  lncc_walk_kernel<WIN, true><<<grid, TPB, 0, s>>>(a, b, D, H, W, eps, nullptr, fields);
  if (da && db)
    lncc_box_kernel<WIN, kBoth><<<grid, TPB, 0, s>>>(a, b, fields, gout, D, H, W, da, db);
  else if (da)
    lncc_box_kernel<WIN, kOnlyA><<<grid, TPB, 0, s>>>(a, b, fields, gout, D, H, W, da, nullptr);
  else
    lncc_box_kernel<WIN, kOnlyB><<<grid, TPB, 0, s>>>(a, b, fields, gout, D, H, W, nullptr, db);
}
}  // namespace

#define LNCC_WINDOWS(X) X(3) X(5) X(7) X(9) X(11) X(13) X(15)

/* Workspace of kmh_lncc_fwd and kmh_lncc_bwd: one float per tile (16 x 8 x 32 voxels) and sample for the forward, and behind
 * them the backward's five coefficient fields, 20 bytes per voxel = 2.5 times the two inputs.  0 for arguments the entries refuse. */
KMH_API size_t kmh_lncc_ws_bytes(int N, int D, int H, int W, int window) {
  if (!lncc_ok(N, D, H, W, window)) return 0;
  return lncc_partial_bytes(N, D, H, W) + (size_t)kFields * N * D * H * W * sizeof(float);
}

/* a, b: (N, D, H, W) float32 contiguous; window odd in [3, 15]; fewer than 2^31 voxels per sample.  out: N floats.  ws:
 * kmh_lncc_ws_bytes bytes, of which only the per-tile partials are written. */
KMH_API int kmh_lncc_fwd(const float* a, const float* b, int N, int D, int H, int W, int window, float eps, float* out, void* ws,
                         void* stream) {
  if (!lncc_ok(N, D, H, W, window) || !a || !b || !out || !ws || !(eps >= 0.f)) return -22;
  hipStream_t s = (hipStream_t)stream;
  switch (window) {
#define X(w) case w: lncc_fwd_launch<w>(a, b, N, D, H, W, eps, out, (float*)ws, s); break;
    LNCC_WINDOWS(X)
#undef X
  }
  return KMH_LAUNCH_CHECK();
}

/* da[n, v] = gout[n] d out[n] / d a[n, v], db likewise; either may be NULL.  ws: kmh_lncc_ws_bytes bytes (the fields are
 * recomputed here: nothing of the forward's is read). */
KMH_API int kmh_lncc_bwd(const float* a, const float* b, const float* gout, int N, int D, int H, int W, int window, float eps,
                         float* da, float* db, void* ws, void* stream) {
  if (!lncc_ok(N, D, H, W, window) || !a || !b || !gout || !ws || !(eps >= 0.f)) return -22;
  if (!da && !db) return 0;
  hipStream_t s = (hipStream_t)stream;
  float* fields = (float*)((char*)ws + lncc_partial_bytes(N, D, H, W));
  switch (window) {
#define X(w) case w: lncc_bwd_launch<w>(a, b, gout, N, D, H, W, eps, da, db, fields, s); break;
    LNCC_WINDOWS(X)
#undef X
  }
  return KMH_LAUNCH_CHECK();
}
