// Gaussian smoothing of a volume along its three spatial axes, and its exact transpose: what the registration pyramids apply
// before they shrink (ANTs --smoothing-sigmas, elastix' pyramid schedules) and what regularises a dense displacement field.
//
// Definition (tests/gauss_ref.py restates it in fp64; scipy.ndimage.gaussian_filter(mode="nearest", truncate=t) agrees):
//   per axis with sigma > 0:  R = int(t sigma + 0.5),  w[k] = exp(-k^2 / 2 sigma^2) / sum_k exp(-k^2 / 2 sigma^2),  k = -R .. R,
//   out[i] = sum_k w[k] x[clamp(i + k, 0, n - 1)]      -- the replicated border;
//   an axis with R = 0 is not touched (bit for bit); the passes run along W, then H, then D.
// The weights come from the host: computed and normalised in fp64, rounded to fp32 once (ops.gaussian_kernel1d), handed over as
// the half-kernel w[0 .. R] and copied into the kernels' ARGUMENTS by value -- no host-to-device copy, nothing a driver's step
// would wait for.  Every output is one fma chain over its taps in a fixed order (forward: k = -R .. R): interior, border, every
// channel and every sample round identically, runs repeat bit for bit and a batch equals its samples.
//
// Transpose (the gradient with respect to x), a gather, no atomics; passes along D, then H, then W:
//   0 < j < n - 1:  dx[j] = sum_k w[k] g[j - k]  over the k with 0 <= j - k <= n - 1,
//   j = 0:          dx[0] = sum_i g[i] T[i],  T[i] = sum_{k <= -i} w[k] = sum_{k >= i} w[k],  i = 0 .. min(R, n - 1),
//   j = n - 1:      the mirror image, dx[n - 1] = sum_i g[n - 1 - i] T[i];
//   a line with n <= R folds at both ends at once (i reaches the far end in both sums); n = 1 is its own transpose.
// The tail sums T[0 .. R] are computed on the host in fp64 too.
//
// The operator is bandwidth-bound: 4 B in and 4 B out per voxel is its floor.  Each active axis is one pass here, so an axis costs
// a little over 8 B per voxel and three axes a little over 24; x is not fused into y.  What the two pass kernels make sure of is
// that a voxel is read from memory about once per pass and not 2 R + 1 times:
//   x pass (rows kernel): a workgroup owns 1024 consecutive voxels of a channel plane -- whole rows or pieces of rows, whatever
//       W is; four per lane, 256 apart -- and stages them with R more on either side in LDS, one coalesced copy; a tap of voxel v lies in v's row, so within
//       [v - R, v + R], so inside the tile.  Each lane then reads its 2 R + 1 taps from LDS at unit stride across the lanes (no
//       bank conflicts).  Traffic: 4 (1 + 2 R / 1024) B in + 4 B out per voxel.
//   y and z passes (walk kernel): one line per lane, lanes along x (z pass: along the whole H W plane), so every load and store is
//       coalesced.  The axis is cut into segments of S outputs (a multiple of 8; S >= 2 R); a lane walks its segment with the
//       last 2 R + 8 samples of its line in a ring in LDS -- a lane-private column, ring[slot][lane], so no barrier and no bank
//       conflict -- loading 8 new samples at a time, the next 8 already in flight while the current 8 outputs are summed: each
//       row of the ring is read once per step and feeds the 8 accumulators it reaches, (2 R + 8) / 8 LDS reads per output.
//       Traffic: 4 (1 + 2 R / S) B in + 4 B out per voxel; S is the whole axis when the other two axes alone fill the device,
//       and shrinks to no less than max(2 R, 16) when they do not (R <= 8: S = 16 at 128^3, S = 32 at 256^3); the R rows a
//       segment reads beyond its ends are its neighbours' own rows, in flight through L2 at about the same time.
//   The weights sit in LDS too (staged once per workgroup from the kernel's arguments): a tap of the x pass costs two LDS reads
//   and an fma; the walk reads the 8 weights of a ring row as two aligned 16-byte broadcasts (four copies of the kernel in LDS,
//   shifted by 0 .. 3 floats, make any start aligned), so a row costs three LDS reads for its 8 fmas.
// profiles/gauss_bench.json has the measured ratios to the floor.  A pass cannot run in place (it reads its neighbours), so two
// or three active axes ping-pong through a workspace of the volume's size (kmh_gauss_ws_bytes).
// Every loop is bounded by R, by a segment's length or by the tile's size; no waiting loops, nothing between workgroups.
// Limits (kmh_gauss_* return -22 past them, ops refuses with ValueError before allocating): R <= 32 per axis (sigma <= 8 at
// truncate = 4), a channel plane of fewer than 2^29 voxels (32-bit indices inside a plane), N C <= 65535 (gridDim.y).
#include "common.h"

namespace {

constexpr int kTPB = 256;          // rows kernel: lanes per workgroup
constexpr int kVPT = 4;            // rows kernel: voxels per lane, kTPB apart
constexpr int kTile = kTPB * kVPT; // rows kernel: consecutive voxels per workgroup
constexpr int kMaxR = 32;
constexpr int kLanes = 128;        // walk kernel: lines per workgroup
constexpr int kU = 8;              // walk kernel: samples loaded, and outputs summed, per step
constexpr int kWfPitch = 72;       // walk kernel: floats between the four shifted copies of the weights (>= 2 kMaxR + 1, a multiple of 4)
static_assert(kU == 8 && kWfPitch % 4 == 0 && kWfPitch >= 2 * kMaxR + 1, "the walk kernel reads its 8 weights as two float4");
constexpr int kWalkBlocks = 4096;  // workgroups the walk kernel wants before it stops cutting the axis into segments

struct GaussTaps {
  float w[kMaxR + 1];      // w[|k|]
  float t[kMaxR + 1];      // T[i] = sum_{k >= i} w[k] (the transpose only)
};

// The weights go from the kernel's arguments into LDS once per workgroup (lane j picks w[j] by a chain of selects over constant
// indices, so the argument struct stays in scalar registers), as the full symmetric kernel wf[k + R] = w[|k|] and the tails: a tap then costs LDS reads, which pipeline,
// not a scalar load from the argument segment and its wait.
template <bool TRANSPOSE>
__device__ __forceinline__ float stage_taps(const GaussTaps& taps, int R, float* wf, float* tl) {
  const int j = threadIdx.x;                         // lane j <= R stages w[j] and T[j]
  float w = 0.f, t = 0.f;
#pragma unroll
  for (int c = 0; c <= kMaxR; ++c) {                 // a select chain: the struct is only ever indexed by a constant
    w = j == c ? taps.w[c] : w;
    if (TRANSPOSE) t = j == c ? taps.t[c] : t;
  }
  if (j <= R) {
    wf[R + j] = w;
    wf[R - j] = w;
    if (TRANSPOSE) tl[j] = t;
  }
  return w;
}

// x pass.  TRANSPOSE with W == 1 is the forward sum (the operator on one sample is a scalar).
template <bool TRANSPOSE>
__global__ __launch_bounds__(kTPB) void gauss_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int plane, int W,
                                                          int R, GaussTaps taps) {
  __shared__ float tile[kTile + 2 * kMaxR];
  __shared__ float wf[2 * kMaxR + 1];
  __shared__ float tl[kMaxR + 1];
  const int tid = threadIdx.x, v0 = blockIdx.x * kTile;
  const long long base = (long long)blockIdx.y * plane;
  const float* s = src + base;
  for (int e = tid; e < kTile + 2 * R; e += kTPB) {  // voxels v0 - R .. v0 + kTile - 1 + R of the plane; what lies outside is never read back
    const int idx = v0 - R + e;
    tile[e] = idx >= 0 && idx < plane ? s[idx] : 0.f;
  }
  stage_taps<TRANSPOSE>(taps, R, wf, tl);
  __syncthreads();
  const float* wc = wf + R;                          // wc[k] = w[|k|]
#pragma unroll
  for (int j = 0; j < kVPT; ++j) {
    const int lt = tid + j * kTPB, v = v0 + lt;
    if (v >= plane) break;
    const int p = v % W;
    const int lo = -p, hi = W - 1 - p;               // the row's ends as offsets from this voxel's column: lo <= 0 <= hi
    const float* t = tile + lt + R;                  // t[d]: the sample d columns from this voxel's, -R <= d <= R
    float acc = 0.f;
    if (!TRANSPOSE || W == 1) {
#pragma unroll 4
      for (int k = -R; k <= R; ++k) {                // bounded by R
        const int d = k < lo ? lo : (k > hi ? hi : k);
        acc = fmaf(wc[k], t[d], acc);
      }
    } else if (p > 0 && p < W - 1) {
      const int k0 = -R > -hi ? -R : -hi, k1 = R < p ? R : p;      // the k with 0 <= p - k <= W - 1
#pragma unroll 4
      for (int k = k0; k <= k1; ++k) acc = fmaf(wc[k], t[-k], acc);
    } else {
      const int m = R < W - 1 ? R : W - 1;
      const int step = p == 0 ? 1 : -1;
      for (int i = 0; i <= m; ++i) acc = fmaf(tl[i], t[i * step], acc);
    }
    dst[base + v] = acc;
  }
}

// y and z passes.  Line l of nlines: base = (l / inner) * outer + l % inner, samples `stride` apart (z: inner = H W,
// outer = D H W, stride = H W; y: inner = W, outer = H W, stride = W).  blockIdx.y = the segment: outputs [s0, min(s0 + S, n)).
// The ring holds the logical rows i0 - R .. i0 + R + kU - 1 of the line for the step's outputs i0 .. i0 + kU - 1, row j at slot
// (j - (s0 - R)) mod (2 R + kU); a logical row outside [0, n - 1] is the clamped sample (forward) or 0 (transpose).
// A step reads each row of the ring ONCE and feeds it to the kU accumulators it reaches (row i0 - R + rr, output i0 + u:
// k = rr - R - u, weight wf[rr - u]): rows ascending, so every output is still one fma chain over k = -R .. R.
// The transpose is the same sum -- w is symmetric, and away from the ends A^T is the convolution with zeros outside instead
// of replicas -- except at the outputs 0 and n - 1, which are summed again from the ring with the tail weights.
// TRANSPOSE is launched for n >= 2 only (n == 1 takes the forward instance).
template <bool TRANSPOSE>
__global__ __launch_bounds__(kLanes) void gauss_walk_kernel(const float* __restrict__ src, float* __restrict__ dst, long long nlines,
                                                            long long inner, long long outer, long long stride, int n, int S, int R,
                                                            GaussTaps taps) {
  extern __shared__ __attribute__((aligned(16))) float ring[];      // (2 R + kU) * kLanes floats, then wf and its copies, then tl
  const int cap = 2 * R + kU;
  float* wf = ring + cap * kLanes;                   // wf[k + R] = w[|k|]; copy c at wf + c * kWfPitch holds wf shifted down by c
  float* tl = wf + 4 * kWfPitch;
  const float wj = stage_taps<TRANSPOSE>(taps, R, wf, tl);
  if ((int)threadIdx.x <= R) {
    const int j = threadIdx.x;
#pragma unroll
    for (int c = 1; c < 4; ++c) {                    // copy c: 8 consecutive weights from wf[a], a mod 4 == c, are two aligned 16-byte reads
      if (R + j - c >= 0) wf[c * kWfPitch + R + j - c] = wj;
      if (R - j - c >= 0) wf[c * kWfPitch + R - j - c] = wj;
    }
  }
  __syncthreads();                                   // the only barrier: a lane touches its own column of the ring only
  const long long l = (long long)blockIdx.x * kLanes + threadIdx.x;
  if (l >= nlines) return;
  const long long q = l / inner;
  const long long base = q * outer + (l - q * inner);
  const float* s = src + base;
  float* d = dst + base;
  const int s0 = blockIdx.y * S;
  const int s1 = s0 + S < n ? s0 + S : n;
  float* col = ring + threadIdx.x;
  auto fetch = [&](int j) -> float {                 // logical row j: every address lies inside the line
    if (TRANSPOSE) return j >= 0 && j <= n - 1 ? s[j * stride] : 0.f;
    const int c = j < 0 ? 0 : (j > n - 1 ? n - 1 : j);
    return s[c * stride];
  };
  float nxt[kU];
  for (int e0 = 0; e0 < 2 * R; e0 += kU) {           // rows s0 - R .. s0 + R - 1 at slots 0 .. 2 R - 1, kU loads in flight together
#pragma unroll
    for (int u = 0; u < kU; ++u) nxt[u] = fetch(s0 - R + e0 + u);      // (past 2 R: a row the next batch loads again; in bounds)
#pragma unroll
    for (int u = 0; u < kU; ++u)
      if (e0 + u < 2 * R) col[(e0 + u) * kLanes] = nxt[u];
  }
#pragma unroll
  for (int u = 0; u < kU; ++u) nxt[u] = fetch(s0 + R + u);
  int head = 0;                                      // slot of row i0 - R
  int wslot = 2 * R;                                 // slot of row i0 + R
  for (int i0 = s0; i0 < s1; i0 += kU) {             // bounded by S
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      col[wslot * kLanes] = nxt[u];
      wslot = wslot + 1 == cap ? 0 : wslot + 1;
    }
    if (i0 + kU < s1) {                              // the next step's samples fly while this step's outputs are summed
#pragma unroll
      for (int u = 0; u < kU; ++u) nxt[u] = fetch(i0 + kU + R + u);
    }
    float acc[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) acc[u] = 0.f;
    int sl = head;
    for (int rr = 0; rr < cap; ++rr) {               // row i0 - R + rr; bounded by 2 R + kU
      const float v = col[sl * kLanes];
      sl = sl + 1 == cap ? 0 : sl + 1;
      if (rr >= kU - 1 && rr <= 2 * R) {             // within R of every output of the step: the weights wf[rr - 7 .. rr]
        const int a = rr - (kU - 1), c = a & 3;
        const float4* wr = reinterpret_cast<const float4*>(wf + c * kWfPitch + (a - c));
        const float4 w0 = wr[0], w1 = wr[1];         // wf[a .. a + 3], wf[a + 4 .. a + 7]; output u takes wf[rr - u]
        acc[0] = fmaf(w1.w, v, acc[0]); acc[1] = fmaf(w1.z, v, acc[1]); acc[2] = fmaf(w1.y, v, acc[2]); acc[3] = fmaf(w1.x, v, acc[3]);
        acc[4] = fmaf(w0.w, v, acc[4]); acc[5] = fmaf(w0.z, v, acc[5]); acc[6] = fmaf(w0.y, v, acc[6]); acc[7] = fmaf(w0.x, v, acc[7]);
      } else {
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = rr - u;
          if (j >= 0 && j <= 2 * R) acc[u] = fmaf(wf[j], v, acc[u]);
        }
      }
    }
    if (TRANSPOSE) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int i = i0 + u;
        if (i < s1 && (i == 0 || i == n - 1)) {      // row i: up from row 0 (i == 0), down from row n - 1 (i == n - 1)
          int a = head + u + R;
          a = a >= cap ? a - cap : a;
          float b = 0.f;
          for (int j = 0; j <= R; ++j) {
            b = fmaf(tl[j], col[a * kLanes], b);
            if (i == 0) a = a + 1 == cap ? 0 : a + 1;
            else a = a == 0 ? cap - 1 : a - 1;
          }
          acc[u] = b;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u)
      if (i0 + u < s1) d[(i0 + u) * stride] = acc[u];
    head = head + kU >= cap ? head + kU - cap : head + kU;
  }
}

__global__ __launch_bounds__(kTPB) void gauss_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int plane) {
  const int v = blockIdx.x * kTPB + threadIdx.x;
  if (v < plane) dst[(long long)blockIdx.y * plane + v] = src[(long long)blockIdx.y * plane + v];
}

bool gauss_shape_ok(int N, int C, int D, int H, int W, int rz, int ry, int rx) {
  return N >= 1 && C >= 1 && D >= 1 && H >= 1 && W >= 1 && (long long)N * C <= 65535 && (long long)D * H * W < (1ll << 29) &&
         rz >= 0 && ry >= 0 && rx >= 0 && rz <= kMaxR && ry <= kMaxR && rx <= kMaxR;
}

struct Axis {
  int n, R;
  long long inner;         // 0: the x axis (rows kernel); else the walk kernel's inner (stride = inner)
  const float *w, *t;
};

template <bool TRANSPOSE>
int gauss_walk(const float* src, float* dst, long long total, const Axis& ax, const GaussTaps& taps, hipStream_t s) {
  const long long nlines = total / ax.n, inner = ax.inner, outer = inner * ax.n;
  const long long colblocks = (nlines + kLanes - 1) / kLanes;
  if (colblocks >= (1ll << 31)) return -22;
  int smin = 2 * ax.R > 16 ? 2 * ax.R : 16;
  smin = (smin + kU - 1) / kU * kU;
  long long nseg = (kWalkBlocks + colblocks - 1) / colblocks;                  // segments wanted to fill the device
  const long long most = (ax.n + smin - 1) / smin;                             // segments of at least smin outputs
  nseg = nseg > most ? most : nseg;
  nseg = nseg > 65535 ? 65535 : nseg;
  int S = (int)((ax.n + nseg - 1) / nseg);
  S = (S + kU - 1) / kU * kU;
  nseg = (ax.n + S - 1) / S;
  const dim3 grid((unsigned)colblocks, (unsigned)nseg);
  const size_t lds = ((size_t)(2 * ax.R + kU) * kLanes + 4 * kWfPitch + kMaxR + 1) * sizeof(float);      // ring, wf x 4, tl: at most 38 KB
  if (TRANSPOSE && ax.n > 1)
    gauss_walk_kernel<true><<<grid, kLanes, lds, s>>>(src, dst, nlines, inner, outer, inner, ax.n, S, ax.R, taps);
  else
    gauss_walk_kernel<false><<<grid, kLanes, lds, s>>>(src, dst, nlines, inner, outer, inner, ax.n, S, ax.R, taps);
  return KMH_LAUNCH_CHECK();
}

template <bool TRANSPOSE>
int gauss_run(const float* x, float* out, void* ws, int N, int C, int D, int H, int W, const Axis* order, hipStream_t s) {
  const int plane = D * H * W;
  const long long total = (long long)N * C * plane;
  const dim3 grid((unsigned)((plane + kTPB - 1) / kTPB), (unsigned)(N * C));
  Axis act[3];
  int k = 0;
  for (int a = 0; a < 3; ++a)
    if (order[a].R > 0) act[k++] = order[a];
  if (k == 0) {
    gauss_copy_kernel<<<grid, kTPB, 0, s>>>(x, out, plane);
    return KMH_LAUNCH_CHECK();
  }
  if (k > 1 && !ws) return -22;
  const float* src = x;
  for (int i = 0; i < k; ++i) {
    float* dst = (k - 1 - i) % 2 == 0 ? out : (float*)ws;      // the last pass lands in out
    GaussTaps taps;
    for (int j = 0; j <= kMaxR; ++j) {
      taps.w[j] = j <= act[i].R ? act[i].w[j] : 0.f;
      taps.t[j] = TRANSPOSE && j <= act[i].R ? act[i].t[j] : 0.f;
    }
    int rc;
    if (act[i].inner == 0) {
      const dim3 tiles((unsigned)((plane + kTile - 1) / kTile), (unsigned)(N * C));
      gauss_rows_kernel<TRANSPOSE><<<tiles, kTPB, 0, s>>>(src, dst, plane, W, act[i].R, taps);
      rc = KMH_LAUNCH_CHECK();
    } else {
      rc = gauss_walk<TRANSPOSE>(src, dst, total, act[i], taps, s);
    }
    if (rc) return rc;
    src = dst;
  }
  return 0;
}

}  // namespace

KMH_API size_t kmh_gauss_ws_bytes(int N, int C, int D, int H, int W, int rz, int ry, int rx) {
  if (!gauss_shape_ok(N, C, D, H, W, rz, ry, rx)) return 0;
  const int active = (rz > 0) + (ry > 0) + (rx > 0);
  return active > 1 ? (size_t)N * C * D * H * W * sizeof(float) : 0;
}

KMH_API int kmh_gauss_fwd(const float* x, float* out, void* ws, int N, int C, int D, int H, int W, int rz, int ry, int rx,
                          const float* wz, const float* wy, const float* wx, void* stream) {
  if (!x || !out || x == out || !gauss_shape_ok(N, C, D, H, W, rz, ry, rx)) return -22;
  if ((rz > 0 && !wz) || (ry > 0 && !wy) || (rx > 0 && !wx)) return -22;
  const Axis order[3] = {{W, rx, 0, wx, nullptr}, {H, ry, W, wy, nullptr}, {D, rz, (long long)H * W, wz, nullptr}};
  return gauss_run<false>(x, out, ws, N, C, D, H, W, order, (hipStream_t)stream);
}

KMH_API int kmh_gauss_bwd(const float* gout, float* dx, void* ws, int N, int C, int D, int H, int W, int rz, int ry, int rx,
                          const float* wz, const float* wy, const float* wx, const float* tz, const float* ty, const float* tx,
                          void* stream) {
  if (!gout || !dx || gout == dx || !gauss_shape_ok(N, C, D, H, W, rz, ry, rx)) return -22;
  if ((rz > 0 && !(wz && tz)) || (ry > 0 && !(wy && ty)) || (rx > 0 && !(wx && tx))) return -22;
  const Axis order[3] = {{D, rz, (long long)H * W, wz, tz}, {H, ry, W, wy, ty}, {W, rx, 0, wx, tx}};
  return gauss_run<true>(gout, dx, ws, N, C, D, H, W, order, (hipStream_t)stream);
}
