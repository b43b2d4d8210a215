// Fused align_img + soft DiceLoss (scripts/train.py:146-164 with loss_fn == "dice"; keymorph/utils.py:14-21,
// keymorph/loss_ops.py:16-63) WITHOUT the warped segmentation ever being stored.  Dice couples every voxel of a
// (sample, channel) row through its three sums, so the cotangent of the warp is only known after a full pass:
//   pass A (warp_dice_sums_kernel)  per (n, c): sum t p, sum p^2, sum t^2 with p = warp(x)[n, c] recomputed on the fly;
//   host: loss rows 1 - (2 I + 1) / (P + T + 1), and for the backward ca = -2 g / den, cb = 2 g num / den^2;
//   pass B (warp_dice_grad_kernel)  d(loss)/d(grid) = sum_c (ca[n,c] t + cb[n,c] p) * d p / d grid, p recomputed again.
// Per output voxel: A reads 12 + 8 C bytes, B reads 12 + 8 C and writes 12 -- the three-launch route (warp, Dice sums,
// axpby, grid backward) moves 24 + 32 C.  Both kernels are persistent over 1024-voxel chunks (lane-contiguous like
// sample_fwd_lc_kernel) and fetch the NEXT chunk's grid rows into registers before the current chunk's gathers.
// ILP = voxels of a lane whose gathers are in flight together (PASSES / ILP sub-passes per chunk)
#include "sampler_taps.h"

namespace {

constexpr int WD_MAXC = 128;

// the tap of chunk voxel l from its staged grid row
__device__ __forceinline__ void chunk_tap(TapB& q, const float* sg, int l, int cnt, int D, int H, int W, unsigned plane_bytes) {
  q = make_tapb(make_tap(sg[l * 3], sg[l * 3 + 1], sg[l * 3 + 2], D, H, W), D, H, W);
  if (l >= cnt) {     // past the chunk: every corner reads 0 through the range check, and the weights must be finite
    park(q, plane_bytes);                 // (sg holds stale LDS there: 0 * NaN would poison the wave's sums; the gradient
    q.fx = q.fy = q.fz = 0.f;             //  kernel gets no contribution and stores nothing of this row)
  }
}

// the grid rows of `chunk` on their way into registers (in flight under the current chunk's gathers); returns whether the
// chunk is a fast one -- a ragged or unaligned chunk is copied by commit_rows when its turn comes
__device__ __forceinline__ bool prefetch_chunk(const float* gbase, long long ovox, int chunk, GridRows& g, int tid) {
  const long long vb = (long long)chunk * CHUNK;
  const bool fast = rows_fast(gbase + vb * 3, chunk_count(ovox, vb));
  fetch_rows(gbase + vb * 3, fast, g, tid);
  return fast;
}

// LAB variants: both segmentations are exactly one-hot (what scripts/train.py:54-79 builds: one_hot of a label map,
// augmented with NEAREST sampling), so a voxel's C channel values are determined by ONE byte.  kmh_onehot_to_labels checks
// that on the device and writes the label maps; the kernels then gather 8 corner LABELS per voxel once instead of 8 corner
// values per channel (56 B of gathers and 56 B of fixed-segmentation reads per voxel become 8 + 1), and feed
// v_k = [label_k == c] into the SAME blend / derivative arithmetic: bit-identical results.  `gate` (device int): the LAB
// kernels return at once when it reads 0, the dense ones when it reads non-zero -- no host synchronisation decides.
struct LabTaps { unsigned c[8]; unsigned t; };      // 8 corner labels (255 = none) and the fixed label
__device__ __forceinline__ unsigned ld_lab(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return (unsigned)__builtin_amdgcn_raw_buffer_load_b8(r, (int)off, 0, 0) & 255u;
}
// q's byte offsets are 4 * voxel index: the label map has one byte per voxel
__device__ __forceinline__ void gather_labels(__amdgpu_buffer_rsrc_t r, const TapB& q, bool live, LabTaps& L) {
  const unsigned o[4] = {q.o00 >> 2, q.o01 >> 2, q.o10 >> 2, q.o11 >> 2};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned a = ld_lab(r, o[k]), b = ld_lab(r, o[k] + 1u);
    L.c[2 * k] = live ? (q.sel ? b : a) : 255u;             // as pair_b: the last column's pair sits one to the left
    L.c[2 * k + 1] = (live && !q.sel) ? b : 255u;
  }
}

// the labels of sub-pass j0 of the chunk at voxel vb: 8 corner labels and the fixed label of each of the lane's ILP voxels
template <int ILP>
__device__ __forceinline__ void load_labels(const unsigned char* __restrict__ labx, const unsigned char* __restrict__ labf,
                                            int n, long long plane, long long ovox, long long vb, int j0, int cnt,
                                            const TapB (&q)[ILP], LabTaps (&lab)[ILP], int tid) {
  const int left = cnt - j0 * TPB;                 // voxels of the chunk from this sub-pass on (may be <= 0)
  const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(labx + (long long)n * plane), 0, (int)plane, 0x00020000);
  const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char*>(labf + (long long)n * ovox + vb + j0 * TPB), 0, left > 0 ? left : 0, 0x00020000);
#pragma unroll
  for (int u = 0; u < ILP; ++u) {
    const bool live = tid + (j0 + u) * TPB < cnt;
    gather_labels(rl, q[u], live, lab[u]);
    const unsigned t = ld_lab(rt, (unsigned)(tid + u * TPB));
    lab[u].t = live ? t : 255u;
  }
}

// channel c of the same voxels: the 8 corner values v and the fixed value tv -- [label == c] (LAB) or gathered from the float
// tensors; lanes past the chunk get zeros either way
template <bool LAB, int ILP>
__device__ __forceinline__ void corner_values(const float* __restrict__ x, const float* __restrict__ fixed, int n, int c,
                                              int C, long long plane, unsigned plane_bytes, long long ovox, long long vb,
                                              int j0, int cnt, const TapB (&q)[ILP], const LabTaps (&lab)[ILP],
                                              float (&v)[ILP][8], float (&tv)[ILP], int tid) {
  if constexpr (LAB) {
#pragma unroll
    for (int u = 0; u < ILP; ++u) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[u][k] = lab[u].c[k] == (unsigned)c ? 1.f : 0.f;
      tv[u] = lab[u].t == (unsigned)c ? 1.f : 0.f;
    }
  } else {
    const int left = cnt - j0 * TPB;
    const unsigned fbytes = left > 0 ? 4u * (unsigned)left : 0u;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(x + ((long long)n * C + c) * plane, plane_bytes);
    const __amdgpu_buffer_rsrc_t rf = make_rsrc(fixed + ((long long)n * C + c) * ovox + vb + j0 * TPB, fbytes);
#pragma unroll
    for (int u = 0; u < ILP; ++u) {
      gather8_b(rx, q[u], v[u]);
      tv[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rf, 4 * (tid + u * TPB), 0, 0));
    }
  }
}

// partial: (N, gridDim.x, C, 3) doubles
template <int WD_ILP, bool LAB = false>
__global__ __launch_bounds__(TPB) void warp_dice_sums_kernel(
    const float* __restrict__ x, const float* __restrict__ grid, const float* __restrict__ fixed,
    double* __restrict__ partial, int C, int D, int H, int W, long long ovox, int nchunk,
    const unsigned char* __restrict__ labx = nullptr, const unsigned char* __restrict__ labf = nullptr,
    const int* __restrict__ gate = nullptr) {
  if (gate && ((*gate != 0) != LAB)) return;           // uniform: the other variant of this launch pair does the work
  __shared__ __attribute__((aligned(16))) float sg[TPB * PASSES * 3];
  __shared__ double racc[TPB / kWave][WD_MAXC][3];
  const int n = blockIdx.y, tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  for (int e = tid; e < (TPB / kWave) * WD_MAXC * 3; e += TPB) (&racc[0][0][0])[e] = 0.0;
  const long long plane = (long long)D * H * W;
  const unsigned plane_bytes = (unsigned)(plane * 4);
  const float* gbase = grid + (long long)n * ovox * 3;
  const ChunkWalk cw = chunk_walk(blockIdx.x, gridDim.x, nchunk);
  int chunk = cw.cur;
  GridRows nxt = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  bool nfast = false;
  if (chunk < cw.end) nfast = prefetch_chunk(gbase, ovox, chunk, nxt, tid);
#pragma unroll 1
  for (; chunk < cw.end; chunk += cw.step) {
    const long long vb = (long long)chunk * CHUNK;
    const int cnt = chunk_count(ovox, vb);
    __syncthreads();                                  // the previous chunk's readers of sg are done
    commit_rows(gbase + vb * 3, cnt, nfast, nxt, sg, tid);
    __syncthreads();
    if (chunk + cw.step < cw.end)                     // the next chunk's rows: in flight under this chunk's gathers
      nfast = prefetch_chunk(gbase, ovox, chunk + cw.step, nxt, tid);
#pragma unroll 1
    for (int j0 = 0; j0 < PASSES; j0 += WD_ILP) {
      TapB q[WD_ILP];
#pragma unroll
      for (int u = 0; u < WD_ILP; ++u) chunk_tap(q[u], sg, tid + (j0 + u) * TPB, cnt, D, H, W, plane_bytes);
      LabTaps lab[WD_ILP];
      if constexpr (LAB) load_labels<WD_ILP>(labx, labf, n, plane, ovox, vb, j0, cnt, q, lab, tid);
#pragma unroll 1
      for (int c = 0; c < C; ++c) {
        float v[WD_ILP][8], tv[WD_ILP];
        corner_values<LAB, WD_ILP>(x, fixed, n, c, C, plane, plane_bytes, ovox, vb, j0, cnt, q, lab, v, tv, tid);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int u = 0; u < WD_ILP; ++u) {
          const float o = blend8(v[u], q[u].fx, q[u].fy, q[u].fz);      // 0 for lanes past the chunk (all corners read 0)
          s0 = fmaf(tv[u], o, s0); s1 = fmaf(o, o, s1); s2 = fmaf(tv[u], tv[u], s2);
        }
        s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
        if (lane == 0) { racc[wid][c][0] += (double)s0; racc[wid][c][1] += (double)s1; racc[wid][c][2] += (double)s2; }
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < C * 3; e += TPB) {
    const int c = e / 3, k = e - c * 3;
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < TPB / kWave; ++w) s += racc[w][c][k];
    partial[(((long long)n * gridDim.x + blockIdx.x) * C + c) * 3 + k] = s;
  }
}

// partial (N, nb, C, 3) -> sums (N*C, 3) floats: one wave per (n, c, k), fixed order
__global__ __launch_bounds__(TPB) void warp_dice_final_kernel(const double* __restrict__ partial, int nb, int C, int total,
                                                              float* __restrict__ sums) {
  const int e = blockIdx.x * (TPB / kWave) + (threadIdx.x >> 6);
  if (e >= total) return;
  const int lane = threadIdx.x & 63;
  const int n = e / (C * 3), r = e - n * (C * 3);
  const double* p = partial + (long long)n * nb * C * 3 + r;
  double s = 0.0;
  for (int b = lane; b < nb; b += kWave) s += p[(long long)b * C * 3];
  s = wave_sum(s);
  if (lane == 0) sums[e] = (float)s;
}

template <int WD_ILP, bool LAB = false>
__global__ __launch_bounds__(TPB) void warp_dice_grad_kernel(
    const float* __restrict__ x, const float* __restrict__ grid, const float* __restrict__ fixed,
    const float* __restrict__ ca, const float* __restrict__ cb, float* __restrict__ dgrid, int C, int D, int H, int W,
    long long ovox, int nchunk, const unsigned char* __restrict__ labx = nullptr,
    const unsigned char* __restrict__ labf = nullptr, const int* __restrict__ gate = nullptr) {
  if (gate && ((*gate != 0) != LAB)) return;
  __shared__ __attribute__((aligned(16))) float sg[TPB * PASSES * 3];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long long plane = (long long)D * H * W;
  const unsigned plane_bytes = (unsigned)(plane * 4);
  const float* gbase = grid + (long long)n * ovox * 3;
  const ChunkWalk cw = chunk_walk(blockIdx.x, gridDim.x, nchunk);
  int chunk = cw.cur;
  GridRows nxt = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  bool nfast = false;
  if (chunk < cw.end) nfast = prefetch_chunk(gbase, ovox, chunk, nxt, tid);
#pragma unroll 1
  for (; chunk < cw.end; chunk += cw.step) {
    const long long vb = (long long)chunk * CHUNK;
    const int cnt = chunk_count(ovox, vb);
    __syncthreads();                                  // the previous chunk's gradient rows have left sg
    commit_rows(gbase + vb * 3, cnt, nfast, nxt, sg, tid);
    __syncthreads();
    if (chunk + cw.step < cw.end) nfast = prefetch_chunk(gbase, ovox, chunk + cw.step, nxt, tid);
#pragma unroll 1
    for (int j0 = 0; j0 < PASSES; j0 += WD_ILP) {
      TapB q[WD_ILP];
      float gx[WD_ILP], gy[WD_ILP], gz[WD_ILP];
#pragma unroll
      for (int u = 0; u < WD_ILP; ++u) {
        chunk_tap(q[u], sg, tid + (j0 + u) * TPB, cnt, D, H, W, plane_bytes);
        gx[u] = gy[u] = gz[u] = 0.f;
      }
      LabTaps lab[WD_ILP];
      if constexpr (LAB) load_labels<WD_ILP>(labx, labf, n, plane, ovox, vb, j0, cnt, q, lab, tid);
#pragma unroll 1
      for (int c = 0; c < C; ++c) {
        const float a = ca[n * C + c], b = cb[n * C + c];
        float v[WD_ILP][8], tv[WD_ILP];
        corner_values<LAB, WD_ILP>(x, fixed, n, c, C, plane, plane_bytes, ovox, vb, j0, cnt, q, lab, v, tv, tid);
#pragma unroll
        for (int u = 0; u < WD_ILP; ++u) {
          const float o = blend8(v[u], q[u].fx, q[u].fy, q[u].fz);
          const float go = fmaf(a, tv[u], b * o);          // 0 past the chunk: tv and every corner read 0
          float dx, dy, dz;
          blend_grads(v[u], q[u].fx, q[u].fy, q[u].fz, dx, dy, dz);
          gx[u] = fmaf(dx, go, gx[u]); gy[u] = fmaf(dy, go, gy[u]); gz[u] = fmaf(dz, go, gz[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < WD_ILP; ++u) {              // coordinates in, gradient out: grad_row_out's form costs this kernel 2 VGPRs
        const int l = tid + (j0 + u) * TPB;
        float mx, my, mz;                              // d(ix)/d(gx) incl. the clamp mask, from the coordinates still in sg
        unnorm_clip(sg[l * 3], W, mx); unnorm_clip(sg[l * 3 + 1], H, my); unnorm_clip(sg[l * 3 + 2], D, mz);
        if (any_nan(sg[l * 3], sg[l * 3 + 1], sg[l * 3 + 2])) mx = my = mz = 0.f;
        sg[l * 3] = gx[u] * mx; sg[l * 3 + 1] = gy[u] * my; sg[l * 3 + 2] = gz[u] * mz;
      }
    }
    __syncthreads();
    unstage_rows(dgrid + ((long long)n * ovox + vb) * 3, cnt, sg, tid);
  }
}

// x (N, C, V) floats -> lab (N, V) bytes when every voxel is exactly one-hot (one channel == 1.0f, all others == 0.0f);
// any other voxel clears *ok (preset to 1 by the launcher; same-value stores from many threads)
__global__ __launch_bounds__(TPB) void onehot_to_labels_kernel(const float* __restrict__ x, int C, long long V,
                                                               unsigned char* __restrict__ lab, int* __restrict__ ok) {
  const int n = blockIdx.y;
  const float* xn = x + (long long)n * C * V;
  unsigned char* ln = lab + (long long)n * V;
  // 16-byte loads need every channel plane (and the byte map) aligned: V % 4 == 0 and aligned bases; else the scalar loop
  const bool vec = (V & 3) == 0 && ((reinterpret_cast<unsigned long long>(x) & 15) == 0) &&
                   ((reinterpret_cast<unsigned long long>(lab) & 3) == 0);
  const long long V4 = vec ? (V >> 2) : 0;
  bool good = true;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < V4; i += (long long)gridDim.x * TPB) {
    int ones[4] = {0, 0, 0, 0}, which[4] = {0, 0, 0, 0};
    bool clean = true;
    for (int c = 0; c < C; ++c) {
      const float4 v = *reinterpret_cast<const float4*>(xn + (long long)c * V + 4 * i);
      const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (vv[j] == 1.f) { ++ones[j]; which[j] = c; }
        else if (vv[j] != 0.f) clean = false;            // (NaN lands here too)
      }
    }
    good = good && clean && ones[0] == 1 && ones[1] == 1 && ones[2] == 1 && ones[3] == 1;
    *reinterpret_cast<unsigned*>(ln + 4 * i) = (unsigned)which[0] | ((unsigned)which[1] << 8) | ((unsigned)which[2] << 16) |
                                               ((unsigned)which[3] << 24);
  }
  if (!vec) {                                            // unaligned shapes: one voxel per thread
    for (long long v = (long long)blockIdx.x * TPB + threadIdx.x; v < V; v += (long long)gridDim.x * TPB) {
      int ones = 0, which = 0;
      for (int c = 0; c < C; ++c) {
        const float t = xn[(long long)c * V + v];
        if (t == 1.f) { ++ones; which = c; } else if (t != 0.f) good = false;
      }
      good = good && ones == 1;
      ln[v] = (unsigned char)which;
    }
  }
  if (!good) *ok = 0;
}

// the label maps and their gate come all three or not at all; returns false for a partial set, else sets `labs`
static inline bool labs_arg(const unsigned char* lab_x, const unsigned char* lab_fixed, const int* gate, bool& labs) {
  labs = lab_x && lab_fixed && gate;
  return labs || !(lab_x || lab_fixed || gate);
}

}  // namespace

/* Fused align_img + soft Dice sums: sums[(n*C + c)*3 + {0,1,2}] = {sum t p, sum p^2, sum t^2} over the output voxels, with
 * p = grid_sample(x, grid)[n, c] (bilinear, border, align_corners = False) and t = fixed[n, c]; the warped tensor is never
 * written.  Replaces keymorph/utils.py:14-21 followed by the three reductions of keymorph/loss_ops.py:28-52 (caller
 * scripts/train.py:146-164).  ws: kmh_reduce_ws_bytes().  Returns KMH_EINVAL (-22) when the lane-contiguous kernel does
 * not apply (W < 2, a plane of >= 2^31 voxels, C > 128): the caller then uses the separate entry points. */
/* The ONE statement of when the fused warp + Dice kernels apply (both entry points return -22 otherwise, and
 * kmh_warp_dice_ok lets the host decide BEFORE it builds an autograd node: the unfused composition align_img + DiceLoss is
 * the documented fallback): the lane-contiguous sampler (W >= 2, not switched off by KMH_SAMPLER_OLD), < 2^30 voxels per
 * channel plane (32-bit byte offsets), <= 128 channels (the sums' LDS table), and N * C rows whose block partials --
 * (N, nb, C, 3) doubles with nb >= 1 -- fit the reduction workspace. */
static bool warp_dice_supported(int N, int C, int D, int H, int W) {
  return N > 0 && C > 0 && C <= WD_MAXC && lane_contiguous_ok(D, H, W) && (long long)D * H * W < (1ll << 30) &&
         (long long)N * C <= 65536;
}
KMH_API int kmh_warp_dice_ok(int N, int C, int D, int H, int W) { return warp_dice_supported(N, C, D, H, W) ? 1 : 0; }

KMH_API int kmh_warp_dice_sums(const float* x, const float* grid, const float* fixed, float* sums, int N, int C, int D,
                               int H, int W, int Do, int Ho, int Wo, const unsigned char* lab_x,
                               const unsigned char* lab_fixed, const int* gate, void* ws, void* stream) {
  if (!warp_dice_supported(N, C, D, H, W)) return -22;
  bool labs;
  if (!labs_arg(lab_x, lab_fixed, gate, labs)) return -22;
  const long long ovox = (long long)Do * Ho * Wo;
  const int nchunk = ceil_div(ovox, (long long)CHUNK);
  static const int capa = env_int("KMH_WD_BLOCKS", 768);   // ~ resident blocks of the chip
  long long nb = persistent_blocks(capa, N, nchunk);
  const long long nb_cap = 65536 / ((long long)N * C);   // partial (N, nb, C, 3) doubles inside the reduction workspace
  if (nb > nb_cap) nb = nb_cap;                          // (>= 1: warp_dice_supported)
  if (nb < 1) nb = 1;
  hipStream_t s = (hipStream_t)stream;
  static const int ilp = env_int("KMH_WD_ILP_A", 4);        // A/B switch (tools/bench_warp_dice.py)
  const dim3 g((unsigned)nb, N);
  // with label maps: BOTH variants are launched with the same grid; the device flag lets exactly one of them work
  if (labs)
    warp_dice_sums_kernel<4, true><<<g, TPB, 0, s>>>(x, grid, fixed, (double*)ws, C, D, H, W, ovox, nchunk, lab_x,
                                                         lab_fixed, gate);
  if (ilp == 4)
    warp_dice_sums_kernel<4><<<g, TPB, 0, s>>>(x, grid, fixed, (double*)ws, C, D, H, W, ovox, nchunk, nullptr, nullptr,
                                                  labs ? gate : nullptr);
  else
    warp_dice_sums_kernel<2><<<g, TPB, 0, s>>>(x, grid, fixed, (double*)ws, C, D, H, W, ovox, nchunk, nullptr, nullptr,
                                                  labs ? gate : nullptr);
  const int total = N * C * 3;
  warp_dice_final_kernel<<<ceil_div(total, TPB / kWave), TPB, 0, s>>>((const double*)ws, (int)nb, C, total, sums);
  return KMH_LAUNCH_CHECK();
}

/* x (N, C, V) floats -> lab (N, V) bytes = the channel that holds the 1 when every voxel is exactly one-hot; ok[0] (device
 * int, this call only ever CLEARS it: preset it to 1, chain several tensors onto one flag) stays 1 iff that held
 * everywhere.  What keymorph/utils.py:200-240 (one_hot / one_hot_subsampled_pair) and nearest-sampled augmentation
 * (keymorph/augmentation.py:160-163) produce is exactly one-hot; a soft segmentation clears the flag and the Dice kernels
 * then read the float tensors.  C <= 255. */
KMH_API int kmh_onehot_to_labels(const float* x, int N, int C, long long V, unsigned char* lab, int* ok, void* stream) {
  if (N <= 0 || C <= 0 || C > 255 || V <= 0) return -22;
  long long nb = (V / 4 + TPB - 1) / TPB;
  if (nb > 4096) nb = 4096;
  if (nb < 1) nb = 1;
  onehot_to_labels_kernel<<<dim3((unsigned)nb, N), TPB, 0, (hipStream_t)stream>>>(x, C, V, lab, ok);
  return KMH_LAUNCH_CHECK();
}

/* d/d(grid) of sum_{n,c} g[n,c] * DiceRow[n,c] given ca[n*C+c] = -2 g / den and cb[n*C+c] = 2 g num / den^2 (num = 2 I + 1,
 * den = P + T + 1 from kmh_warp_dice_sums): dgrid[n, v, :] = sum_c (ca t + cb p) * d p / d grid, p recomputed from x.
 * Autograd of keymorph/loss_ops.py:16-63 through keymorph/utils.py:14-21 in one pass. */
KMH_API int kmh_warp_dice_bwd_grid(const float* x, const float* grid, const float* fixed, const float* ca, const float* cb,
                                   float* dgrid, int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                                   const unsigned char* lab_x, const unsigned char* lab_fixed, const int* gate, void* stream) {
  if (!warp_dice_supported(N, C, D, H, W)) return -22;
  bool labs;
  if (!labs_arg(lab_x, lab_fixed, gate, labs)) return -22;
  const long long ovox = (long long)Do * Ho * Wo;
  const int nchunk = ceil_div(ovox, (long long)CHUNK);
  static const int cap = env_int("KMH_WD_BLOCKS", 768);
  static const int ilp = env_int("KMH_WD_ILP_B", 4);      // 1.97 ms vs 2.58 (ILP 2) at 2 x 14 x 256^3
  const dim3 g((unsigned)persistent_blocks(cap, N, nchunk), N);
  hipStream_t s = (hipStream_t)stream;
  if (labs)
    warp_dice_grad_kernel<2, true><<<g, TPB, 0, s>>>(x, grid, fixed, ca, cb, dgrid, C, D, H, W, ovox, nchunk, lab_x,
                                                         lab_fixed, gate);
  if (ilp == 4)
    warp_dice_grad_kernel<4><<<g, TPB, 0, s>>>(x, grid, fixed, ca, cb, dgrid, C, D, H, W, ovox, nchunk, nullptr, nullptr,
                                                  labs ? gate : nullptr);
  else
    warp_dice_grad_kernel<2><<<g, TPB, 0, s>>>(x, grid, fixed, ca, cb, dgrid, C, D, H, W, ovox, nchunk, nullptr, nullptr,
                                                  labs ? gate : nullptr);
  return KMH_LAUNCH_CHECK();
}
