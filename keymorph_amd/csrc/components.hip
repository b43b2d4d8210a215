// Connected components of binary 3-D masks with full 26-neighbour connectivity, and the reference's clean_mask on top of
// them (keymorph/model.py:622-659: skimage.morphology.label with its default connectivity, keep a component iff
// size / max_size > threshold).  N independent samples per call; sizes, the maximum and the keep decision stay on the device.
//
// Union-find over the 13 "backward" neighbours of every set voxel on a parent array with the invariant parent[i] <= i, so
// the root of a component is its smallest raster-order index and label = root + 1 is canonical: the same on every run.
//   init    parent[i] = start of i's run of set voxels along x inside the block's 256 indices (a block-local LDS scan:
//           whole row segments are linked before any atomic), size[i] = 0                                    (one launch)
//   merge   union(i, j) for the set backward neighbours j of i that the left neighbour does not already cover
//                                                                        (one launch, atomicMin on parent)
//   flatten parent[i] = find(i) [labels[i] = root + 1 | 0]               (one launch)
//   sizes   atomicAdd(size[root], 1)   max   atomicMax(max[n], size)     keep   out = size / max > threshold    (one each)
// No workgroup ever waits on another's progress (no grid barrier, no cooperative launch, no flag): every loop below ends
// because an index strictly decreases, whatever the other workgroups do.
//
// Memory model (MI355X_MICROARCH.md "Stale without an agent-scope acquire"): a plain load may return another CU's OLDER value
// of parent[].  The merge and flatten kernels read parent[] with relaxed agent-scope atomic loads, which bypass the CU's L1;
// that keeps the chains they walk short, but correctness does NOT rest on their freshness.  What holds is the second form: the
// algorithm is PROVED CORRECT UNDER STALE READS.  parent[i] only ever decreases, and whenever it is replaced (p -> b in unite,
// p -> root in find_compress) the replacing thread goes on to join p's tree with the new value or has just walked from p to
// it, so every value parent[i] ever held ends in i's tree: a stale parent is still an ancestor-to-be with a smaller-or-equal
// index, a stale "root" is only an earlier point of the same walk, and the value atomicMin RETURNS (atomics act on the one
// coherent copy) is the truth the retry loop continues from.  Launch boundaries publish everything for the plain loads of
// the later passes.
// Integer work, bound by scattered 4-byte atomics: 1 B read + 8 B of workspace touched a few times per voxel.
#include "common.h"

namespace {
constexpr int TPB = 256;

__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of i as far as this thread can see.  Terminates: parent[x] <= x always, so every step that does not stop strictly
// decreases x, and x >= 0.
__device__ __forceinline__ int find_root(const int* parent, int i) {
  int x = i, p = ld(parent + x);
  while (p != x) { x = p; p = ld(parent + x); }
  return x;
}

// find_root, then hang i directly under the root found: r is an ancestor of i and r <= parent[i], so atomicMin keeps the
// invariant and every value parent[i] ever holds stays an ancestor.  Only NON-roots are rewritten (r != i means parent[i] < i
// already), so the "old == a" test of unite() on an apparent root is not disturbed.
__device__ __forceinline__ int find_compress(int* parent, int i) {
  const int p = ld(parent + i);
  if (p == i) return i;
  const int r = find_root(parent, p);
  if (r != p) atomicMin(parent + i, r);
  return r;
}

// Joins the trees of a and b.  Each round takes the (apparent) roots a > b and tries parent[a] = min(parent[a], b).  If the
// returned old value is a, a was a root and now hangs under b: done.  Otherwise another thread hung a under old < a in the
// meantime; since atomicMin may or may not have stored b, both old and b are now ancestors-to-be of a, so the round is
// repeated for the pair (old, b).  Terminates: max(a, b) strictly decreases from round to round (find_root never increases
// an index, and the larger one is replaced by old < a), and indices are >= 0.
__device__ __forceinline__ void unite(int* parent, int a, int b) {
  for (;;) {
    a = find_compress(parent, a);
    b = find_compress(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);
    if (old == a) return;
    a = old;
  }
}

// `continues`: voxel i is set, its left neighbour (same row) is set and lies in the same block of TPB consecutive indices
__device__ __forceinline__ bool continues(const unsigned char* m, int i, int W) {
  return (threadIdx.x > 0) && (i % W != 0) && m[i - 1];
}

// One block per TPB consecutive indices of one sample.  s = (continues ? -1 : i) under an inclusive max-scan is the start of
// i's run (every index between the start and i continues), a voxel of the same component with a smaller-or-equal index.
__global__ __launch_bounds__(TPB) void cc_init_kernel(const unsigned char* __restrict__ mask, int* __restrict__ parent_all,
                                                      int* __restrict__ size, int V, int W, int* __restrict__ bad) {
  __shared__ int s[2][TPB];
  const int i = blockIdx.x * TPB + threadIdx.x;
  const long long base = (long long)blockIdx.y * V;
  const unsigned char* m = mask + base;
  const bool in = i < V;
  const bool set = in && m[i];
  int v = (set && continues(m, i, W)) ? -1 : i;
  int cur = 0;
  s[0][threadIdx.x] = v;
  __syncthreads();
  for (int o = 1; o < TPB; o <<= 1) {           // Hillis-Steele: log2(TPB) rounds, every thread takes part in every barrier
    if ((int)threadIdx.x >= o) v = max(v, s[cur][threadIdx.x - o]);
    s[cur ^ 1][threadIdx.x] = v;
    cur ^= 1;
    __syncthreads();
  }
  if (!in) return;
  parent_all[base + i] = set ? v : i;
  size[base + i] = 0;
  if (m[i] > 1 && *bad == 0) *bad = 1;          // benign race: every writer stores the same value
}

__global__ __launch_bounds__(TPB) void cc_merge_kernel(const unsigned char* __restrict__ mask, int* __restrict__ parent_all,
                                                       int D, int H, int W) {
  const int V = D * H * W;
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= V) return;
  const unsigned char* m = mask + (long long)blockIdx.y * V;
  if (!m[i]) return;
  int* parent = parent_all + (long long)blockIdx.y * V;
  const int x = i % W, y = (i / W) % H, z = i / (W * H);
  // The 13 neighbours that precede i in raster order: (dz, dy, dx) < (0, 0, 0) lexicographically.  If the left neighbour L is
  // set it is in i's component and unites, in this same launch, with ITS backward neighbours, which include every backward
  // neighbour of i with dx <= 0: i then only needs L itself (already linked by the init when L is in the same block) and the
  // dx = +1 column.
  const bool left = x > 0 && m[i - 1];
  if (left && !continues(m, i, W)) unite(parent, i, i - 1);
  for (int dz = -1; dz <= 0; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = left ? 1 : -1; dx <= 1; ++dx) {
        if (dz == 0 && (dy > 0 || (dy == 0 && dx >= 0))) continue;
        const int zz = z + dz, yy = y + dy, xx = x + dx;
        if (zz < 0 || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        const int j = (zz * H + yy) * W + xx;
        if (m[j]) unite(parent, i, j);
      }
}

// parent[i] = root(i) in place.  Concurrent readers of parent[i] see the old ancestor or the root: both are ancestors, and
// a root's own entry never changes here, so every thread still ends at the true root (all unions completed with the
// previous launch).  labels: root + 1 for set voxels, 0 for background (may be NULL).
__global__ __launch_bounds__(TPB) void cc_flatten_kernel(const unsigned char* __restrict__ mask, int* __restrict__ parent_all,
                                                         int* __restrict__ labels, int V) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= V) return;
  const long long base = (long long)blockIdx.y * V;
  int lab = 0;
  if (mask[base + i]) {
    const int r = find_root(parent_all + base, i);
    __hip_atomic_store(parent_all + base + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    lab = r + 1;
  }
  if (labels) labels[base + i] = lab;
}

// size[root] += 1 per set voxel.  After the flatten pass the lanes of a wave mostly share one root (a big component would
// otherwise send a million atomics to ONE address), so each wave first groups its lanes by root -- leader lane, ballot of
// the lanes with the leader's root, one atomicAdd of the group's population count -- until every lane is served.  The loop
// is wave-uniform (`active` is a ballot) and ends because every round retires at least the leader.  Integer adds: any order
// gives the same sizes.
__global__ __launch_bounds__(TPB) void cc_sizes_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ parent,
                                                       int* __restrict__ size, int V) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  const long long base = (long long)blockIdx.y * V;
  const int lane = threadIdx.x & (kWave - 1);
  const int root = (i < V && mask[base + i]) ? parent[base + i] : -1;
  unsigned long long active = __ballot(root >= 0);
  while (active) {
    const int leader = __ffsll((long long)active) - 1;
    const int r = __shfl(root, leader, kWave);
    const unsigned long long same = __ballot(root == r);
    if (lane == leader) atomicAdd(size + base + r, (int)__popcll(same));
    active &= ~same;
  }
}

__global__ __launch_bounds__(TPB) void cc_max_kernel(const int* __restrict__ size, int* __restrict__ maxsz, int V) {
  __shared__ int red[TPB / kWave];
  const int i = blockIdx.x * TPB + threadIdx.x;
  int v = i < V ? size[(long long)blockIdx.y * V + i] : 0;
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < TPB / kWave; ++w) v = max(v, red[w]);
    if (v > 0) atomicMax(maxsz + blockIdx.y, v);
  }
}

// numpy's decision on two integers: size / max_size in double, strictly greater than the threshold
__global__ __launch_bounds__(TPB) void cc_keep_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ parent,
                                                      const int* __restrict__ size, const int* __restrict__ maxsz,
                                                      double threshold, unsigned char* __restrict__ out, int V) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= V) return;
  const long long base = (long long)blockIdx.y * V;
  unsigned char keep = 0;
  if (mask[base + i]) {
    const int mx = maxsz[blockIdx.y];
    const int sz = size[base + parent[base + i]];
    keep = (mx > 0 && (double)sz / (double)mx > threshold) ? 1 : 0;
  }
  out[base + i] = keep;
}

size_t info_offset(long long NV) { return ((size_t)NV * 8 + 255) & ~(size_t)255; }

int label_into(const unsigned char* mask, int* labels, int N, int D, int H, int W, void* ws, hipStream_t s) {
  const long long V = (long long)D * H * W, NV = V * N;
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || V >= (1ll << 31) || N > 65535 || !mask || !ws) return -22;
  int* parent = (int*)ws;
  int* size = parent + NV;
  int* info = (int*)((char*)ws + info_offset(NV));        // N maxima, then the "value other than 0 / 1" flag
  if (hipMemsetAsync(info, 0, (size_t)(N + 1) * sizeof(int), s) != hipSuccess) return (int)hipGetLastError();
  const dim3 g(ceil_div(V, TPB), N);
  cc_init_kernel<<<g, TPB, 0, s>>>(mask, parent, size, (int)V, W, info + N);
  cc_merge_kernel<<<g, TPB, 0, s>>>(mask, parent, D, H, W);
  cc_flatten_kernel<<<g, TPB, 0, s>>>(mask, parent, labels, (int)V);
  return KMH_LAUNCH_CHECK();
}
}  // namespace

/* parent (4 B) + size (4 B) per voxel, then N + 1 ints: the largest component size of every sample and one flag that is set
 * when the mask holds a value other than 0 / 1 (`info`, which the entry points below also copy out on request). */
KMH_API size_t kmh_components3d_ws_bytes(int N, int D, int H, int W) {
  return info_offset((long long)N * D * H * W) + (size_t)(N + 1) * sizeof(int);
}

/* mask (N, D, H, W) bytes, non-zero = set -> labels (N, D, H, W) int32: 1 + the raster-order linear index (within the
 * sample) of the component's first voxel, 0 = background.  info (N + 1 ints, may be NULL): see kmh_components3d_ws_bytes;
 * the maxima are only filled by kmh_clean_mask3d. */
KMH_API int kmh_components3d(const unsigned char* mask, int* labels, int N, int D, int H, int W, int* info, void* ws,
                             void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!labels) return -22;
  if (int e = label_into(mask, labels, N, D, H, W, ws, s)) return e;
  if (info) {
    const int* src = (const int*)((char*)ws + info_offset((long long)N * D * H * W));
    if (hipMemcpyAsync(info, src, (size_t)(N + 1) * sizeof(int), hipMemcpyDeviceToDevice, s) != hipSuccess)
      return (int)hipGetLastError();
  }
  return 0;
}

/* out (N, D, H, W) bytes = 1 where the voxel's component has size / (largest size of its sample) > threshold, else 0. */
KMH_API int kmh_clean_mask3d(const unsigned char* mask, unsigned char* out, int N, int D, int H, int W, double threshold,
                             int* info, void* ws, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!out) return -22;
  if (int e = label_into(mask, nullptr, N, D, H, W, ws, s)) return e;
  const long long V = (long long)D * H * W, NV = V * N;
  int* parent = (int*)ws;
  int* size = parent + NV;
  int* winfo = (int*)((char*)ws + info_offset(NV));
  const dim3 g(ceil_div(V, TPB), N);
  cc_sizes_kernel<<<g, TPB, 0, s>>>(mask, parent, size, (int)V);
  cc_max_kernel<<<g, TPB, 0, s>>>(size, winfo, (int)V);
  cc_keep_kernel<<<g, TPB, 0, s>>>(mask, parent, size, winfo, threshold, out, (int)V);
  if (info && hipMemcpyAsync(info, winfo, (size_t)(N + 1) * sizeof(int), hipMemcpyDeviceToDevice, s) != hipSuccess)
    return (int)hipGetLastError();
  return KMH_LAUNCH_CHECK();
}
