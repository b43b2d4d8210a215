// Dice on integer label maps themselves (loss_ops.label_dice): the reference's fast_dice (keymorph/loss_ops.py:66-106) counts
// |x = l|, |y = l| and |x = l and y = l| per label from channel-argmax maps; a label map that was warped as a label map
// (csrc/label_warp.hip) has no channels to argmax, and ids up to 2035 (FreeSurfer aparc+aseg) cannot be given any.  Two passes
// over the maps, no (N, L, ...) tensor: which ids occur (kmh_label_presence_int, the four integer widths; kmh_label_presence of
// labels.hip is its int64-only precedent and stays), then the counts of the <= 4096 ids that do, through an id -> slot table.
// Integer work, HBM bound: both maps are read once per pass.  Integer sums: the order of the flushes cannot matter.
#include "common.h"

namespace {
constexpr int TPB = 256;

// flags[l] = 1 for every id l in [0, nflags) that occurs; flags[nflags] = 1 if any id falls outside
template <typename T>
__global__ __launch_bounds__(TPB) void label_presence_int_kernel(const T* __restrict__ seg, long long n, int nflags,
                                                                 int* __restrict__ flags) {
  const long long stride = (long long)gridDim.x * TPB;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) {
    const long long l = (long long)seg[i];
    const int slot = (l >= 0 && l < nflags) ? (int)l : nflags;
    if (flags[slot] == 0) flags[slot] = 1;      // benign race: every writer stores the same value
  }
}

// counts (3, nlab) += {|x = l|, |y = l|, |x = l and y = l|} with l the slot of the id (slot_of[id], ids in [0, nids)); an id
// outside the table or a slot outside [0, nlab) is not counted (the presence pass has refused such maps before this runs).
// Per-workgroup LDS tables of 32-bit counts (a workgroup reads far fewer than 2^32 voxels), flushed with 64-bit atomics.
template <typename T>
__global__ __launch_bounds__(TPB) void label_pair_counts_kernel(const T* __restrict__ x, const T* __restrict__ y, long long n,
                                                                const unsigned short* __restrict__ slot_of, int nids, int nlab,
                                                                unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned hist[];     // 3 x nlab
  for (int i = threadIdx.x; i < 3 * nlab; i += TPB) hist[i] = 0u;
  __syncthreads();
  const long long stride = (long long)gridDim.x * TPB;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) {
    const long long lx = (long long)x[i], ly = (long long)y[i];
    const int sx = (lx >= 0 && lx < nids) ? (int)slot_of[lx] : nlab;
    const int sy = (ly >= 0 && ly < nids) ? (int)slot_of[ly] : nlab;
    if (sx < nlab) atomicAdd(&hist[sx], 1u);
    if (sy < nlab) atomicAdd(&hist[nlab + sy], 1u);
    if (lx == ly && sx < nlab) atomicAdd(&hist[2 * nlab + sx], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * nlab; i += TPB)
    if (hist[i]) atomicAdd(&counts[i], (unsigned long long)hist[i]);
}

// elem_bytes 1 is unsigned (uint8, bool), 2 / 4 / 8 are signed: the label maps of csrc/label_warp.hip
static bool int_type_ok(int elem_bytes, int is_signed) {
  return (elem_bytes == 1 && !is_signed) || ((elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8) && is_signed);
}
static int blocks_for(long long n, int per_thread, int cap) {
  long long nb = (n + (long long)TPB * per_thread - 1) / ((long long)TPB * per_thread);
  return (int)(nb > cap ? cap : nb);
}
}  // namespace

/* kmh_label_presence for the integer widths: seg holds n ids of elem_bytes 1 (unsigned) or 2 / 4 / 8 (signed); flags
 * (nflags + 1 ints, zeroed by the caller, or carrying an earlier call's flags: the call only ever sets them) gets
 * flags[l] = 1 iff id l occurs, flags[nflags] = 1 iff an id lies outside [0, nflags). */
KMH_API int kmh_label_presence_int(const void* seg, int elem_bytes, int is_signed, long long n, int nflags, int* flags,
                                   void* stream) {
  if (!seg || !flags || n <= 0 || nflags <= 0 || !int_type_ok(elem_bytes, is_signed)) return -22;
  const int nb = blocks_for(n, 8, 4096);
  hipStream_t s = (hipStream_t)stream;
  switch (elem_bytes) {
    case 1: label_presence_int_kernel<unsigned char><<<nb, TPB, 0, s>>>((const unsigned char*)seg, n, nflags, flags); break;
    case 2: label_presence_int_kernel<short><<<nb, TPB, 0, s>>>((const short*)seg, n, nflags, flags); break;
    case 4: label_presence_int_kernel<int><<<nb, TPB, 0, s>>>((const int*)seg, n, nflags, flags); break;
    default: label_presence_int_kernel<long long><<<nb, TPB, 0, s>>>((const long long*)seg, n, nflags, flags); break;
  }
  return KMH_LAUNCH_CHECK();
}

/* x, y: two label maps of n ids each, one element type (as kmh_label_presence_int).  slot_of: nids entries, the slot in
 * [0, nlab) of every id that occurs (any value >= nlab: the id is not counted); nlab <= 4096.  counts (3 * nlab uint64, zeroed
 * by the caller) = {|x = l|, |y = l|, |x = l and y = l|} per slot: kmh_label_counts without the channels. */
KMH_API int kmh_label_pair_counts(const void* x, const void* y, int elem_bytes, int is_signed, long long n,
                                  const unsigned short* slot_of, int nids, int nlab, unsigned long long* counts, void* stream) {
  if (!x || !y || !slot_of || !counts || n <= 0 || nids <= 0 || nlab < 1 || nlab > 4096 || !int_type_ok(elem_bytes, is_signed))
    return -22;
  const int nb = blocks_for(n, 16, 2048);
  const size_t lds = (size_t)3 * nlab * 4;
  hipStream_t s = (hipStream_t)stream;
  switch (elem_bytes) {
    case 1:
      label_pair_counts_kernel<unsigned char><<<nb, TPB, lds, s>>>((const unsigned char*)x, (const unsigned char*)y, n, slot_of,
                                                                     nids, nlab, counts);
      break;
    case 2:
      label_pair_counts_kernel<short><<<nb, TPB, lds, s>>>((const short*)x, (const short*)y, n, slot_of, nids, nlab, counts);
      break;
    case 4:
      label_pair_counts_kernel<int><<<nb, TPB, lds, s>>>((const int*)x, (const int*)y, n, slot_of, nids, nlab, counts);
      break;
    default:
      label_pair_counts_kernel<long long><<<nb, TPB, lds, s>>>((const long long*)x, (const long long*)y, n, slot_of, nids, nlab,
                                                                 counts);
      break;
  }
  return KMH_LAUNCH_CHECK();
}
