// kernels_tlp_order.hip — the row order of TargetLoadPacking's class form (k_tlp_fast2<..., CLS>, kernels_trimaran.hip): a counting
// sort of the pod rows by tlp_pod_milli.  Runs once per pod batch, where the column is uploaded — not in kernels_trimaran.hip, whose
// machine code stamps the counter profiles of the sweeps.
#include <hip/hip_runtime.h>

#include "spx_internal.h"

namespace spx {
namespace {

constexpr int kBlock = 1024;          // rows per block of the histogram / scatter passes, bins per step of the scan
constexpr int kSlots = 2 * kBlock;    // the block's table of distinct bins (open addressing: at most kBlock of them are taken)
constexpr uint32_t kEmpty = 0xffffffffu;

// values in [0, amb_size) have a bin of their own; everything else (negative, larger) shares the last one
__device__ __forceinline__ uint32_t order_bin(int64_t v, int32_t amb_size) {
  return (v >= 0 && v < static_cast<int64_t>(amb_size)) ? static_cast<uint32_t>(v) : static_cast<uint32_t>(amb_size);
}

// The block's rows counted per distinct bin in LDS first: a pod batch repeats a few values thousands of times (the default request),
// and one global atomic per row on such an address serialises in the L2 (0.10 ms per pass for config #2's batch; flush_stats in
// kernels_trimaran.hip met the same).  Returns the row's slot and its rank among the block's rows of the same bin; after the
// barrier skey[s] / scnt[s] hold the distinct bins and their counts.  Every thread of the block calls it.
__device__ __forceinline__ void block_count(uint32_t* skey, uint32_t* scnt, bool live, uint32_t bin, uint32_t* slot, uint32_t* rank) {
  for (int s = threadIdx.x; s < kSlots; s += kBlock) skey[s] = kEmpty, scnt[s] = 0u;
  __syncthreads();
  *slot = 0u, *rank = 0u;
  if (live) {
    uint32_t s = (bin * 2654435761u) >> 21;  // 11 bits
    for (;;) {
      const uint32_t prev = atomicCAS(skey + s, kEmpty, bin);
      if (prev == kEmpty || prev == bin) break;
      s = (s + 1u) & (kSlots - 1);
    }
    *slot = s;
    *rank = atomicAdd(scnt + s, 1u);
  }
  __syncthreads();
}
static_assert(kSlots == 2048, "block_count's hash keeps 11 bits");

__global__ __launch_bounds__(kBlock) void k_tlp_order_hist(const int64_t* pod, int64_t n, int32_t amb_size, uint32_t* hist) {
  __shared__ uint32_t skey[kSlots], scnt[kSlots];
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const bool live = r < n;
  uint32_t slot, rank;
  block_count(skey, scnt, live, live ? order_bin(pod[r], amb_size) : 0u, &slot, &rank);
  for (int s = threadIdx.x; s < kSlots; s += kBlock)
    if (skey[s] != kEmpty) atomicAdd(hist + skey[s], scnt[s]);
}

// Exclusive scan in place, one block, kBlock bins per step (coalesced; a wave scans its 64 bins with shuffles, the waves' totals meet
// in LDS): a bin's count becomes the position of its first row.  In the same pass the rows the class form evaluates among the bins
// inside the table — a bin at positions [o, o + c) holds its first position and every multiple of 64 behind it — are added to
// *evaluated, and the first position of the last bin (the rows outside the table) is left in *other_start.
__global__ __launch_bounds__(kBlock) void k_tlp_order_scan(uint32_t* hist, int n_bins, uint32_t* other_start, uint32_t* evaluated) {
  __shared__ uint32_t wsum[kBlock / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t carry = 0, ev = 0;
  for (int base = 0; base < n_bins; base += kBlock) {  // (uniform bounds: every lane takes part in the shuffles)
    const int b = base + t;
    const uint32_t c = b < n_bins ? hist[b] : 0u;
    uint32_t x = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = static_cast<uint32_t>(__shfl_up(static_cast<int>(x), d));
      if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
      const uint32_t v = wsum[w];
      before += w < wave ? v : 0u;
      total += v;
    }
    const uint32_t o = carry + before + x - c;
    if (b < n_bins) {
      hist[b] = o;
      if (b == n_bins - 1) *other_start = o;
      else if (c > 0u) ev += 1u + ((o + c - 1u) >> 6) - (o >> 6);
    }
    carry += total;
    __syncthreads();
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) ev += static_cast<uint32_t>(__shfl_xor(static_cast<int>(ev), m));
  if (lane == 0 && ev != 0u) atomicAdd(evaluated, ev);
}

__global__ __launch_bounds__(kBlock) void k_tlp_order_scatter(const int64_t* pod, int64_t n, int32_t amb_size, uint32_t* cursor, int32_t* order) {
  __shared__ uint32_t skey[kSlots], scnt[kSlots];
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const bool live = r < n;
  uint32_t slot, rank;
  block_count(skey, scnt, live, live ? order_bin(pod[r], amb_size) : 0u, &slot, &rank);
  for (int s = threadIdx.x; s < kSlots; s += kBlock)
    if (skey[s] != kEmpty) scnt[s] = atomicAdd(cursor + skey[s], scnt[s]);  // the count gives way to the block's first position in the bin
  __syncthreads();
  if (live) {
    const uint64_t pos = static_cast<uint64_t>(scnt[slot]) + rank;
    if (pos < static_cast<uint64_t>(n)) order[pos] = static_cast<int32_t>(r);  // (always: the cursors partition [0, n))
  }
}

// the rows the class form evaluates among those outside the table, whose order is whatever the scatter left: the first position of
// every chunk of 64 and every position whose value differs from the one before it — the test k_tlp_fast2<..., CLS> makes per chunk
__global__ __launch_bounds__(256) void k_tlp_order_count(const int64_t* pod, int64_t n, const int32_t* order, const uint32_t* other_start, uint32_t* evaluated) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  bool ev = false;  // no early exit: the ballot wants every lane
  if (p < n && p >= static_cast<int64_t>(*other_start)) ev = (p & 63) == 0 || p == 0 || pod[order[p]] != pod[order[p - 1]];
  const unsigned long long m = __ballot(ev);
  if ((threadIdx.x & 63) == 0 && m != 0) atomicAdd(evaluated, static_cast<uint32_t>(__builtin_popcountll(m)));
}

}  // namespace

// scratch: [amb_size + 1] bins | the last bin's first position | the rows evaluated
size_t tlp_order_scratch_words(int32_t amb_size) { return static_cast<size_t>(amb_size) + 3; }

void launch_tlp_order(const int64_t* pod_milli, int64_t n_rows, int32_t amb_size, int32_t* order, uint32_t* scratch, hipStream_t s) {
  const int n_bins = amb_size + 1;
  const unsigned blocks = static_cast<unsigned>((n_rows + kBlock - 1) / kBlock);
  (void)hipMemsetAsync(scratch, 0, tlp_order_scratch_words(amb_size) * sizeof(uint32_t), s);
  hipLaunchKernelGGL(k_tlp_order_hist, dim3(blocks), dim3(kBlock), 0, s, pod_milli, n_rows, amb_size, scratch);
  hipLaunchKernelGGL(k_tlp_order_scan, dim3(1), dim3(kBlock), 0, s, scratch, n_bins, scratch + n_bins, scratch + n_bins + 1);
  hipLaunchKernelGGL(k_tlp_order_scatter, dim3(blocks), dim3(kBlock), 0, s, pod_milli, n_rows, amb_size, scratch, order);
  hipLaunchKernelGGL(k_tlp_order_count, dim3(static_cast<unsigned>((n_rows + 255) / 256)), dim3(256), 0, s, pod_milli, n_rows, order, scratch + n_bins,
                     scratch + n_bins + 1);
}

}  // namespace spx
