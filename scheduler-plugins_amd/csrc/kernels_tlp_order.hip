// kernels_tlp_order.hip — the row order of TargetLoadPacking's class form (k_tlp_fast2<..., CLS>, kernels_trimaran.hip): a counting
// sort of the pod rows by tlp_pod_milli, then its chunks of 64 positions put in the order the sweep should launch them in (heaviest
// first).  Runs once per pod batch, where the column is uploaded — not in kernels_trimaran.hip, whose
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

// the sum of v over the block, in every thread (wsum: one word per wave; two barriers, so the same wsum serves the next call)
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* wsum) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), m));
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t total = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) total += wsum[w];
  __syncthreads();
  return total;
}

// The exclusive scan of the bins, over many blocks (one block walking all 65 537 bins took 0.063 ms of the build's 0.11): first the
// count of each block's kBlock bins ...
__global__ __launch_bounds__(kBlock) void k_tlp_order_totals(const uint32_t* hist, int n_bins, uint32_t* totals) {
  __shared__ uint32_t wsum[kBlock / 64];
  const int b = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t total = block_sum(b < n_bins ? hist[b] : 0u, wsum);
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// ... then, per block, the totals of the blocks before it (the prologue) and the scan of its own bins in place (coalesced; a wave scans
// its 64 bins with shuffles, the waves' totals meet in LDS): a bin's count becomes the position of its first row.  In the same pass the
// rows the class form evaluates among the bins inside the table — a bin at positions [o, o + c) holds its first position and every
// multiple of 64 behind it — are added to *evaluated (one atomic per block), and the first position of the last bin (the rows outside
// the table) is left in *other_start.
__global__ __launch_bounds__(kBlock) void k_tlp_order_scan(uint32_t* hist, int n_bins, const uint32_t* totals, uint32_t* other_start, uint32_t* evaluated) {
  __shared__ uint32_t wsum[kBlock / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t mine = 0;
  for (int i = t; i < static_cast<int>(blockIdx.x); i += kBlock) mine += totals[i];
  const uint32_t carry = block_sum(mine, wsum);
  const int b = blockIdx.x * kBlock + t;
  const uint32_t c = b < n_bins ? hist[b] : 0u;
  uint32_t x = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {  // (every lane takes part in the shuffles)
    const uint32_t y = static_cast<uint32_t>(__shfl_up(static_cast<int>(x), d));
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  uint32_t before = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) before += w < wave ? wsum[w] : 0u;
  __syncthreads();
  const uint32_t o = carry + before + x - c;
  uint32_t ev = 0;
  if (b < n_bins) {
    hist[b] = o;
    if (b == n_bins - 1) *other_start = o;
    else if (c > 0u) ev = 1u + ((o + c - 1u) >> 6) - (o >> 6);
  }
  ev = block_sum(ev, wsum);
  if (t == 0 && ev != 0u) atomicAdd(evaluated, ev);
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

// One pass over the positions of the sorted order (a wave = a chunk of 64, as in k_tlp_fast2<..., CLS>), with the test that kernel
// makes per chunk: a position is evaluated when it is the first of its chunk or its value differs from the one before it.
//   - the evaluated positions among the rows outside the table, whose order is whatever the scatter left, are added to *evaluated
//     (the scan counted the ones inside);
//   - keys[chunk] = the chunk's evaluated positions — what its wave will cost — or 64 when it holds any value outside the table
//     (whole chunks only: the last, partial one is not scheduled).
__global__ __launch_bounds__(256) void k_tlp_order_count_key(const int64_t* pod, int64_t n, int32_t amb_size, const int32_t* order, const uint32_t* other_start,
                                                             uint32_t* evaluated, uint32_t* keys, int64_t n_chunks) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const uint32_t last = static_cast<uint32_t>(n - 1);
  bool ev = false, outside = false;  // no early exit: the ballots want every lane
  if (p < n) {
    const int64_t v = pod[min(static_cast<uint32_t>(order[p]), last)];
    ev = (p & 63) == 0 || v != pod[min(static_cast<uint32_t>(order[p - 1]), last)];
    outside = order_bin(v, amb_size) == static_cast<uint32_t>(amb_size);
  }
  const unsigned long long m = __ballot(ev), mo = __ballot(ev && p >= static_cast<int64_t>(*other_start)), out = __ballot(outside);
  if ((threadIdx.x & 63) == 0) {
    if (mo != 0) atomicAdd(evaluated, static_cast<uint32_t>(__builtin_popcountll(mo)));
    if ((p >> 6) < n_chunks) keys[p >> 6] = out != 0 ? 64u : static_cast<uint32_t>(__builtin_popcountll(m));
  }
}

// The chunk schedule (SPX_OPT_TLP_CHUNK_SCHED): a stable counting sort of the whole chunks by descending key, one block —
// dest[chunk] = the chunk's place in the launch.  k_tlp_fast2 maps unit -> chunk in launch order, and a wave with e evaluated positions
// issues about 100 e + 15 (64 - e) instructions; in value order the heaviest chunks (the batch's rare large values) come last, and the
// grid drains through them while the store queues run empty.  Heaviest first, the tail is waves that only store.  (Heavy and light
// chunks alternating measured better than heaviest first in tools/micro/wcls.hip and worse in the sweep: profiles/r11/tlp_tail_ab.md.)
//   Keys are 1..64 (bins 0..64).  Pass 1 counts the bins in LDS; pass 2 walks the chunks kBlock at a time, in order: a chunk's rank
// among its round's chunks of the same key is (those in the waves before: wcnt) + (those in the lanes before: the ballots), which keeps
// the sort stable.  (One block: 5 us for the 1 562 chunks of 100 000 rows, linear in the chunks.)
constexpr int kKeyBins = 65;
__global__ __launch_bounds__(kBlock) void k_tlp_order_sched(const uint32_t* keys, int64_t n_chunks, uint32_t* dest) {
  __shared__ uint32_t base[kKeyBins], wcnt[kBlock / 64][kKeyBins];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int k = t; k < kKeyBins; k += kBlock) base[k] = 0u;
  for (int k = t; k < (kBlock / 64) * kKeyBins; k += kBlock) (&wcnt[0][0])[k] = 0u;
  __syncthreads();
  for (int64_t c = t; c < n_chunks; c += kBlock) atomicAdd(base + min(keys[c], 64u), 1u);
  __syncthreads();
  if (t == 0) {  // counts -> first place of each key, largest key first
    uint32_t at = 0;
    for (int k = kKeyBins - 1; k >= 0; --k) {
      const uint32_t n = base[k];
      base[k] = at;
      at += n;
    }
  }
  __syncthreads();
  for (int64_t c0 = 0; c0 < n_chunks; c0 += kBlock) {  // (uniform bounds: every lane takes part in the ballots and barriers)
    const int64_t c = c0 + t;
    const bool live = c < n_chunks;
    const uint32_t key = live ? min(keys[c], 64u) : 127u;  // (127: no live lane's peer)
    unsigned long long peers = ~0ull;
#pragma unroll
    for (int b = 0; b < 7; ++b) {
      const bool bit = (key >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const uint32_t rank = static_cast<uint32_t>(__builtin_popcountll(peers & ((1ull << lane) - 1ull)));
    if (live && rank == 0u) wcnt[wave][key] = static_cast<uint32_t>(__builtin_popcountll(peers));
    __syncthreads();
    if (live) {
      uint32_t before = 0;
      for (int w = 0; w < wave; ++w) before += wcnt[w][key];
      dest[c] = base[key] + before + rank;
    }
    __syncthreads();
    if (t < kKeyBins) {
      uint32_t add = 0;
#pragma unroll
      for (int w = 0; w < kBlock / 64; ++w) add += wcnt[w][t], wcnt[w][t] = 0u;
      base[t] += add;
    }
    __syncthreads();
  }
}

// The sorted order moved to where the sweep reads it, whole chunks to their scheduled place (dest; the last, partial chunk always stays
// last).
__global__ __launch_bounds__(256) void k_tlp_order_move(int64_t n, const int32_t* sorted, const uint32_t* dest, int64_t n_chunks, int32_t* order) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= n) return;
  int64_t chunk = p >> 6;
  if (chunk < n_chunks) chunk = min(static_cast<int64_t>(dest[chunk]), n_chunks - 1);  // (always below n_chunks: a permutation)
  order[chunk * 64 + (p & 63)] = sorted[p];
}

}  // namespace

// scratch: [amb_size + 1] bins | the last bin's first position | the rows evaluated | the scan's block totals | per whole chunk: key,
// scheduled place | [n_rows] the sorted order before the move
static size_t scan_blocks(int32_t amb_size) { return (static_cast<size_t>(amb_size) + 1 + kBlock - 1) / kBlock; }
size_t tlp_order_scratch_words(int32_t amb_size, int64_t n_rows) {
  return static_cast<size_t>(amb_size) + 3 + scan_blocks(amb_size) + 2 * static_cast<size_t>(n_rows / 64) + static_cast<size_t>(n_rows);
}
size_t tlp_order_evaluated_word(int32_t amb_size) { return static_cast<size_t>(amb_size) + 2; }

void launch_tlp_order(const int64_t* pod_milli, int64_t n_rows, int32_t amb_size, bool chunk_sched, int32_t* order, uint32_t* scratch, hipStream_t s) {
  const int n_bins = amb_size + 1;
  const unsigned blocks = static_cast<unsigned>((n_rows + kBlock - 1) / kBlock), rows256 = static_cast<unsigned>((n_rows + 255) / 256);
  const unsigned sblocks = static_cast<unsigned>(scan_blocks(amb_size));
  const int64_t n_chunks = n_rows / 64;
  uint32_t* other_start = scratch + n_bins;
  uint32_t* evaluated = other_start + 1;
  uint32_t* totals = evaluated + 1;
  uint32_t* keys = totals + sblocks;
  uint32_t* dest = keys + n_chunks;
  const bool sched = chunk_sched && n_chunks > 1;
  int32_t* sorted = sched ? reinterpret_cast<int32_t*>(dest + n_chunks) : order;  // (value order: the scatter writes the order itself)
  (void)hipMemsetAsync(scratch, 0, (static_cast<size_t>(n_bins) + 2) * sizeof(uint32_t), s);
  hipLaunchKernelGGL(k_tlp_order_hist, dim3(blocks), dim3(kBlock), 0, s, pod_milli, n_rows, amb_size, scratch);
  hipLaunchKernelGGL(k_tlp_order_totals, dim3(sblocks), dim3(kBlock), 0, s, scratch, n_bins, totals);
  hipLaunchKernelGGL(k_tlp_order_scan, dim3(sblocks), dim3(kBlock), 0, s, scratch, n_bins, totals, other_start, evaluated);
  hipLaunchKernelGGL(k_tlp_order_scatter, dim3(blocks), dim3(kBlock), 0, s, pod_milli, n_rows, amb_size, scratch, sorted);
  hipLaunchKernelGGL(k_tlp_order_count_key, dim3(rows256), dim3(256), 0, s, pod_milli, n_rows, amb_size, sorted, other_start, evaluated, keys, n_chunks);
  if (!sched) return;
  hipLaunchKernelGGL(k_tlp_order_sched, dim3(1), dim3(kBlock), 0, s, keys, n_chunks, dest);
  hipLaunchKernelGGL(k_tlp_order_move, dim3(rows256), dim3(256), 0, s, n_rows, sorted, dest, n_chunks, order);
}

}  // namespace spx
