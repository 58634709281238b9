// kernels_node_columns.hip — NodeMetadata (pkg/nodemetadata/node_metadata.go) and PodState (pkg/podstate/pod_state.go): plugins whose
// Score is one int64 per node, the same for every pod, and whose NormalizeScore is a min-max over the nodes it is handed.
//
// Upstream hands NormalizeScore the nodes that passed the cycle's Filters, so the bytes of a row depend on the pod as soon as a Filter
// plugin or a caller's mask is in play (as for Allocatable, kernels_profile.hip).  Two regimes:
//   no Filter   : k_node_rows normalises the column once (one workgroup, one row, no status table) into a scratch row, and
//                 k_node_broadcast writes that row into [row_begin, row_end) — 16 bytes per lane and store, a 4 KiB tile of the row held
//                 in registers over the rows of a wave;
//   Filters     : k_node_rows, one wave per pod row (a whole workgroup when the call is for one row): pass 1 takes min and max over the
//                 nodes that are feasible (and, NodeMetadata, valid), pass 2 writes the row.  The status bytes are read as dwords, 4 nodes
//                 per lane; the raw column is N x 8 bytes and stays in L2.
//
// One rule set, two parameterisations (all arithmetic int64 as Go performs it: wrapping difference and product, a quotient
// truncating toward zero, the byte = the reference's value clamped to [0, 255]):
//                   valid range                     all valid equal   invalid cell   no valid cell in the row
//   NodeMetadata    (s - min) * 99 / (max - min) + 1        1              0          every cell 0           node_metadata.go:150-210
//   PodState        (s - lo) * 100 / (hi - lo)               0             n/a         n/a (nothing to write: 0)   pod_state.go:66-91
// Every cell of a row is written by the same rule, the cells of infeasible nodes included (NodeMetadata: an invalid node's cell is 0
// whether feasible or not); only the cells of feasible nodes mean anything.
//
// The quotient.  For 0 <= d <= R, R = max - min in [1, 2^40) and K in {99, 100}: with b = RN(K / R) * (1 + 2^-49) the float64 product
// RN(d * b) lies in [x, x * (1 + 2^-48)) for x = d * K / R (d < 2^40 converts exactly; three roundings of 2^-53 each against the
// 2^-49 pushed in), so it is at least x and exceeds it by less than 100 * 2^-48 < 2^-41 < 1 / R, while frac(x) <= 1 - 1 / R when
// x is no integer: floor(RN(d * b)) = floor(x), the reference's quotient (nothing wraps below 2^40 * 100).  Rows with a wider or
// a wrapped (negative) range, and the cells of infeasible nodes outside [min, max], take the plain int64 sequence.  The choice is
// per row, hence wave-uniform.
//
// Also here: the two key-building kernels of QOSSort (spx_qos_sort, spx_uploads.hip), around kernels_sort.hip's radix passes.
#include "spx_internal.h"

namespace spx {

namespace {

constexpr int kMaxRowWaves = 16;  // waves a single-row launch puts on its row
constexpr int kRowsPerBlock = 4;  // rows per workgroup of a batch launch, one wave each
constexpr int kNpl = 4;           // nodes per lane and tile: one dword per status table

__device__ __forceinline__ int64_t shfl_xor_i64(int64_t v, int m) {
  const int lo = __shfl_xor(static_cast<int>(v & 0xffffffffLL), m, 64);
  const int hi = __shfl_xor(static_cast<int>(v >> 32), m, 64);
  return (static_cast<int64_t>(hi) << 32) | static_cast<uint32_t>(lo);
}

// OR of the Filter status bytes of nodes n0..n0+3 (n0 a multiple of 4 inside the padded row); bytes past n_nodes are the caller's to ignore
__device__ __forceinline__ uint32_t infeasible4(const NodeColArgs& a, int64_t pod, int64_t n0) {
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (a.status[k]) w |= *reinterpret_cast<const uint32_t*>(a.status[k] + pod * a.row_stride + n0);
  return w;
}

// the reference's sequence for one cell: ((s - lo) * K) / (hi - lo) + base, wrapping, truncating, clamped to a byte
__device__ __forceinline__ uint32_t cell_plain(uint64_t d, uint64_t range, uint64_t k, uint64_t base) {
  const int64_t num = static_cast<int64_t>(d * k), den = static_cast<int64_t>(range);
  const int64_t q = den == -1 ? static_cast<int64_t>(0 - static_cast<uint64_t>(num)) : num / den;  // (Go: MinInt64 / -1 wraps)
  const int64_t v = static_cast<int64_t>(static_cast<uint64_t>(q) + base);
  return v < 0 ? 0u : (v > 255 ? 255u : static_cast<uint32_t>(v));
}

template <int KIND>
__global__ __launch_bounds__(64 * kMaxRowWaves) void k_node_rows(NodeColArgs a) {
  const bool single = a.row_end - a.row_begin == 1 || a.block_per_row;  // uniform
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t pod = single ? a.row_begin + static_cast<int64_t>(blockIdx.x) : a.row_begin + static_cast<int64_t>(blockIdx.x) * kRowsPerBlock + w;
  const int wave = single ? w : 0, n_waves = single ? static_cast<int>(blockDim.x >> 6) : 1;
  if (pod >= a.row_end) return;  // wave-uniform; a batch launch has no workgroup barrier
  constexpr bool kMeta = KIND == kNodeColMeta;
  constexpr uint64_t kMul = kMeta ? 99 : 100, kBase = kMeta ? 1 : 0;
  const int64_t tiles = (a.row_stride + 64 * kNpl - 1) / (64 * kNpl);
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  bool any = false;
  for (int64_t t = wave; t < tiles; t += n_waves) {
    const int64_t n0 = (t * 64 + lane) * kNpl;
    if (n0 >= a.n_nodes) continue;
    const uint32_t bad = infeasible4(a, pod, n0);
#pragma unroll
    for (int j = 0; j < kNpl; ++j) {
      const int64_t n = n0 + j;
      if (n >= a.n_nodes || ((bad >> (8 * j)) & 0xffu)) continue;
      const int64_t s = a.raw[n];
      if (kMeta && s == INT64_MIN) continue;  // invalidScore takes no part in the bounds
      lo = s < lo ? s : lo;
      hi = s > hi ? s : hi;
      any = true;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int64_t olo = shfl_xor_i64(lo, m), ohi = shfl_xor_i64(hi, m);
    lo = olo < lo ? olo : lo;
    hi = ohi > hi ? ohi : hi;
  }
  bool some = __ballot(any) != 0;
  if (n_waves > 1) {  // a whole workgroup on one row: combine the waves
    __shared__ int64_t s_lo[kMaxRowWaves], s_hi[kMaxRowWaves];
    __shared__ uint32_t s_any[kMaxRowWaves];
    if (lane == 0) s_lo[wave] = lo, s_hi[wave] = hi, s_any[wave] = some ? 1u : 0u;
    __syncthreads();
    lo = INT64_MAX, hi = INT64_MIN, some = false;
    for (int k = 0; k < n_waves; ++k) {
      lo = s_lo[k] < lo ? s_lo[k] : lo;
      hi = s_hi[k] > hi ? s_hi[k] : hi;
      some |= s_any[k] != 0;
    }
  }
  const uint64_t range = some ? static_cast<uint64_t>(hi) - static_cast<uint64_t>(lo) : 0;  // max - min as Go's int64 holds it (may have wrapped)
  const bool fast = static_cast<int64_t>(range) > 0 && range < (1ull << 40);
  const double b = fast ? (static_cast<double>(kMul) / static_cast<double>(range)) * (1.0 + 0x1p-49) : 0.0;
  uint8_t* out = a.out_score + pod * a.row_stride;
  for (int64_t t = wave; t < tiles; t += n_waves) {
    const int64_t n0 = (t * 64 + lane) * kNpl;
    if (n0 >= a.row_stride) continue;
    uint32_t word = 0;
    if (n0 < a.n_nodes && some) {
#pragma unroll
      for (int j = 0; j < kNpl; ++j) {
        const int64_t n = n0 + j;
        if (n >= a.n_nodes) continue;
        const int64_t s = a.raw[n];
        if (kMeta && s == INT64_MIN) continue;  // 0: reserved for nodes without valid metadata
        uint32_t v;
        const uint64_t d = static_cast<uint64_t>(s) - static_cast<uint64_t>(lo);
        if (range == 0) v = static_cast<uint32_t>(kBase);
        else if (fast && d <= range) v = static_cast<uint32_t>(static_cast<double>(static_cast<int64_t>(d)) * b) + static_cast<uint32_t>(kBase);
        else v = cell_plain(d, range, kMul, kBase);
        word |= v << (8 * j);
      }
    }
    *reinterpret_cast<uint32_t*>(out + n0) = word;
  }
}

// the pod-independent row into rows [row_begin, row_end): a workgroup takes a 4 KiB tile of the row (4 x 16 bytes per lane, every
// store of a wave 1 KiB contiguous) and kBroadcastRows rows, its 4 waves taking every fourth of them
constexpr int kBroadcastVec = 4;
constexpr int kBroadcastRows = 64;
__global__ __launch_bounds__(256) void k_node_broadcast(const uint8_t* __restrict__ row, uint8_t* __restrict__ out, int64_t row_stride, int64_t row_begin,
                                                       int64_t row_end) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t col0 = static_cast<int64_t>(blockIdx.x) * (64 * 16 * kBroadcastVec) + lane * 16;
  uint4 v[kBroadcastVec];
#pragma unroll
  for (int j = 0; j < kBroadcastVec; ++j) {
    const int64_t c = col0 + j * 64 * 16;
    v[j] = c < row_stride ? *reinterpret_cast<const uint4*>(row + c) : uint4{0, 0, 0, 0};  // row_stride is a multiple of 16
  }
  const int64_t r0 = row_begin + static_cast<int64_t>(blockIdx.y) * kBroadcastRows;
  const int64_t r1 = r0 + kBroadcastRows < row_end ? r0 + kBroadcastRows : row_end;
  for (int64_t r = r0 + wave; r < r1; r += 4) {
    uint8_t* dst = out + r * row_stride + col0;
#pragma unroll
    for (int j = 0; j < kBroadcastVec; ++j)
      if (col0 + j * 64 * 16 < row_stride) *reinterpret_cast<uint4*>(dst + j * 64 * 16) = v[j];
  }
}

__global__ __launch_bounds__(256) void k_qos_class_keys(const uint8_t* __restrict__ qos, int64_t n, int32_t* cls, int32_t* none, int32_t* zero) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  cls[i] = qos[i];
  none[i] = -1;
  zero[i] = 0;
}

__global__ __launch_bounds__(256) void k_qos_rank_keys(const int32_t* __restrict__ perm, int64_t n, int64_t* rank) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) rank[perm[i]] = i;  // perm is a permutation of [0, n)
}

template <int KIND>
void launch_rows(const NodeColArgs& a, hipStream_t s) {
  const unsigned rows = static_cast<unsigned>(a.row_end - a.row_begin);
  const bool whole = rows == 1 || a.block_per_row;
  NodeColArgs b = a;
  b.block_per_row = whole && rows > 1;
  hipLaunchKernelGGL(k_node_rows<KIND>, dim3(whole ? rows : (rows + kRowsPerBlock - 1) / kRowsPerBlock), dim3(whole ? 64u * kMaxRowWaves : 64u * kRowsPerBlock), 0, s, b);
}

}  // namespace

void launch_node_column(const NodeColArgs& a, hipStream_t s) {
  if (a.row_end <= a.row_begin) return;
  const bool meta = a.kind == kNodeColMeta;
  if (a.status[0] || a.status[1] || a.status[2]) {
    if (meta) launch_rows<kNodeColMeta>(a, s);
    else launch_rows<kNodeColPodState>(a, s);
    return;
  }
  NodeColArgs one = a;  // the column, normalised over every node, as row 0 of the scratch row
  one.row_begin = 0, one.row_end = 1, one.block_per_row = 0;
  one.out_score = a.norm_row;
  if (meta) launch_rows<kNodeColMeta>(one, s);
  else launch_rows<kNodeColPodState>(one, s);
  const unsigned col_tiles = static_cast<unsigned>((a.row_stride + 64 * 16 * kBroadcastVec - 1) / (64 * 16 * kBroadcastVec));
  // (the grid's y holds 65 535 groups of kBroadcastRows rows: 4.19 M rows per launch)
  constexpr int64_t kRowsPerLaunch = int64_t{65535} * kBroadcastRows;
  for (int64_t r = a.row_begin; r < a.row_end; r += kRowsPerLaunch) {
    const int64_t end = r + kRowsPerLaunch < a.row_end ? r + kRowsPerLaunch : a.row_end;
    hipLaunchKernelGGL(k_node_broadcast, dim3(col_tiles, static_cast<unsigned>((end - r + kBroadcastRows - 1) / kBroadcastRows)), dim3(256), 0, s, a.norm_row,
                       a.out_score, a.row_stride, r, end);
  }
}

void launch_qos_class_keys(const uint8_t* qos, int64_t n, int32_t* cls_out, int32_t* none_out, int32_t* zero_out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_qos_class_keys, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, qos, n, cls_out, none_out, zero_out);
}

void launch_qos_rank_keys(const int32_t* perm, int64_t n, int64_t* rank_out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_qos_rank_keys, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, perm, n, rank_out);
}

}  // namespace spx
