// kernels_cosched.hip — Coscheduling's PreFilter gate (pkg/coscheduling/core/core.go:243-305, :406-467) for every PodGroup and pending pod.
//
// CheckClusterResource subtracts the nodes' left-overs from the request in list order and drops a resource for good the first time it is
// <= 0, so a group passes iff every resource it names has a present node i whose prefix sum S_g,r[i] of left-overs reaches the request
// (DESIGN.md 3.9b).  S_g,r = S_base,r + step_g,r: the prefix sums of the snapshot, plus what the group's own assigned pods give back from
// their node onwards.
//   k_cosched_scan       one workgroup per slot: int64 inclusive prefix sums of left_base over the present nodes, chunk by chunk with a carry,
//                        their maximum over the present nodes, and the total
//   k_cosched_gate_flat  a thread per group without assigned pods: the slot's overall maximum against the request
//   k_cosched_gate_walk  a workgroup per group with assigned pods: max over present i of S_base,r[i] + step_g,r(i) by a dense walk over
//                        the nodes, the group's steps (node, cumulative add-back per slot) staged in LDS a tile at a time
//   k_cosched_status     a thread per pending pod: the ordered checks of PreFilter, one byte
//   k_cosched_unschedulable  after an argmax: the decision rows of pods whose gate failed become "no node"
// Plain integer vector code on a few MB; everything is exact in int64 (the upload bounds every sum by 2^62).
#include "spx_internal.h"

namespace spx {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxSlots = SPX_COSCHED_MAX_SLOTS;
constexpr int kStepTile = 128;  // steps of a group in LDS at a time: 128 x (4 + 16 x 8) B = 16.5 KiB

__device__ __forceinline__ int64_t shfl_up64(int64_t v, int d) { return static_cast<int64_t>(__shfl_up(static_cast<long long>(v), static_cast<unsigned>(d), 64)); }
__device__ __forceinline__ int64_t shfl_xor64(int64_t v, int m) { return static_cast<int64_t>(__shfl_xor(static_cast<long long>(v), m, 64)); }
__device__ __forceinline__ int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

__device__ __forceinline__ int64_t wave_max(int64_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max64(v, shfl_xor64(v, m));
  return v;
}

__global__ __launch_bounds__(kBlock) void k_cosched_scan(CoschedArgs a) {
  __shared__ int64_t wave_sum[kWaves];
  __shared__ int64_t wave_best[kWaves];
  __shared__ int wave_any[kWaves];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t N = a.n_nodes;
  const int64_t* left = a.left_base + static_cast<int64_t>(s) * N;
  int64_t* prefix = a.prefix + static_cast<int64_t>(s) * N;
  int64_t carry = 0, best = INT64_MIN;
  int any = 0;
  for (int64_t base = 0; base < N; base += kBlock) {
    const int64_t i = base + tid;
    const bool present = i < N && a.node_present[i] != 0;  // an absent node adds nothing and is no prefix of its own
    int64_t v = present ? left[i] : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t up = shfl_up64(v, d);
      if (lane >= d) v += up;
    }
    if (lane == 63) wave_sum[wave] = v;
    __syncthreads();
    int64_t before = carry, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) before += wave_sum[w];
      total += wave_sum[w];
    }
    v += before;
    if (i < N) prefix[i] = v;
    if (present) best = max64(best, v), any = 1;
    carry += total;
    __syncthreads();  // wave_sum is rewritten by the next chunk
  }
  best = wave_max(best);
  any = __any(any);
  if (lane == 0) wave_best[wave] = best, wave_any[wave] = any;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kWaves; ++w) best = max64(best, wave_best[w]), any |= wave_any[w];
    a.slot_max[s] = best;
    a.slot_total[s] = carry;
    if (s == 0) *a.any_present = any;
  }
}

// the verdict of one group from its per-slot maxima: pass / open bits and the closing gap
__device__ void write_verdict(const CoschedArgs& a, int g, uint32_t mask, const int64_t* best, const int64_t* last, bool any) {
  const int S = a.n_slots;
  uint32_t pass = 0, open = 0;
  for (int r = 0; r < S; ++r) {
    int64_t gap = 0;
    if ((mask >> r) & 1u) {
      const int64_t req = a.req[static_cast<int64_t>(g) * S + r];
      if (any && best[r] >= req) pass |= 1u << r;
      else open |= 1u << r, gap = req - last[r];  // with no present node nothing was subtracted: last = 0
    }
    a.gap[static_cast<int64_t>(g) * S + r] = gap;
  }
  a.pass_mask[g] = pass;
  a.open_mask[g] = open;
}

__global__ __launch_bounds__(kBlock) void k_cosched_gate_flat(CoschedArgs a) {
  const int g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= a.n_groups) return;
  if (a.step_ptr[g + 1] > a.step_ptr[g]) return;  // k_cosched_gate_walk's
  const bool any = *a.any_present != 0;
  int64_t best[kMaxSlots], last[kMaxSlots];
  for (int r = 0; r < a.n_slots; ++r) best[r] = a.slot_max[r], last[r] = any ? a.slot_total[r] : 0;
  write_verdict(a, g, a.req_mask[g], best, last, any);
}

__global__ __launch_bounds__(kBlock) void k_cosched_gate_walk(CoschedArgs a) {
  __shared__ int32_t s_node[kStepTile];
  __shared__ int64_t s_cum[kStepTile * kMaxSlots];
  __shared__ int64_t s_best[kWaves][kMaxSlots];
  const int g = a.walk_group[blockIdx.x], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = a.n_slots;
  const int64_t N = a.n_nodes;
  const uint32_t mask = a.req_mask[g];
  const int32_t k0 = a.step_ptr[g], k1 = a.step_ptr[g + 1];
  int64_t best[kMaxSlots];
#pragma unroll
  for (int r = 0; r < kMaxSlots; ++r) best[r] = INT64_MIN;
  for (int32_t t0 = k0; t0 < k1; t0 += kStepTile) {
    const int nt = min(kStepTile, k1 - t0);
    __syncthreads();  // the previous tile is still being read
    for (int j = tid; j < nt; j += kBlock) s_node[j] = a.step_node[t0 + j];
    for (int j = tid; j < nt * S; j += kBlock) s_cum[j] = a.step_cum[static_cast<int64_t>(t0) * S + j];
    __syncthreads();
    // the nodes this tile decides: from its first step (the first tile: from node 0, before any step) up to the next tile's first step
    const int64_t lo = t0 == k0 ? 0 : s_node[0];
    const int64_t hi = t0 + nt < k1 ? a.step_node[t0 + nt] : N;
    for (int64_t i = lo + tid; i < hi; i += kBlock) {
      if (!a.node_present[i]) continue;
      int l = 0, h = nt;  // the steps at nodes <= i: s_node[0 .. l)
      while (l < h) {
        const int m = (l + h) >> 1;
        if (s_node[m] <= i) l = m + 1;
        else h = m;
      }
#pragma unroll
      for (int r = 0; r < kMaxSlots; ++r) {
        if (r < S && ((mask >> r) & 1u)) {
          const int64_t add = l > 0 ? s_cum[(l - 1) * S + r] : 0;
          best[r] = max64(best[r], a.prefix[static_cast<int64_t>(r) * N + i] + add);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kMaxSlots; ++r) {
    const int64_t m = wave_max(best[r]);
    if (lane == 0) s_best[wave][r] = m;
  }
  __syncthreads();
  if (tid == 0) {
    const bool any = *a.any_present != 0;
    int64_t last[kMaxSlots];
    for (int r = 0; r < S; ++r) {
      for (int w = 1; w < kWaves; ++w) s_best[0][r] = max64(s_best[0][r], s_best[w][r]);
      // every step sits on a present node, so the last present node has seen all of them
      last[r] = a.slot_total[r] + a.step_cum[static_cast<int64_t>(k1 - 1) * S + r];
    }
    write_verdict(a, g, mask, s_best[0], last, any);
  }
}

__global__ __launch_bounds__(kBlock) void k_cosched_status(CoschedArgs a) {
  const int64_t pod = a.row_begin + static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (pod >= a.row_end) return;
  const int g = a.pod_group[pod];
  uint8_t st = 0;
  if (g >= 0 && a.g_exists[g]) {  // no label, or no PodGroup object: Success (core.go:246-249)
    const int64_t quorum_gap = static_cast<int64_t>(a.min_member[g]) - a.listed[g];
    if (a.backed_off[g]) st = SPX_COSCHED_ST_BACKED_OFF;
    else if (quorum_gap > 0) st = SPX_COSCHED_ST_FEW_SIBLINGS;
    else if (quorum_gap + a.gated[g] > 0) st = SPX_COSCHED_ST_GATED;  // quorumGap only grows along the walk (core.go:270-277)
    else if (a.has_min_resources[g] && !a.permitted[g] && a.open_mask[g] != 0) st = SPX_COSCHED_ST_RESOURCE_GAP;
  }
  a.out_status[pod] = st;
}

__global__ __launch_bounds__(kBlock) void k_cosched_unschedulable(const uint8_t* status, int64_t row_begin, int64_t row_end, int64_t* best_score, int32_t* best_node,
                                                                  int32_t* best_ties, int32_t* best_feasible) {
  const int64_t pod = row_begin + static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (pod >= row_end || status[pod] == 0) return;
  best_node[pod] = -1;
  best_score[pod] = 0;
  best_ties[pod] = 0;
  best_feasible[pod] = 0;
}

inline unsigned blocks_for(int64_t n) { return static_cast<unsigned>((n + kBlock - 1) / kBlock); }

}  // namespace

void launch_cosched_gate(const CoschedArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_cosched_scan, dim3(static_cast<unsigned>(a.n_slots)), dim3(kBlock), 0, s, a);
  if (a.n_groups > 0) hipLaunchKernelGGL(k_cosched_gate_flat, dim3(blocks_for(a.n_groups)), dim3(kBlock), 0, s, a);
  if (a.n_walk > 0) hipLaunchKernelGGL(k_cosched_gate_walk, dim3(static_cast<unsigned>(a.n_walk)), dim3(kBlock), 0, s, a);
}

void launch_cosched_status(const CoschedArgs& a, hipStream_t s) {
  if (a.row_end > a.row_begin) hipLaunchKernelGGL(k_cosched_status, dim3(blocks_for(a.row_end - a.row_begin)), dim3(kBlock), 0, s, a);
}

void launch_cosched_unschedulable(const uint8_t* status, int64_t row_begin, int64_t row_end, int64_t* best_score, int32_t* best_node, int32_t* best_ties,
                                  int32_t* best_feasible, hipStream_t s) {
  if (row_end > row_begin)
    hipLaunchKernelGGL(k_cosched_unschedulable, dim3(blocks_for(row_end - row_begin)), dim3(kBlock), 0, s, status, row_begin, row_end, best_score, best_node,
                       best_ties, best_feasible);
}

}  // namespace spx
