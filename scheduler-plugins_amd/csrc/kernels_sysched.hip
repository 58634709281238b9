// kernels_sysched.hip — SySched (pkg/sysched/sysched.go) on gfx950.
//
// Reference: SySched.Score sysched.go:234-279 once per (pod, node) — with P = getSyscalls(pod), H = HostSyscalls[node] and Q_q =
// getSyscalls(q) for the pods q of HostToPods[node]:  len(P) == 0 -> math.MaxInt64 (:249-251, before the host lookup); no host entry
// -> 0 (:253-259); else |H \ P| + sum_q |(H u P) \ Q_q| (:261-271; calcScore is the set size, :217-231) — then NormalizeScore
// (:281-288), upstream's helper.DefaultNormalizeScore(100, reverse = true): max = largest score of the list, floored at 0;
// max == 0 -> every score 100; else 100 - 100 * s / max in int64 with truncating division.
//
// Closed form (syscall names interned to bit positions; k residents, a = sum_q |H \ Q_q|, c[b] = residents whose set holds b):
//   |(H u P) \ Q| = |H \ Q| + |(P \ H) \ Q|, and sum_q |(P \ H) \ Q_q| = sum over b in P \ H of (k - c[b]), so
//   score = popc(H & ~P) + a + k popc(P & ~H) - sum over b in P \ H of c[b].
// The last sum is non-zero only where a resident's set holds a name the cached host set lacks (a SeccompProfile changed after addPod
// cached H): such nodes carry their (b, c[b]) pairs, b outside H, in a CSR and are patched behind a per-node test.
//
//   k_sysched_raw    the raw scores of a chunk of distinct sets, int32 [sets in chunk][row_stride]: a lane per node with the node's
//                    words of H in registers, the set's words wave-uniform (scalar loads), and the set's maximum over all nodes
//   k_sysched_norm   no Filter in play: NormalizeScore of each distinct set's row, once, into the row of the first pod that has the
//                    set (launch_rows_expand copies it to the others)
//   k_sysched_rows   Filter plugins or a feasibility mask in play, or a row range: a workgroup per pod row — maximum over the pod's
//                    feasible nodes from the set's raw row (4 B x N, L2-resident), then one byte per cell; infeasible cells get 0
//
// The pod with the empty set: math.MaxInt64 on every node.  DefaultNormalizeScore then forms 100 * MaxInt64, which wraps to -100 in
// int64; -100 / MaxInt64 truncates to 0 and the score is 100 - 0: a row of 100.  No popcounts are spent on it.
#include "spx_internal.h"

namespace spx {
namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kSetsPerBlock = 8;  // sets a workgroup of k_sysched_raw walks with its nodes' words in registers

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m));
  return v;
}

// NormalizeScore of one score against the row maximum m > 0: 100 - floor(100 s / m), exactly.
// x = 100 s < 2^31 (s < SPX_SYSCHED_MAX_SCORE, checked at the upload) and 0 <= s <= m, so t = x / m lies in [0, 100].  float(x) and
// float(m) carry a relative error of 2^-24 each, the reciprocal and the product another 2^-24 each: the float32 product is within
// 100 * 4 * 2^-24 < 2^-17 of t, so its floor q is floor(t) - 1, floor(t) or floor(t) + 1.  The remainder x - q m, formed in 32-bit
// integers (|x - q m| < 2 m < 2^26: the wrapped difference is the true one), says which, and one step corrects it.
__device__ __forceinline__ uint32_t norm_cell(uint32_t s, uint32_t m, float rcp) {
  const uint32_t x = 100u * s;
  uint32_t q = static_cast<uint32_t>(static_cast<float>(x) * rcp);
  const int32_t rem = static_cast<int32_t>(x - q * m);
  if (rem < 0) --q;
  else if (rem >= static_cast<int32_t>(m)) ++q;
  return 100u - q;
}

// KW: the words kept in registers (n_words rounded up to 1, 2, 4, 8 or 16; the words past n_words are zero and cost nothing)
template <int KW>
__global__ __launch_bounds__(kBlock) void k_sysched_raw(SyschedArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const bool live = n < a.n_nodes;
  const int W = a.n_words;
  uint64_t h[KW];
#pragma unroll
  for (int w = 0; w < KW; ++w) h[w] = (live && w < W) ? a.host_bits[static_cast<int64_t>(w) * a.n_nodes + n] : 0;
  const bool here = live && a.present[n] != 0;
  const int32_t k = here ? a.n_resident[n] : 0;
  const int32_t base = here ? a.resident_missing[n] : 0;
  const int32_t st0 = here ? a.stale_ptr[n] : 0, st1 = here ? a.stale_ptr[n + 1] : 0;

  const int32_t s_first = a.set_begin + static_cast<int32_t>(blockIdx.y) * kSetsPerBlock;
  const int32_t s_last = min(s_first + kSetsPerBlock, a.set_end);
  for (int32_t s = s_first; s < s_last; ++s) {  // wave-uniform
    const bool empty = a.set_empty[s] != 0;
    if (empty && !a.out_raw64) continue;
    const uint64_t* __restrict__ p = a.set_bits + static_cast<int64_t>(s) * W;
    int32_t only_h = 0, only_p = 0;
#pragma unroll
    for (int w = 0; w < KW; ++w) {
      const uint64_t pw = w < W ? p[w] : 0;  // uniform address: a scalar load
      only_h += __popcll(h[w] & ~pw);
      only_p += __popcll(pw & ~h[w]);
    }
    int32_t score = here ? only_h + base + k * only_p : 0;
    for (int32_t i = st0; i < st1; ++i) {  // rare: a resident whose set is not inside H
      const int32_t b = a.stale_bit[i];
      if ((p[b >> 6] >> (b & 63)) & 1) score -= a.stale_count[i];
    }
    if (a.out_raw64) {
      if (live) a.out_raw64[n] = empty ? INT64_MAX : static_cast<int64_t>(score);
      continue;
    }
    if (live) a.raw[static_cast<int64_t>(s - a.set_begin) * a.row_stride + n] = score;
    const int32_t mx = wave_max(score);  // (lanes past n_nodes hold 0: the maximum's floor)
    if (lane == 0 && mx > 0) atomicMax(a.set_max + s, mx);
  }
}

__global__ __launch_bounds__(kBlock) void k_sysched_norm(SyschedArgs a) {
  const int32_t s = a.set_begin + static_cast<int32_t>(blockIdx.y);
  const int32_t at = a.set_first[s];
  if (at == a.set_first[s + 1]) return;  // no pod of the batch has this set
  const int64_t n0 = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * 4;
  if (n0 >= a.row_stride) return;
  const int64_t row = a.order[at];
  uint32_t word = 0;
  if (a.set_empty[s]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) word |= (n0 + j < a.n_nodes ? 100u : 0u) << (8 * j);
  } else {
    const uint32_t m = static_cast<uint32_t>(a.set_max[s]);
    const float rcp = 1.0f / static_cast<float>(m);
    const int4 r = *reinterpret_cast<const int4*>(a.raw + static_cast<int64_t>(s - a.set_begin) * a.row_stride + n0);
    const int32_t v[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t b = n0 + j >= a.n_nodes ? 0u : (m == 0 ? 100u : norm_cell(static_cast<uint32_t>(v[j]), m, rcp));
      word |= b << (8 * j);
    }
  }
  *reinterpret_cast<uint32_t*>(a.out_score + row * a.row_stride + n0) = word;
}

// feasibility of the four nodes from n0 on for `pod`: byte j non-zero = node n0 + j does not count
__device__ __forceinline__ uint32_t infeasible4(const SyschedArgs& a, int64_t pod, int64_t n0) {
  uint32_t bad = 0;
#pragma unroll
  for (int t = 0; t < 3; ++t)
    if (a.other_status[t]) bad |= *reinterpret_cast<const uint32_t*>(a.other_status[t] + pod * a.row_stride + n0);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (n0 + j >= a.n_nodes) bad |= 0xffu << (8 * j);
  return bad;
}

__global__ __launch_bounds__(kBlock) void k_sysched_rows(SyschedArgs a) {
  __shared__ int32_t part[kBlock / kWave];
  const int64_t pod = a.order[a.set_first[a.set_begin] + static_cast<int64_t>(blockIdx.x)];
  if (pod < a.row_begin || pod >= a.row_end) return;  // workgroup-uniform
  const int32_t s = a.pod_set[pod];
  const bool empty = a.set_empty[s] != 0;
  const int32_t* __restrict__ raw = a.raw + static_cast<int64_t>(s - a.set_begin) * a.row_stride;
  uint32_t m = 0;
  if (!empty) {
    int32_t mx = 0;  // the list's maximum, floored at 0
    for (int64_t n0 = static_cast<int64_t>(threadIdx.x) * 4; n0 < a.row_stride; n0 += kBlock * 4) {
      const uint32_t bad = infeasible4(a, pod, n0);
      const int4 r = *reinterpret_cast<const int4*>(raw + n0);
      const int32_t v[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (!((bad >> (8 * j)) & 0xffu)) mx = max(mx, v[j]);
    }
    mx = wave_max(mx);
    if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = mx;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) mx = max(mx, part[w]);
    m = static_cast<uint32_t>(mx);
  }
  const float rcp = m ? 1.0f / static_cast<float>(m) : 0.0f;
  for (int64_t n0 = static_cast<int64_t>(threadIdx.x) * 4; n0 < a.row_stride; n0 += kBlock * 4) {
    const uint32_t bad = infeasible4(a, pod, n0);
    int4 r = {0, 0, 0, 0};
    if (!empty) r = *reinterpret_cast<const int4*>(raw + n0);
    const int32_t v[4] = {r.x, r.y, r.z, r.w};
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t b = 0;
      if (!((bad >> (8 * j)) & 0xffu)) b = (empty || m == 0) ? 100u : norm_cell(static_cast<uint32_t>(v[j]), m, rcp);
      word |= b << (8 * j);
    }
    *reinterpret_cast<uint32_t*>(a.out_score + pod * a.row_stride + n0) = word;
  }
}

}  // namespace

void launch_sysched_raw(const SyschedArgs& a, hipStream_t s) {
  if (a.set_end <= a.set_begin || a.n_nodes <= 0) return;
  const dim3 grid(static_cast<unsigned>((a.n_nodes + kBlock - 1) / kBlock), static_cast<unsigned>((a.set_end - a.set_begin + kSetsPerBlock - 1) / kSetsPerBlock));
  const int W = a.n_words;
  if (W <= 1) hipLaunchKernelGGL(k_sysched_raw<1>, grid, dim3(kBlock), 0, s, a);
  else if (W <= 2) hipLaunchKernelGGL(k_sysched_raw<2>, grid, dim3(kBlock), 0, s, a);
  else if (W <= 4) hipLaunchKernelGGL(k_sysched_raw<4>, grid, dim3(kBlock), 0, s, a);
  else if (W <= 8) hipLaunchKernelGGL(k_sysched_raw<8>, grid, dim3(kBlock), 0, s, a);
  else hipLaunchKernelGGL(k_sysched_raw<16>, grid, dim3(kBlock), 0, s, a);
}

void launch_sysched_norm(const SyschedArgs& a, hipStream_t s) {
  if (a.set_end <= a.set_begin) return;
  const dim3 grid(static_cast<unsigned>((a.row_stride / 4 + kBlock - 1) / kBlock), static_cast<unsigned>(a.set_end - a.set_begin));
  hipLaunchKernelGGL(k_sysched_norm, grid, dim3(kBlock), 0, s, a);
}

void launch_sysched_rows(const SyschedArgs& a, int64_t n_listed, hipStream_t s) {
  if (n_listed <= 0) return;
  hipLaunchKernelGGL(k_sysched_rows, dim3(static_cast<unsigned>(n_listed)), dim3(kBlock), 0, s, a);
}

}  // namespace spx
