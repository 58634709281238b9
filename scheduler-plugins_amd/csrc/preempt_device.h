// preempt_device.h — the one copy of the device helpers that the preemption kernels share: kernels_preempt.hip (CapacityScheduling's
// dry run), kernels_ptol.hip (PreemptionToleration's) and kernels_ptol_seq.hip (its sequential loop).  The launch shape (a wave per
// node, a lane per preemptor, 256-bit sets over a node's pod list), the register helpers of the cell walks, NodeResourcesFit, and the
// key pickOneNodeForPreemption orders candidates by.  What is one plugin's stays with it: cmp2, the quota state and the capacity walk in
// cap_cell.h (kernels_preempt.hip and kernels_preempt_seq.hip), the toleration walk in ptol_cell.h.
//
// Everything is in the anonymous namespace: each translation unit gets its own copy.  NodeResourcesFit (default args) and
// pickOneNodeForPreemption restate upstream kube-scheduler code that is not in the reference tree.
#pragma once

#include "spx_internal.h"

namespace spx {

namespace {

constexpr int S = SPX_QUOTA_SLOTS;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kWords = SPX_PREEMPT_MAX_NODE_PODS / 32;
constexpr int kPdbs = SPX_PREEMPT_MAX_NODE_PDBS;

// A wave-uniform value the whole cell keeps reading (the node's Allocatable, the aggregate Min) would sit in scalar registers for the
// length of the kernel, next to the pod records the walk streams through them, and the allocator runs out of those first; a vector
// register per lane is what these kernels have to spare.
__device__ __forceinline__ int64_t in_vgpr(int64_t x) {
  asm volatile("" : "+v"(x));
  return x;
}

// bit k of a 256-bit set kept as eight registers; k is wave-uniform, so every index below is a compile-time one
__device__ __forceinline__ bool get_bit(const uint32_t* m, int k) {
  uint32_t w = 0;
#pragma unroll
  for (int i = 0; i < kWords; ++i) w = (k >> 5) == i ? m[i] : w;
  return (w >> (k & 31)) & 1u;
}
__device__ __forceinline__ void set_bit(uint32_t* m, int k, bool pred) {
#pragma unroll
  for (int i = 0; i < kWords; ++i) m[i] |= (pred && (k >> 5) == i) ? (1u << (k & 31)) : 0u;
}

// NodeResourcesFit.fitsRequest with default args on the lane's copy of the node (nominated pods already charged): the pod count, then per
// resource "insufficient iff req > 0 && req > allocatable - requested".  A pod whose requests are all zero fails none of those.
__device__ __forceinline__ bool fits(const int64_t* fit, const int64_t* alloc, const int64_t* requested) {
  bool ok = requested[3] + 1 <= alloc[3];
#pragma unroll
  for (int s = 0; s < S; ++s)
    if (s != 3) ok &= !(fit[s] > 0 && fit[s] > alloc[s] - requested[s]);
  return ok;
}

// a candidate's keys in the order pickOneNodeForPreemption compares them; smaller is better
struct PickKey {
  int32_t viol, hi, n_vict;
  int64_t sum, neg_start;
};
__device__ __forceinline__ int cmp_key(const PickKey& x, const PickKey& y) {
  if (x.viol != y.viol) return x.viol < y.viol ? -1 : 1;
  if (x.hi != y.hi) return x.hi < y.hi ? -1 : 1;
  if (x.sum != y.sum) return x.sum < y.sum ? -1 : 1;
  if (x.n_vict != y.n_vict) return x.n_vict < y.n_vict ? -1 : 1;
  if (x.neg_start != y.neg_start) return x.neg_start < y.neg_start ? -1 : 1;
  return 0;
}

inline unsigned blocks_for(int64_t n, int per) { return static_cast<unsigned>((n + per - 1) / per); }

}  // namespace

}  // namespace spx
