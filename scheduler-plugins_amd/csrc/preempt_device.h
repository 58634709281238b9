// preempt_device.h — the one copy of the device helpers that the preemption kernels share: kernels_preempt.hip (CapacityScheduling's
// dry run), kernels_ptol.hip (PreemptionToleration's), each one's variant with NRT's Filter and the two sequential loops.  The launch shape (a wave per node, a lane per
// preemptor, 256-bit sets over a node's pod list), the register helpers of the cell walks, NodeResourcesFit, the accumulator both
// pick kernels fold cells into, and the overlay of the two loops with the code that moves it.  What is one plugin's stays with it: cmp2,
// the quota state and the capacity walk in cap_cell.h (kernels_preempt.hip and kernels_preempt_seq.hip), the toleration walk in ptol_cell.h.
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

// The refit of a cell walk (RunFilterPluginsWithNominatedPods) is NodeResourcesFit and whatever its Refit policy adds to it.  What a walk
// (ptol_cell.h, cap_cell.h) asks of the policy, in walk order: begin() once per cell, by the whole wave; moved() whenever the pod at index
// j of the pod records leaves (add false) or rejoins (add true) the copy of the node of the lanes with pred set, by the whole wave; ok()
// wherever the refit is asked, by the lanes that ask, so it holds no cross-lane operation.  FitOnly adds nothing and compiles to nothing;
// nrt_refit.h's NrtRefit is NodeResourceTopologyMatch's Filter, which sees the pods removed so far.
struct FitOnly {
  __device__ __forceinline__ void begin(int64_t, int64_t, int) {}
  __device__ __forceinline__ void moved(int, bool, bool) {}
  __device__ __forceinline__ bool ok() { return true; }
};

// pickOneNodeForPreemption over a set of cells of one row: the best candidate's keys, the lowest node that has them, and the candidate
// and tie counts.  40 bytes without padding: the pick kernels merge their threads' sets through an array of these in LDS.
struct PickAcc {
  int64_t sum, neg_start;
  int32_t viol, hi, n_vict, node, cand, ties;
  // the keys in the order pickOneNodeForPreemption compares them; smaller is better
  __device__ __forceinline__ int cmp(const PickAcc& y) const {
    if (viol != y.viol) return viol < y.viol ? -1 : 1;
    if (hi != y.hi) return hi < y.hi ? -1 : 1;
    if (sum != y.sum) return sum < y.sum ? -1 : 1;
    if (n_vict != y.n_vict) return n_vict < y.n_vict ? -1 : 1;
    if (neg_start != y.neg_start) return neg_start < y.neg_start ? -1 : 1;
    return 0;
  }
  // one cell; a thread takes its nodes in ascending order, so of equal keys the first one stays
  __device__ __forceinline__ void take(const PreemptCell& c, int64_t n) {
    if (c.status != SPX_PREEMPT_ST_CANDIDATE) return;
    merge(PickAcc{c.prio_sum, -c.start, c.n_violations, c.hi_prio, c.n_victims, static_cast<int32_t>(n), 1, 1});
  }
  // another set, which is not empty (x.cand > 0): of equal keys the lowest node of the final tie set
  __device__ __forceinline__ void merge(const PickAcc& x) {
    const int o = cand ? x.cmp(*this) : -1;
    const int32_t all = cand + x.cand, tied = ties + x.ties, low = min(node, x.node);
    if (o < 0) *this = x;
    else if (o == 0) ties = tied, node = low;
    cand = all;
  }
  __device__ __forceinline__ void store(int32_t* pick, int64_t R, int64_t i) const {
    pick[0 * R + i] = node, pick[1 * R + i] = node >= 0 ? n_vict : 0, pick[2 * R + i] = node >= 0 ? viol : 0;
    pick[3 * R + i] = cand, pick[4 * R + i] = ties;
  }
};
static_assert(sizeof(PickAcc) == 40, "LDS per thread of the pick kernels");
constexpr PickAcc kNoPick{0, 0, 0, 0, 0, -1, 0, 0};  // the empty set

inline unsigned blocks_for(int64_t n, int per) { return static_cast<unsigned>((n + per - 1) / per); }

// ---------------------------------------------------------------- what the two sequential preemption loops share
// kernels_ptol_seq.hip (PreemptionToleration) and kernels_preempt_seq.hip (CapacityScheduling, 3.9f), and the walks
// they run (ptol_cell.h, cap_cell.h).  The rows of the list are attempted once each, in list order, and row i is evaluated against the
// state that rows 0..i-1 left.  The uploaded records are never written; what a loop changes lives in an overlay next to them
// (SeqOverlay, spx_internal.h):
//
//     gone [node][8]        256-bit set: positions of the node's uploaded list that an earlier row evicted (T1)
//     requested [node][8]   the working copy of NodeInfo.Requested, less the evicted pods (T1)
//     nom_cleared [nom]     an uploaded nominated record is no longer charged (T3, T4)
//     head [node], row_next [row], row_cleared [row]
//                           the rows the loop nominated to the node (T2), newest first; the record of such a pod is the row's own
//                           [field][row] record, and row_cleared takes it out again (T3).  The charged sums do not depend on the order.
//     victims [row][8]      the victim set of each row's picked cell, for spx_fetch_preempt_victims
//
// An apply kernel is one wave; seq_store_victims, seq_evict and seq_nominate are called by all of its lanes.
// position k of the node's uploaded list left with an earlier row.  Wave-uniform in the walks: the skips are branches of the wave.
__device__ __forceinline__ bool seq_left(const uint32_t* gone, int64_t node, int k) { return (gone[node * kWords + (k >> 5)] >> (k & 31)) & 1u; }

// lane 0 keeps the victim set of row i's picked cell
__device__ __forceinline__ void seq_store_victims(const SeqOverlay& o, int64_t i, const uint32_t* vict, int lane) {
  if (lane != 0) return;
#pragma unroll
  for (int w = 0; w < kWords; ++w) o.victims[i * kWords + w] = vict[w];
}

// T1, the part every loop has: the victims leave node n
__device__ __forceinline__ void seq_evict(const SeqOverlay& o, int64_t n, const uint32_t* vict, int lane) {
  if (lane != 0) return;
#pragma unroll
  for (int w = 0; w < kWords; ++w) o.gone[n * kWords + w] |= vict[w];
}

// T3: nominated pods of node n with a lower priority than row i's lose their nomination, the uploaded ones and the loop's alike;
// then T2: row i is nominated to the node.  row_prio: the column of the unit's row record whose low 32 bits are a row's priority.
__device__ __forceinline__ void seq_nominate(const SeqOverlay& o, const PreemptNode& nd, const PreemptNom* noms, int32_t n, int64_t i, int prio, int lane, const int64_t* row_prio) {
  for (int j = nd.nom_begin + lane; j < nd.nom_end; j += 64)
    if (noms[j].prio < prio) o.nom_cleared[j] = 1;
  if (lane != 0) return;
  for (int k = o.head[n]; k >= 0; k = o.row_next[k])
    if (static_cast<int>(row_prio[k]) < prio) o.row_cleared[k] = 1;
  o.row_next[i] = o.head[n];
  o.head[n] = static_cast<int32_t>(i);
}

}  // namespace

}  // namespace spx
