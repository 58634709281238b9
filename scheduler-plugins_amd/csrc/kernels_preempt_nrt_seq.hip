// kernels_preempt_nrt_seq.hip — CapacityScheduling's sequential preemption loop with NodeResourceTopologyMatch's Filter in the refit
// (DESIGN.md 3.9j): kernels_preempt_seq.hip's step with nrt_refit.h's NrtRefit as the refit policy of cap_cell.h's walk.
//
// A step is the five launches of 3.9f on one stream, enqueued up front; the first two and the pick are that loop's own, as they are:
//
//   k_cap_seq_row      (kernels_preempt_seq.hip) PreFilter's sums and row i's record
//   k_cap_seq_marks    (kernels_preempt_seq.hip) the borrowed marks from the current Used; they depend on no Filter
//   k_cnrt_seq_cells   a wave per node: cell (i, node) with the overlay and the Filter, every lane the same cell, lane 0 stores.  One
//                      wave per workgroup, as k_cnrt_cells: the release sums are the launch's dynamic LDS (pnrt_lds_bytes), which four
//                      waves would need four times; the PDB budgets are the wave's 4 KiB
//   k_ptol_seq_pick    (kernels_ptol_seq.hip) the pick of column i
//   k_cnrt_seq_apply   one wave: cell (i, picked node) again for its victim set, then cap_cell.h's cap_seq_apply_tail: the set is stored,
//                      T4, T1 with the movement of Used and of the aggregate, T3 and T2, as k_cap_seq_apply
//
// The NRT row record is a function of the preemptors' uploaded columns alone: k_cnrt_rows (kernels_preempt_nrt.hip) writes it for every
// row before step 0.
//
// T5: the zone table, the placement info and the per-pod releases are read as uploaded at every step.  The reference's NRT caches have
// no pod-delete path (pkg/noderesourcetopology/cache/passthrough.go, discardreserved.go, overreserve.go change on an NRT update, a
// Reserve / Unreserve or a resync only), so between two PostFilter calls of a batch the table stays as reported.  A pod that left at an
// earlier step is gone from NodeInfo: nobody calls RemovePod for it again, so it is never on NRT's preemption stack again.  Here the walk
// skips the positions in `gone` before it moves a pod, so NrtRefit::moved never sees them: no release, no entry in the stack size or the
// contributing count.  NRT ignores nominated pods: T2 and T3 do not touch the Filter.  Nothing of NRT's is carried on the device.
//
// What this loop alone has: a victim the Filter kept, which NodeResourcesFit would have reprieved, leaves its quota through T1 like any
// other, and the moved Used flips borrowed marks and over-min branches on nodes no step touched.  Integer vector code only.
#include "cap_cell.h"
#include "nrt_refit.h"

namespace spx {

namespace {

__device__ __forceinline__ NrtRefit refit_of(const CnrtSeqArgs& p, int64_t* sum) {
  NrtRefit rf;
  rf.a = &p.n, rf.R = p.q.t.row_stride, rf.sum = sum;
  return rf;
}

__global__ __launch_bounds__(64) void k_cnrt_seq_cells(CnrtSeqArgs p) {
  extern __shared__ int64_t s_sum[];
  __shared__ int16_t s_budget[kPdbs][64];
  const CapSeqArgs& q = p.q;
  const PreemptArgs& a = q.t;
  const int64_t node = blockIdx.x;
  if (node >= a.n_nodes) return;  // before anything touches LDS
  const int lane = threadIdx.x;
  uint32_t vict[kWords];
  const PreemptCell out = cap_cell<true, NrtRefit>(a, &q, node, q.step, true, s_budget, lane, vict, refit_of(p, s_sum));  // every lane the same cell
  if (lane == 0) a.cells[node * a.row_stride + q.step] = out;
}

__global__ __launch_bounds__(64) void k_cnrt_seq_apply(CnrtSeqArgs p) {
  extern __shared__ int64_t s_sum[];
  __shared__ int16_t s_budget[kPdbs][64];
  const CapSeqArgs& q = p.q;
  const PreemptArgs& a = q.t;
  const int lane = threadIdx.x;
  const int64_t R = a.row_stride, i = q.step;
  const int32_t n = a.pick[i];
  const uint32_t flags = static_cast<uint32_t>(a.row_rec[kFlags * R + i]);
  const int prio = static_cast<int>(a.row_rec[kPrio * R + i]);

  // every lane computes the picked cell of row i
  uint32_t vict[kWords] = {};
  if (n >= 0) (void)cap_cell<true, NrtRefit>(a, &q, n, i, true, s_budget, lane, vict, refit_of(p, s_sum));
  cap_seq_apply_tail(q, n, i, flags, prio, vict, lane);
}

}  // namespace

// step p.q.step of the loop between its marks and its pick: the row's column
void launch_cnrt_seq_cells(const CnrtSeqArgs& p, hipStream_t s) {
  if (p.q.t.n_nodes > 0) hipLaunchKernelGGL(k_cnrt_seq_cells, dim3(static_cast<unsigned>(p.q.t.n_nodes)), dim3(64), pnrt_lds_bytes(p.n), s, p);
}

// after the pick: the victim set of the picked cell and what the row changes
void launch_cnrt_seq_apply(const CnrtSeqArgs& p, hipStream_t s) { hipLaunchKernelGGL(k_cnrt_seq_apply, dim3(1), dim3(64), pnrt_lds_bytes(p.n), s, p); }

}  // namespace spx
