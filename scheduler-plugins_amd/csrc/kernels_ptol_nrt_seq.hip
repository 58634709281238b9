// kernels_ptol_nrt_seq.hip — PreemptionToleration's sequential preemption loop with NodeResourceTopologyMatch's Filter in the refit
// (DESIGN.md 3.9i): kernels_ptol_seq.hip's step with nrt_refit.h's NrtRefit as the refit policy of ptol_cell.h's walk.
//
// A step is the three launches of 3.9e on one stream, enqueued up front:
//
//   k_ptol_seq_pick    (kernels_ptol_seq.hip) the pick of column i
//   k_pnrt_seq_apply   one wave: cell (i, picked node) again with the overlay and the Filter for its victim set, then ptol_cell.h's
//                      ptol_seq_apply_tail: the set is stored, T4, T1, T3 + T2 and the step's dirty nodes, as k_ptol_seq_apply
//   k_pnrt_seq_cells   dirty slots x ceil(rows / 64): the column of each dirty node for the rows after i.  One wave per workgroup, as
//                      k_pnrt_cells: the release sums are the launch's dynamic LDS (pnrt_lds_bytes), which four waves would need four
//                      times.  Rows <= i and PreemptNever rows store nothing.
//
// T5: the zone table, the placement info and the per-pod releases are read as uploaded at every step.  The reference's NRT caches have
// no pod-delete path (pkg/noderesourcetopology/cache/passthrough.go, discardreserved.go, overreserve.go change on an NRT update, a
// Reserve / Unreserve or a resync only), so between two PostFilter calls of a batch the table stays as reported.  A pod that left at an
// earlier step is gone from NodeInfo: nobody calls RemovePod for it again, so it is never on NRT's preemption stack again.  Here the walk
// skips the positions in `gone` before it moves a pod, so NrtRefit::moved never sees them: no release, no entry in the stack size or the
// contributing count.  NRT ignores nominated pods: T2 and T3 do not touch the Filter.  Nothing of NRT's is carried on the device.
//
// A PreemptNever row keeps the cells of the untouched state (the full sweep of k_pnrt_cells before step 0), and its victim set is
// computed with the overlay switched off: what spx_preempt_toleration_nrt_dry_run gives for it.  Integer vector code only.
#include "nrt_refit.h"
#include "ptol_cell.h"

namespace spx {

namespace {

__device__ __forceinline__ NrtRefit refit_of(const PnrtSeqArgs& p, int64_t* sum) {
  NrtRefit rf;
  rf.a = &p.n, rf.R = p.q.t.row_stride, rf.sum = sum;
  return rf;
}

__global__ __launch_bounds__(64) void k_pnrt_seq_apply(PnrtSeqArgs p) {
  extern __shared__ int64_t s_sum[];
  __shared__ int16_t s_budget[kPdbs][64];
  const PtolSeqArgs& q = p.q;
  const PtolArgs& a = q.t;
  const int lane = threadIdx.x;
  const int64_t R = a.row_stride, i = q.o.step;
  const int32_t n = q.pick[i];
  const int64_t meta = a.row_rec[kMeta * R + i];

  // every lane computes the picked cell of row i
  uint32_t vict[kWords] = {};
  if (n >= 0) (void)ptol_cell<true, NrtRefit>(a, &q, n, i, true, meta & kNever, s_budget, lane, vict, refit_of(p, s_sum));
  ptol_seq_apply_tail(q, n, i, meta, vict, lane);
}

__global__ __launch_bounds__(64) void k_pnrt_seq_cells(PnrtSeqArgs p) {
  extern __shared__ int64_t s_sum[];
  __shared__ int16_t s_budget[kPdbs][64];
  const PtolSeqArgs& q = p.q;
  const PtolArgs& a = q.t;
  const int64_t i = q.o.step, R = a.row_stride;
  const int64_t node = q.dirty[i * q.n_dirty + blockIdx.x];
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * 64;
  if (node < 0 || r0 + 63 <= i) return;  // an unused slot, or a block whose rows have all had their turn: before anything touches LDS
  const int lane = threadIdx.x;
  const int64_t r = r0 + lane;
  const bool active = r < a.n_rows && r > i;
  const int64_t rr = active ? r : a.n_rows - 1;  // an idle lane shadows the last row and stores nothing
  const bool want = active && !(a.row_rec[kMeta * R + rr] & kNever);  // a PreemptNever row keeps the cells of the untouched state
  uint32_t vict[kWords];
  const PreemptCell out = ptol_cell<true, NrtRefit>(a, &q, node, rr, want, false, s_budget, lane, vict, refit_of(p, s_sum));
  if (want) a.cells[node * R + r] = out;
}

}  // namespace

// step p.q.o.step of the loop after its pick: what the row changes, and the cells of the rows after it on the nodes it changed
void launch_pnrt_seq_step(const PnrtSeqArgs& p, hipStream_t s) {
  const PtolSeqArgs& q = p.q;
  const size_t lds = pnrt_lds_bytes(p.n);
  hipLaunchKernelGGL(k_pnrt_seq_apply, dim3(1), dim3(64), lds, s, p);
  if (q.o.step + 1 < q.t.n_rows) hipLaunchKernelGGL(k_pnrt_seq_cells, dim3(q.n_dirty, blocks_for(q.t.n_rows, 64)), dim3(64), lds, s, p);
}

}  // namespace spx
