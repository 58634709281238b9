// kernels_preempt_nrt.hip — CapacityScheduling's preemption dry run with NodeResourceTopologyMatch's Filter in the refit (DESIGN.md
// 3.9h).  SelectVictimsOnNode's removePod (:513) and addPod (:523) run the PreFilter extensions that push and pop NRT's preemption stack,
// and both Filter runs (:607 after the potential victims are gone, :636 inside reprievePod) run NRT's Filter on it.
//
//   k_cnrt_rows   a thread per preemptor: its NRT record next to k_preempt_rows' (nrt_refit.h's k_pnrt_rows on this plugin's arguments)
//   k_cnrt_cells  a wave per node, a lane per preemptor: the walk of cap_cell.h with NrtRefit as its refit policy
//
// The row record (k_preempt_rows), the borrowed marks (k_preempt_marks) and the pick (k_preempt_pick) are kernels_preempt.hip's, as they
// are: none of them depends on a Filter.  The Filter is nrt_refit.h's, shared with kernels_ptol_nrt.hip; its per-lane release sums live
// in dynamic LDS, so a workgroup is one wave here (k_preempt_cells has four) and the PDB budgets are that wave's alone.
#include "cap_cell.h"
#include "nrt_refit.h"

namespace spx {

namespace {

// One wave per workgroup, so that the sums (dynamic LDS: a.n.max_zones * a.n.n_res entries of 64 int64) are the launch's to size.
__global__ __launch_bounds__(64) void k_cnrt_cells(CnrtArgs a) {
  extern __shared__ int64_t s_sum[];
  __shared__ int16_t s_budget[kPdbs][64];
  const int lane = threadIdx.x;
  const int64_t node = a.t.node_begin + blockIdx.x;
  const int64_t R = a.t.row_stride;
  const int64_t r = static_cast<int64_t>(blockIdx.y) * 64 + lane;
  const bool active = r < a.t.n_rows;
  const int64_t rr = active ? r : a.t.n_rows - 1;  // an idle lane shadows the last row and stores nothing

  uint32_t vict[kWords];
  NrtRefit rf;
  rf.a = &a.n, rf.R = R, rf.sum = s_sum;
  const PreemptCell out = cap_cell<false, NrtRefit>(a.t, nullptr, node, rr, active, s_budget, lane, vict, rf);
  if (!active) return;
  a.t.cells[static_cast<int64_t>(blockIdx.x) * R + r] = out;
  if (a.t.victims_out) {
#pragma unroll
    for (int i = 0; i < kWords; ++i) a.t.victims_out[i] = vict[i];
  }
}

}  // namespace

void launch_cnrt_rows(const CnrtArgs& a, hipStream_t s) { launch_nrt_rows(a, s); }

// nodes [a.t.node_begin, a.t.node_begin + n_nodes_launch) x all rows of the list, as launch_preempt_cells; with n_rows == 1 and
// a.t.victims_out set it is the one cell of the victims fetch
void launch_cnrt_cells(const CnrtArgs& a, unsigned n_nodes_launch, hipStream_t s) {
  if (a.t.n_rows > 0 && n_nodes_launch > 0) hipLaunchKernelGGL(k_cnrt_cells, dim3(n_nodes_launch, blocks_for(a.t.n_rows, 64)), dim3(64), pnrt_lds_bytes(a.n), s, a);
}

}  // namespace spx
