// kernels_ptol_nrt.hip — PreemptionToleration's dry run with NodeResourceTopologyMatch's Filter in the refit.
//
//   k_pnrt_rows   a thread per preemptor: its NRT record (spx_nrt_pods_soa's columns) into a [field][row] record next to k_ptol_rows'
//   k_pnrt_cells  a wave per node, a lane per preemptor: the walk of ptol_cell.h with NrtRefit as its refit policy
//
// The Filter, the record's layout and k_pnrt_rows are nrt_refit.h's, shared with kernels_preempt_nrt.hip (CapacityScheduling's dry run).
#include "nrt_refit.h"
#include "ptol_cell.h"

namespace spx {

namespace {

template __global__ void k_pnrt_rows<PnrtArgs>(PnrtArgs);  // ahead of the cells kernel: this unit's code in the order it always had

// One wave per workgroup, so that the sums (dynamic LDS: a.n.max_zones * a.n.n_res entries of 64 int64) are the launch's to size.
__global__ __launch_bounds__(64) void k_pnrt_cells(PnrtArgs a) {
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
  const PreemptCell out = ptol_cell<false, NrtRefit>(a.t, nullptr, node, rr, active, true, s_budget, lane, vict, rf);
  if (!active) return;
  a.t.cells[static_cast<int64_t>(blockIdx.x) * R + r] = out;
  if (a.t.victims_out) {
#pragma unroll
    for (int i = 0; i < kWords; ++i) a.t.victims_out[i] = vict[i];
  }
}

}  // namespace

void launch_pnrt_rows(const PnrtArgs& a, hipStream_t s) { launch_nrt_rows(a, s); }

// nodes [a.t.node_begin, a.t.node_begin + n_nodes_launch) x all rows of the list, as launch_ptol_cells
void launch_pnrt_cells(const PnrtArgs& a, unsigned n_nodes_launch, hipStream_t s) {
  if (a.t.n_rows > 0 && n_nodes_launch > 0) hipLaunchKernelGGL(k_pnrt_cells, dim3(n_nodes_launch, blocks_for(a.t.n_rows, 64)), dim3(64), pnrt_lds_bytes(a.n), s, a);
}

}  // namespace spx
