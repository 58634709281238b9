// kernels_ptol.hip — PreemptionToleration.PostFilter's preemption dry run: SelectVictimsOnNode (pkg/preemptiontoleration/
// preemption_toleration.go:188-299) for every (preemptor, node) cell.  The pick per preemptor is k_preempt_pick of
// kernels_preempt.hip on the cells written here.
//
//   k_ptol_rows   a thread per preemptor: its NodeResourcesFit vector, priority, PreemptNever and pod row into a [field][row] record
//   k_ptol_cells  a wave per node, a lane per preemptor, as k_preempt_cells: the walk of ptol_cell.h on the uploaded state.  There is
//                 no quota state.
//
// The walk and the row record are ptol_cell.h's, shared with kernels_ptol_seq.hip; the bit-set select chains, fits and in_vgpr are
// preempt_device.h's, shared with kernels_preempt.hip as well.
#include "ptol_cell.h"

namespace spx {

namespace {

__global__ __launch_bounds__(kBlock) void k_ptol_rows(PtolArgs a) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (r >= a.n_rows) return;
  const int64_t R = a.row_stride, pod = a.rows[r];
#pragma unroll
  for (int s = 0; s < S; ++s) a.row_rec[(kFit + s) * R + r] = a.pre_fit[pod * S + s];
  a.row_rec[kMeta * R + r] = a.row_meta[r];
  a.row_rec[kRow * R + r] = pod;
}

__global__ __launch_bounds__(kBlock) void k_ptol_cells(PtolArgs a) {
  __shared__ int16_t s_budget[kWaves][kPdbs][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t node = a.node_begin + blockIdx.x;
  const int64_t R = a.row_stride;
  const int64_t r = (static_cast<int64_t>(blockIdx.y) * kWaves + wave) * 64 + lane;
  if (r - lane >= a.n_rows) return;  // the whole wave is past the row list
  const bool active = r < a.n_rows;
  const int64_t rr = active ? r : a.n_rows - 1;  // an idle lane shadows the last row and stores nothing

  uint32_t vict[kWords];
  const PreemptCell out = ptol_cell<false>(a, nullptr, node, rr, active, true, s_budget[wave], lane, vict);
  if (!active) return;
  a.cells[static_cast<int64_t>(blockIdx.x) * R + r] = out;
  if (a.victims_out) {
#pragma unroll
    for (int i = 0; i < kWords; ++i) a.victims_out[i] = vict[i];
  }
}

}  // namespace

void launch_ptol_rows(const PtolArgs& a, hipStream_t s) {
  if (a.n_rows > 0) hipLaunchKernelGGL(k_ptol_rows, dim3(blocks_for(a.n_rows, kBlock)), dim3(kBlock), 0, s, a);
}

// nodes [a.node_begin, a.node_begin + n_nodes_launch) x all rows of the list; cells land at a.cells[(node - node_begin)][row]
void launch_ptol_cells(const PtolArgs& a, unsigned n_nodes_launch, hipStream_t s) {
  if (a.n_rows > 0 && n_nodes_launch > 0)
    hipLaunchKernelGGL(k_ptol_cells, dim3(n_nodes_launch, blocks_for(a.n_rows, kBlock)), dim3(kBlock), 0, s, a);
}

}  // namespace spx
