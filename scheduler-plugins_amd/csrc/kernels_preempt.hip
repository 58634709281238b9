// kernels_preempt.hip — CapacityScheduling.PostFilter's preemption dry run: SelectVictimsOnNode (pkg/capacityscheduling/
// capacity_scheduling.go:486-677) for every (preemptor, node) cell, and pickOneNodeForPreemption per preemptor.
//
//   k_preempt_marks  a thread per node: which pods a preemptor of ANOTHER namespace removes when it borrows back (:572): a pod goes iff
//                    its quota is usedOverMin() when the walk reaches it, and that depends only on the removals of its own namespace's
//                    earlier pods, never on the preemptor — so it is marked once per snapshot
//   k_preempt_rows   a thread per preemptor: namespace, priority, podReq and PreFilter's two nominated sums (:226-265, as k_quota forms
//                    them), usedOverMinWith(nominatedPodsReqInEQWithPodReq) (:545), into a [field][row] record
//   k_preempt_cells  a wave per node, a lane per preemptor.  The node's pod list arrives through wave-uniform (scalar) loads and every
//                    lane walks the same trip count under its own predicate.  Per lane, in registers: the node's Requested, the
//                    preemptor quota's Used, the aggregate Used (8 int64 each) with their scalar-key masks, and three 256-bit sets
//                    (potential victims, PDB-violating, victims); the PDB budgets are 32 int16 per lane in LDS.
//   k_preempt_pick   64 preemptors x 4 node slices per workgroup: the lexicographic minimum of the candidate cells' keys
//
// The walk of a cell, the marks of a node, cmp2 and the row record's layout are cap_cell.h's, shared with kernels_preempt_seq.hip (the
// sequential loop); this unit runs them on the uploaded state.  The launch constants, in_vgpr, the bit-set select chains, fits and the
// pick's key are preempt_device.h's, shared with kernels_ptol.hip and kernels_ptol_seq.hip as well.  The nominated sums are restated
// from kernels_capacity.hip, whose machine code stays as it is.  Integer vector code only; every sum is bounded by the upload's 2^62 check.
#include "cap_cell.h"

namespace spx {

namespace {

__global__ __launch_bounds__(kBlock) void k_preempt_marks(PreemptArgs a) {
  const int64_t node = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (node >= a.n_nodes) return;
  cap_marks<false>(a, nullptr, node);
}

__global__ __launch_bounds__(kBlock) void k_preempt_rows(PreemptArgs a) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (r >= a.n_rows) return;
  const int64_t R = a.row_stride, pod = a.rows[r];
  const int ns = a.pod_ns[pod], prio = a.pod_priority[pod];
  int64_t req[S], in_eq[S], total[S];
  const uint32_t req_p = a.pod_req_present[pod];
  uint32_t in_p = req_p, total_p = req_p, flags = 0;
#pragma unroll
  for (int s = 0; s < S; ++s) req[s] = in_eq[s] = total[s] = a.pod_req[pod * S + s];
  if (ns >= 0 && ns < a.n_namespaces && a.has_quota[ns]) {
    flags |= kHasQuota;
    for (int j = a.q_nom_ptr[ns]; j < a.q_nom_ptr[ns + 1]; ++j) {  // same quota, at least as important as the preemptor (:254)
      if (a.q_nom_pending_index[j] == pod || a.q_nom_priority[j] < prio) continue;
#pragma unroll
      for (int s = 0; s < S; ++s) in_eq[s] = wadd(in_eq[s], a.q_nom_req[static_cast<int64_t>(j) * S + s]);
      in_p |= a.q_nom_req_present[j];
    }
#pragma unroll
    for (int s = 0; s < S; ++s) total[s] = wadd(in_eq[s], a.other_nominated[static_cast<int64_t>(ns) * S + s]);
    total_p = in_p | a.other_nominated_present[ns];
    if (cmp2(in_eq, in_p, a.used + static_cast<int64_t>(ns) * S, a.min + static_cast<int64_t>(ns) * S, a.min_present[ns], 0)) flags |= kMoreThanMin;
  }
  flags |= (req_p & 0xffu) | ((in_p & 0xffu) << 8) | ((total_p & 0xffu) << 16);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    a.row_rec[(kReq + s) * R + r] = req[s];
    a.row_rec[(kInEq + s) * R + r] = in_eq[s];
    a.row_rec[(kTotal + s) * R + r] = total[s];
    a.row_rec[(kFit + s) * R + r] = a.pre_fit[pod * S + s];
  }
  a.row_rec[kPrio * R + r] = prio;
  a.row_rec[kNs * R + r] = ns;
  a.row_rec[kFlags * R + r] = flags;
  a.row_rec[kRow * R + r] = pod;
}

__global__ __launch_bounds__(kBlock) void k_preempt_cells(PreemptArgs a) {
  __shared__ int16_t s_budget[kWaves][kPdbs][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t node = a.node_begin + blockIdx.x;
  const int64_t R = a.row_stride;
  const int64_t r = (static_cast<int64_t>(blockIdx.y) * kWaves + wave) * 64 + lane;
  if (r - lane >= a.n_rows) return;  // the whole wave is past the row list
  const bool active = r < a.n_rows;
  const int64_t rr = active ? r : a.n_rows - 1;  // an idle lane shadows the last row and stores nothing

  uint32_t vict[kWords];
  const PreemptCell out = cap_cell<false>(a, nullptr, node, rr, active, s_budget[wave], lane, vict);
  if (!active) return;
  a.cells[static_cast<int64_t>(blockIdx.x) * R + r] = out;
  if (a.victims_out) {
#pragma unroll
    for (int i = 0; i < kWords; ++i) a.victims_out[i] = vict[i];
  }
}

__global__ __launch_bounds__(kBlock) void k_preempt_pick(PickArgs p) {
  __shared__ PickAcc sh[kBlock];
  const int slice = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t R = p.row_stride, r = static_cast<int64_t>(blockIdx.x) * 64 + lane;  // r < R: the cells of the padding rows are never read below
  PickAcc acc = kNoPick;
  if (r < p.n_rows)
    for (int64_t n = slice; n < p.n_nodes; n += kWaves) acc.take(p.cells[n * R + r], n);
  sh[threadIdx.x] = acc;
  __syncthreads();
  if (slice != 0 || r >= p.n_rows) return;
  for (int w = 1; w < kWaves; ++w)
    if (sh[w * 64 + lane].cand) acc.merge(sh[w * 64 + lane]);
  acc.store(p.pick, R, r);
}

}  // namespace

void launch_preempt_marks(const PreemptArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_preempt_marks, dim3(blocks_for(a.n_nodes, kBlock)), dim3(kBlock), 0, s, a);
}

void launch_preempt_rows(const PreemptArgs& a, hipStream_t s) {
  if (a.n_rows > 0) hipLaunchKernelGGL(k_preempt_rows, dim3(blocks_for(a.n_rows, kBlock)), dim3(kBlock), 0, s, a);
}

// nodes [a.node_begin, a.node_begin + n_nodes_launch) x all rows of the list; cells land at a.cells[(node - node_begin)][row]
void launch_preempt_cells(const PreemptArgs& a, unsigned n_nodes_launch, hipStream_t s) {
  if (a.n_rows > 0 && n_nodes_launch > 0)
    hipLaunchKernelGGL(k_preempt_cells, dim3(n_nodes_launch, blocks_for(a.n_rows, kBlock)), dim3(kBlock), 0, s, a);
}

void launch_preempt_pick(const PickArgs& p, hipStream_t s) {
  if (p.n_rows > 0) hipLaunchKernelGGL(k_preempt_pick, dim3(blocks_for(p.n_rows, 64)), dim3(kBlock), 0, s, p);
}

}  // namespace spx
