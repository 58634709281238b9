// kernels_ptol_seq.hip — PreemptionToleration's sequential preemption loop on the overlay that preempt_device.h
// describes; beyond it this loop keeps only the ids of the nodes each step changed (dirty).
//
// Every step is three launches on one stream, enqueued up front; each reads what the one before it left in device memory:
//
//   k_ptol_seq_pick    one workgroup of 1024 threads over the N cells of column i (stride R) in pickOneNodeForPreemption's order, with
//                      the candidate and tie counts of k_preempt_pick; the step waits for it, so it is as wide as a workgroup gets.
//                      CapacityScheduling's loop (kernels_preempt_seq.hip) picks with it over the same 32-byte cells
//   k_ptol_seq_apply   one wave: cell (i, picked node) again for its victim set, which is stored (32 B per row); then T1-T4 and the
//                      ids of the nodes whose state moved (the picked node and the nodes a dropped nomination sat on; -1 = unused slot):
//                      ptol_cell.h's ptol_seq_apply_tail, which the loop with NRT's Filter (kernels_ptol_nrt_seq.hip) ends its step with too
//   k_ptol_seq_cells   dirty slots x ceil(rows / 256): the column of each dirty node for the rows after i, ptol_cell.h's walk with
//                      the overlay on.  Rows <= i store nothing, so the cells of row i stay what row i saw at its own step.
//
// A PreemptNever row keeps the cells of the untouched state (the full sweep of k_ptol_cells before step 0): no step stores to them, and
// its victim set is computed with the overlay switched off.
//
// The walk and the row record are ptol_cell.h's, shared with kernels_ptol.hip; NodeResourcesFit with default args, the bit-set helpers
// and the pick's accumulator are preempt_device.h's, shared with kernels_preempt.hip as well.  Integer vector code only; every sum is
// bounded by the upload's 2^62 check (the loop only ever moves requests between sums).
#include "ptol_cell.h"

namespace spx {

namespace {

// the working copy of Requested; the other parts of the overlay start as all zero / all -1 bytes (the host's two memsets)
__global__ __launch_bounds__(kBlock) void k_ptol_seq_init(PtolSeqArgs q) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= q.t.n_nodes * S) return;
  q.o.requested[t] = q.t.nodes[t / S].requested[t % S];
}

constexpr int kPickBlock = 1024;

__global__ __launch_bounds__(kPickBlock) void k_ptol_seq_pick(PickArgs p) {
  __shared__ PickAcc sh[kPickBlock];
  const int t = threadIdx.x;
  const int64_t R = p.row_stride, i = p.step;
  PickAcc acc = kNoPick;
  for (int64_t n = t; n < p.n_nodes; n += kPickBlock) acc.take(p.cells[n * R + i], n);
  sh[t] = acc;
  for (int w = kPickBlock / 2; w > 0; w >>= 1) {
    __syncthreads();
    if (t < w && sh[t + w].cand > 0) {
      acc.merge(sh[t + w]);
      sh[t] = acc;
    }
  }
  if (t == 0) acc.store(p.pick, R, i);
}

__global__ __launch_bounds__(64) void k_ptol_seq_apply(PtolSeqArgs q) {
  __shared__ int16_t s_budget[kPdbs][64];
  const PtolArgs& a = q.t;
  const int lane = threadIdx.x;
  const int64_t R = a.row_stride, i = q.o.step;
  const int32_t n = q.pick[i];
  const int64_t meta = a.row_rec[kMeta * R + i];

  // every lane computes the picked cell of row i
  uint32_t vict[kWords] = {};
  if (n >= 0) (void)ptol_cell<true>(a, &q, n, i, true, meta & kNever, s_budget, lane, vict);
  ptol_seq_apply_tail(q, n, i, meta, vict, lane);
}

__global__ __launch_bounds__(kBlock) void k_ptol_seq_cells(PtolSeqArgs q) {
  __shared__ int16_t s_budget[kWaves][kPdbs][64];
  const PtolArgs& a = q.t;
  const int64_t i = q.o.step, R = a.row_stride;
  const int64_t node = q.dirty[i * q.n_dirty + blockIdx.x];
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * kBlock;
  if (node < 0 || r0 + kBlock - 1 <= i) return;  // an unused slot, or a block whose rows have all had their turn
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t r = r0 + wave * 64 + lane;
  if (r - lane >= a.n_rows || r - lane + 63 <= i) return;  // the whole wave is past the row list, or before the rows still to come
  const bool active = r < a.n_rows && r > i;
  const int64_t rr = active ? r : a.n_rows - 1;  // an idle lane shadows the last row and stores nothing
  const bool want = active && !(a.row_rec[kMeta * R + rr] & kNever);  // a PreemptNever row keeps the cells of the untouched state
  uint32_t vict[kWords];
  const PreemptCell out = ptol_cell<true>(a, &q, node, rr, want, false, s_budget[wave], lane, vict);
  if (want) a.cells[node * R + r] = out;
}

}  // namespace

// the overlay of the untouched state
void launch_ptol_seq_init(const PtolSeqArgs& q, hipStream_t s) {
  hipLaunchKernelGGL(k_ptol_seq_init, dim3(blocks_for(q.t.n_nodes * S, kBlock)), dim3(kBlock), 0, s, q);
}

// the pick of column p.step
void launch_ptol_seq_pick(const PickArgs& p, hipStream_t s) { hipLaunchKernelGGL(k_ptol_seq_pick, dim3(1), dim3(kPickBlock), 0, s, p); }

// step q.o.step of the loop after its pick: what the row changes, and the cells of the rows after it on the nodes it changed
void launch_ptol_seq_step(const PtolSeqArgs& q, hipStream_t s) {
  hipLaunchKernelGGL(k_ptol_seq_apply, dim3(1), dim3(64), 0, s, q);
  if (q.o.step + 1 < q.t.n_rows) hipLaunchKernelGGL(k_ptol_seq_cells, dim3(q.n_dirty, blocks_for(q.t.n_rows, kBlock)), dim3(kBlock), 0, s, q);
}

}  // namespace spx
