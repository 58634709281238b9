// kernels_ptol_seq.hip — PreemptionToleration's sequential preemption loop: the rows of the list are attempted once
// each, in list order, and row i is evaluated against the state that rows 0..i-1 left.  The uploaded records are never written; what
// the loop changes lives in an overlay next to them:
//
//     gone [node][8]        256-bit set: positions of the node's uploaded list that an earlier row evicted (T1)
//     requested [node][8]   the working copy of NodeInfo.Requested, less the evicted pods (T1)
//     nom_cleared [nom]     an uploaded nominated record is no longer charged (T3, T4)
//     head [node], row_next [row], row_cleared [row]
//                           the rows the loop nominated to the node (T2), newest first; the record of such a pod is the row's own
//                           [field][row] record, and row_cleared takes it out again (T3).  The charged sum does not depend on the order.
//
// Every step is three launches on one stream, enqueued up front; each reads what the one before it left in device memory:
//
//   k_ptol_seq_pick    one workgroup of 1024 threads over the N cells of column i (stride R) in pickOneNodeForPreemption's order, with
//                      the candidate and tie counts of k_preempt_pick; the step waits for it, so it is as wide as a workgroup gets
//   k_ptol_seq_apply   one wave: cell (i, picked node) again for its victim set, which is stored (32 B per row); then T1-T4 and the
//                      ids of the nodes whose state moved (the picked node and the nodes a dropped nomination sat on; -1 = unused slot)
//   k_ptol_seq_cells   dirty slots x ceil(rows / 256): the column of each dirty node for the rows after i, ptol_cell.h's walk with
//                      the overlay on.  Rows <= i store nothing, so the cells of row i stay what row i saw at its own step.
//
// A PreemptNever row keeps the cells of the untouched state (the full sweep of k_ptol_cells before step 0): no step stores to them, and
// its victim set is computed with the overlay switched off.
//
// The walk and the row record are ptol_cell.h's, shared with kernels_ptol.hip; NodeResourcesFit with default args, the bit-set helpers
// and the pick's key are preempt_device.h's, shared with kernels_preempt.hip as well.  Integer vector code only; every sum is bounded by
// the upload's 2^62 check (the loop only ever moves requests between sums).
#include "ptol_cell.h"

namespace spx {

namespace {

// the working copy of Requested; the other parts of the overlay start as all zero / all -1 bytes (launch_ptol_seq_init)
__global__ __launch_bounds__(kBlock) void k_ptol_seq_init(PtolSeqArgs q) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= q.t.n_nodes * S) return;
  q.requested[t] = q.t.nodes[t / S].requested[t % S];
}

constexpr int kPickBlock = 1024;

__global__ __launch_bounds__(kPickBlock) void k_ptol_seq_pick(PtolSeqArgs q) {
  __shared__ PickKey s_key[kPickBlock];
  __shared__ int32_t s_node[kPickBlock], s_cand[kPickBlock], s_ties[kPickBlock];
  const int t = threadIdx.x;
  const int64_t R = q.t.row_stride, i = q.step;
  PickKey best{0, 0, 0, 0, 0};
  int32_t node = -1, cand = 0, ties = 0;
  for (int64_t n = t; n < q.t.n_nodes; n += kPickBlock) {
    const PreemptCell c = q.t.cells[n * R + i];
    if (c.status != SPX_PREEMPT_ST_CANDIDATE) continue;
    const PickKey key{c.n_violations, c.hi_prio, c.n_victims, c.prio_sum, -c.start};
    const int o = cand ? cmp_key(key, best) : -1;
    ++cand;
    if (o < 0) best = key, node = static_cast<int32_t>(n), ties = 1;
    else if (o == 0) ++ties;  // nodes ascend within a thread: the first one stays
  }
  s_key[t] = best, s_node[t] = node, s_cand[t] = cand, s_ties[t] = ties;
  for (int w = kPickBlock / 2; w > 0; w >>= 1) {
    __syncthreads();
    if (t < w && s_cand[t + w] > 0) {
      const int o = cand ? cmp_key(s_key[t + w], best) : -1;
      cand += s_cand[t + w];
      if (o < 0) best = s_key[t + w], node = s_node[t + w], ties = s_ties[t + w];
      else if (o == 0) ties += s_ties[t + w], node = min(node, s_node[t + w]);  // the lowest node of the final tie set
      s_key[t] = best, s_node[t] = node, s_cand[t] = cand, s_ties[t] = ties;
    }
  }
  if (t != 0) return;
  q.pick[0 * R + i] = node;
  q.pick[1 * R + i] = node >= 0 ? best.n_vict : 0;
  q.pick[2 * R + i] = node >= 0 ? best.viol : 0;
  q.pick[3 * R + i] = cand;
  q.pick[4 * R + i] = ties;
}

__global__ __launch_bounds__(64) void k_ptol_seq_apply(PtolSeqArgs q) {
  __shared__ int16_t s_budget[kPdbs][64];
  const PtolArgs& a = q.t;
  const int lane = threadIdx.x;
  const int64_t R = a.row_stride, i = q.step;
  const int32_t n = q.pick[i];
  const int64_t meta = a.row_rec[kMeta * R + i];
  const int prio = prio_of(meta);
  const bool never = meta & kNever;
  int32_t* const dirty = q.dirty + i * q.n_dirty;

  // every lane computes the picked cell of row i; lane 0 keeps its victim set for spx_fetch_preempt_victims
  uint32_t vict[kWords];
#pragma unroll
  for (int w = 0; w < kWords; ++w) vict[w] = 0;
  if (n >= 0) (void)ptol_cell<true>(a, &q, n, i, true, never, s_budget, lane, vict);
  if (lane == 0) {
#pragma unroll
    for (int w = 0; w < kWords; ++w) q.victims[i * kWords + w] = vict[w];
  }
  if (meta & (kNever | kHold)) {  // nothing moves
    for (int k = lane; k < q.n_dirty; k += 64) dirty[k] = -1;
    return;
  }
  if (lane == 0) {
    // T4: the nominations row i came with are dropped wherever they sit; with T1-T3 below, these are the nodes whose cells are stale
    int n_dirty = 0;
    if (n >= 0) dirty[n_dirty++] = n;
    for (int32_t t = q.row_nom_ptr[i]; t < q.row_nom_ptr[i + 1]; ++t) {
      const int32_t j = q.row_nom[t], m = q.row_nom_node[t];
      if (q.nom_cleared[j]) continue;
      q.nom_cleared[j] = 1;
      bool listed = false;
      for (int k = 0; k < n_dirty; ++k) listed |= dirty[k] == m;
      if (!listed) dirty[n_dirty++] = m;
    }
    for (; n_dirty < q.n_dirty; ++n_dirty) dirty[n_dirty] = -1;
  }
  if (n < 0) return;
  const PreemptNode& nd = a.nodes[n];
  // T1: the victims leave the node
  if (lane == 0) {
#pragma unroll
    for (int w = 0; w < kWords; ++w) q.gone[static_cast<int64_t>(n) * kWords + w] |= vict[w];
  }
  if (lane < S) {
    const PreemptPod* pods = a.pods + nd.pod_begin;
    int64_t sub = 0;
    for (int k = 0; k < nd.pod_end - nd.pod_begin; ++k) sub += get_bit(vict, k) ? pods[k].fit[lane] : 0;
    q.requested[static_cast<int64_t>(n) * S + lane] -= sub;
  }
  // T3: nominated pods of the node with a lower priority lose their nomination, the uploaded ones and the loop's alike
  for (int j = nd.nom_begin + lane; j < nd.nom_end; j += 64)
    if (a.noms[j].prio < prio) q.nom_cleared[j] = 1;
  if (lane == 0) {
    for (int k = q.head[n]; k >= 0; k = q.row_next[k])
      if (prio_of(a.row_rec[kMeta * R + k]) < prio) q.row_cleared[k] = 1;
    // T2: row i is nominated to the node
    q.row_next[i] = q.head[n];
    q.head[n] = static_cast<int32_t>(i);
  }
}

__global__ __launch_bounds__(kBlock) void k_ptol_seq_cells(PtolSeqArgs q) {
  __shared__ int16_t s_budget[kWaves][kPdbs][64];
  const PtolArgs& a = q.t;
  const int64_t i = q.step, R = a.row_stride;
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

// step q.step of the loop: the pick of that row, what it changes, and the cells of the rows after it on the nodes it changed
void launch_ptol_seq_step(const PtolSeqArgs& q, hipStream_t s) {
  hipLaunchKernelGGL(k_ptol_seq_pick, dim3(1), dim3(kPickBlock), 0, s, q);
  hipLaunchKernelGGL(k_ptol_seq_apply, dim3(1), dim3(64), 0, s, q);
  if (q.step + 1 < q.t.n_rows) hipLaunchKernelGGL(k_ptol_seq_cells, dim3(q.n_dirty, blocks_for(q.t.n_rows, kBlock)), dim3(kBlock), 0, s, q);
}

// the pick of column q.step alone: CapacityScheduling's loop (kernels_preempt_seq.hip) picks over the same 32-byte cells
void launch_ptol_seq_pick(const PtolSeqArgs& q, hipStream_t s) { hipLaunchKernelGGL(k_ptol_seq_pick, dim3(1), dim3(kPickBlock), 0, s, q); }

}  // namespace spx
