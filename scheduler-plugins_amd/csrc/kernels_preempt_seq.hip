// kernels_preempt_seq.hip — CapacityScheduling's sequential preemption loop: the rows of the list are attempted once
// each, in list order, and row i is evaluated against the state that rows 0..i-1 left.  A victim's removal moves its quota's Used, and
// with it the over-min branch of every later preemptor, the borrowed marks of that namespace on every node and the aggregate gate: every
// column is coupled to every other, so nothing is swept ahead.  At step i row i's record and its N cells are formed from the current
// state, picked over and applied; only row i writes its column, at its own step.  The overlay is the one preempt_device.h describes (CapSeqArgs carries its
// fields itself, spx_internal.h); next to it this loop keeps
//
//     used [ns][8], used_present [ns], agg_used [8], agg_used_present
//                           the working copies of every quota's Used and of the aggregate (T1, deletePodIfPresent)
//     marks [pod]           the working copy of the pods' marks (cap_cell.h), recomputed from the working Used
//
// Every step is five launches on one stream, enqueued up front; each reads what the one before it left in device memory:
//
//   k_cap_seq_row     one workgroup: PreFilter's two nominated sums (:226-265) over the live nominated entries of every present node —
//                     the uploaded records with their quota requests (spx_upload_preempt_nominated_quota) and the loop's own —, another
//                     quota's entries counting only while that quota is not usedOverMin() on the current Used; then row i's record
//   k_cap_seq_marks   a thread per node: the borrowed marks from the current Used.  Only a preemptor with a quota that is not over its
//                     min reads them (step b's third case), so for any other row the launch leaves at once; the marks are a function
//                     of the current state alone, so what a skipped step left stale the next reader's step recomputes in full
//   k_cap_seq_cells   a wave per node, four nodes per workgroup: cell (i, node), every lane the same cell, lane 0 stores
//   k_ptol_seq_pick   (kernels_ptol_seq.hip) one workgroup of 1024 threads over the N cells of column i
//   k_cap_seq_apply   one wave: cell (i, picked node) again for its victim set, which is stored (32 B per row); then T4, T1, T3, T2
//                     (what cap_cell.h's cap_seq_apply_tail says for the loop with NRT's Filter, kernels_preempt_nrt_seq.hip)
//
// The walk, the marks and the row record are cap_cell.h's, shared with kernels_preempt.hip.  Integer vector code only; every sum is
// bounded by the upload's 2^62 check (the loop only ever moves requests between sums), and the nominated sums wrap as int64, so any
// order of adding gives the same bits.
#include "cap_cell.h"

namespace spx {

namespace {

// the working copies of Requested, of every quota's Used and of the aggregate; the other parts of the overlay start as all zero / all
// -1 bytes (spx_preempt_sequential's memsets), the marks by k_cap_seq_marks with step -1
__global__ __launch_bounds__(kBlock) void k_cap_seq_init(CapSeqArgs q) {
  const PreemptArgs& a = q.t;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t < a.n_nodes * S) q.requested[t] = a.nodes[t / S].requested[t % S];
  if (t < static_cast<int64_t>(a.n_namespaces) * S) q.used[t] = a.used[t];
  if (t < a.n_namespaces) q.used_present[t] = a.used_present[t];
  if (t < S) q.agg_used[t] = a.agg_used[t];
  if (t == 0) *q.agg_used_present = a.agg_used_present;
}

__global__ __launch_bounds__(kBlock) void k_cap_seq_row(CapSeqArgs q) {
  __shared__ int64_t s_sum[2 * S][kBlock];
  __shared__ uint32_t s_p[2][kBlock];
  const PreemptArgs& a = q.t;
  const int t = threadIdx.x;
  const int64_t R = a.row_stride, i = q.step, pod = a.rows[i];
  const int ns = a.pod_ns[pod], prio = a.pod_priority[pod];
  const bool pq = ns >= 0 && ns < a.n_namespaces && a.has_quota[ns];
  int64_t in_eq[S], other[S];
  uint32_t in_p = 0, other_p = 0;
#pragma unroll
  for (int s = 0; s < S; ++s) in_eq[s] = other[s] = 0;
  if (pq) {
    // one live nominated pod of a quota'd namespace: same quota and at least as important (:254), or another quota that is not over
    // its min on the current Used (:258)
    auto entry = [&](int jns, int jprio, const int64_t* r, int64_t stride, uint32_t rp) {
      if (jns == ns) {
        if (jprio < prio) return;
#pragma unroll
        for (int s = 0; s < S; ++s) in_eq[s] = wadd(in_eq[s], r[s * stride]);
        in_p |= rp;
      } else {
        if (cmp2(q.used + static_cast<int64_t>(jns) * S, q.used_present[jns], nullptr, a.min + static_cast<int64_t>(jns) * S, a.min_present[jns], 0)) return;
#pragma unroll
        for (int s = 0; s < S; ++s) other[s] = wadd(other[s], r[s * stride]);
        other_p |= rp;
      }
    };
    for (int64_t n = t; n < a.n_nodes; n += kBlock) {
      const PreemptNode& nd = a.nodes[n];
      if (!nd.present) continue;
      for (int j = nd.nom_begin; j < nd.nom_end; ++j) {
        const int jns = q.nom_ns[j];
        if (q.nom_cleared[j] || a.noms[j].row == pod || jns < 0 || jns >= a.n_namespaces || !a.has_quota[jns]) continue;
        entry(jns, a.noms[j].prio, q.nom_qreq + static_cast<int64_t>(j) * S, 1, q.nom_qreq_present[j]);
      }
      for (int k = q.head[n]; k >= 0; k = q.row_next[k]) {  // the loop's own nominations: earlier rows, so never row i itself
        const uint32_t kf = static_cast<uint32_t>(a.row_rec[kFlags * R + k]);
        if (q.row_cleared[k] || !(kf & kHasQuota)) continue;
        entry(static_cast<int>(a.row_rec[kNs * R + k]), static_cast<int>(a.row_rec[kPrio * R + k]), a.row_rec + kReq * R + k, R, kf & 0xffu);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < S; ++s) s_sum[s][t] = in_eq[s], s_sum[S + s][t] = other[s];
  s_p[0][t] = in_p, s_p[1][t] = other_p;
  __syncthreads();
  if (t < 2 * S) {
    int64_t acc = 0;
    for (int u = 0; u < kBlock; ++u) acc = wadd(acc, s_sum[t][u]);
    s_sum[t][0] = acc;
  } else if (t < 2 * S + 2) {
    uint32_t acc = 0;
    for (int u = 0; u < kBlock; ++u) acc |= s_p[t - 2 * S][u];
    s_p[t - 2 * S][0] = acc;
  }
  __syncthreads();
  if (t != 0) return;
  const uint32_t req_p = a.pod_req_present[pod];
  in_p = req_p | s_p[0][0];
  const uint32_t total_p = in_p | s_p[1][0];
  uint32_t flags = (pq ? kHasQuota : 0u) | ((q.eligible && !q.eligible[i]) ? kHold : 0u);
  int64_t total[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int64_t req = a.pod_req[pod * S + s];
    in_eq[s] = wadd(req, s_sum[s][0]);
    total[s] = wadd(in_eq[s], s_sum[S + s][0]);
    a.row_rec[(kReq + s) * R + i] = req;
    a.row_rec[(kInEq + s) * R + i] = in_eq[s];
    a.row_rec[(kTotal + s) * R + i] = total[s];
    a.row_rec[(kFit + s) * R + i] = a.pre_fit[pod * S + s];
  }
  if (pq && cmp2(in_eq, in_p, q.used + static_cast<int64_t>(ns) * S, a.min + static_cast<int64_t>(ns) * S, a.min_present[ns], 0)) flags |= kMoreThanMin;
  flags |= (req_p & 0xffu) | ((in_p & 0xffu) << 8) | ((total_p & 0xffu) << 16);
  a.row_rec[kPrio * R + i] = prio;
  a.row_rec[kNs * R + i] = ns;
  a.row_rec[kFlags * R + i] = flags;
  a.row_rec[kRow * R + i] = pod;
}

// step < 0: every node, whatever row comes first (the init)
__global__ __launch_bounds__(kBlock) void k_cap_seq_marks(CapSeqArgs q) {
  const PreemptArgs& a = q.t;
  const int64_t node = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (node >= a.n_nodes) return;
  if (q.step >= 0) {
    const uint32_t flags = static_cast<uint32_t>(a.row_rec[kFlags * a.row_stride + q.step]);
    if (!(flags & kHasQuota) || (flags & kMoreThanMin)) return;  // step b's first two cases read the quota bit alone, which never moves
  }
  cap_marks<true>(a, &q, node);
}

__global__ __launch_bounds__(kBlock) void k_cap_seq_cells(CapSeqArgs q) {
  __shared__ int16_t s_budget[kWaves][kPdbs][64];
  const PreemptArgs& a = q.t;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t node = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  if (node >= a.n_nodes) return;
  uint32_t vict[kWords];
  const PreemptCell out = cap_cell<true>(a, &q, node, q.step, true, s_budget[wave], lane, vict);  // every lane the same cell
  if (lane == 0) a.cells[node * a.row_stride + q.step] = out;
}

__global__ __launch_bounds__(64) void k_cap_seq_apply(CapSeqArgs q) {
  __shared__ int16_t s_budget[kPdbs][64];
  const PreemptArgs& a = q.t;
  const int lane = threadIdx.x;
  const SeqOverlay o = q.overlay();
  const int64_t R = a.row_stride, i = o.step;
  const int32_t n = a.pick[i];
  const uint32_t flags = static_cast<uint32_t>(a.row_rec[kFlags * R + i]);
  const int prio = static_cast<int>(a.row_rec[kPrio * R + i]);

  // every lane computes the picked cell of row i
  uint32_t vict[kWords] = {};
  if (n >= 0) (void)cap_cell<true>(a, &q, n, i, true, s_budget, lane, vict);
  // The end of the step, written out here although cap_cell.h's cap_seq_apply_tail says the same: with the call in its place this kernel's
  // machine code moves (107 SGPR spills for 104), and the loop then timed outside the parent's own spread in one run of two
  seq_store_victims(o, i, vict, lane);
  if (flags & kHold) return;  // nothing moves
  // T4: the nominations row i came with are dropped wherever they sit
  for (int32_t t = o.row_nom_ptr[i] + lane; t < o.row_nom_ptr[i + 1]; t += 64) o.nom_cleared[o.row_nom[t]] = 1;
  if (n < 0) return;
  const PreemptNode& nd = a.nodes[n];
  const PreemptPod* pods = a.pods + nd.pod_begin;
  // T1: the victims leave the node, and deletePodIfPresent takes those that are in their quota's set out of its Used and of the
  // aggregate.  Lane s moves slot s, lane 0 the key masks: one wave, no two lanes on one word.
  seq_evict(o, n, vict, lane);
  if (lane < S) {
    int64_t sub = 0;
    for (int k = 0; k < nd.pod_end - nd.pod_begin; ++k) {
      if (!get_bit(vict, k)) continue;
      sub += pods[k].fit[lane];
      const uint8_t m = q.marks[nd.pod_begin + k];
      if ((m & (kMarkQuota | kMarkInSet)) != (kMarkQuota | kMarkInSet)) continue;
      const int64_t dq = pods[k].qreq[lane];
      q.used[static_cast<int64_t>(pods[k].ns) * S + lane] = wsub(q.used[static_cast<int64_t>(pods[k].ns) * S + lane], dq);
      q.agg_used[lane] = wsub(q.agg_used[lane], dq);
      if (lane == 0) q.used_present[pods[k].ns] |= pods[k].qreq_present, *q.agg_used_present |= pods[k].qreq_present;  // SetScalar
    }
    o.requested[static_cast<int64_t>(n) * S + lane] -= sub;
  }
  seq_nominate(o, nd, a.noms, n, i, prio, lane, a.row_rec + kPrio * R);  // T3, T2
}

}  // namespace

// the overlay of the untouched state
void launch_cap_seq_init(const CapSeqArgs& q, hipStream_t s) {
  const int64_t n = std::max<int64_t>(std::max<int64_t>(q.t.n_nodes, q.t.n_namespaces) * S, 1);
  hipLaunchKernelGGL(k_cap_seq_init, dim3(blocks_for(n, kBlock)), dim3(kBlock), 0, s, q);
  CapSeqArgs all = q;
  all.step = -1;
  hipLaunchKernelGGL(k_cap_seq_marks, dim3(blocks_for(q.t.n_nodes, kBlock)), dim3(kBlock), 0, s, all);
}

// the start of step q.step, which depends on no Filter: the row's record and the marks it reads.  The loop with NRT's Filter
// (kernels_preempt_nrt_seq.hip) starts its step with it too.
void launch_cap_seq_row(const CapSeqArgs& q, hipStream_t s) {
  hipLaunchKernelGGL(k_cap_seq_row, dim3(1), dim3(kBlock), 0, s, q);
  hipLaunchKernelGGL(k_cap_seq_marks, dim3(blocks_for(q.t.n_nodes, kBlock)), dim3(kBlock), 0, s, q);
}

// step q.step of the loop up to the pick: the row's record, the marks it reads, its column
void launch_cap_seq_step(const CapSeqArgs& q, hipStream_t s) {
  launch_cap_seq_row(q, s);
  hipLaunchKernelGGL(k_cap_seq_cells, dim3(blocks_for(q.t.n_nodes, kWaves)), dim3(kBlock), 0, s, q);
}

// after the pick: the victim set of the picked cell and what the row changes
void launch_cap_seq_apply(const CapSeqArgs& q, hipStream_t s) { hipLaunchKernelGGL(k_cap_seq_apply, dim3(1), dim3(64), 0, s, q); }

}  // namespace spx
