// ptol_cell.h — PreemptionToleration's SelectVictimsOnNode (pkg/preemptiontoleration/preemption_toleration.go:188-299) for one
// (preemptor, node) cell per lane, and the row record it reads: the one copy of the walk that kernels_ptol.hip (k_ptol_cells, on the
// uploaded state) and kernels_ptol_seq.hip (k_ptol_seq_apply and k_ptol_seq_cells, on the state the loop's earlier rows left) run, and
// with nrt_refit.h's Filter in the refit kernels_ptol_nrt.hip and kernels_ptol_nrt_seq.hip; and the end of a loop's step, which the two
// apply kernels share (ptol_seq_apply_tail).
//
// The walk is DefaultPreemption's with one more predicate per (preemptor, lower-priority pod) pair, ExemptedFromPreemption (:129-181).
// What of it depends on the pod alone is folded into the PtolPod record by the host (flatten_ptol.cc): the class lookup, the parsed
// policy, and scheduledAt + TolerationSeconds as one instant.  What is left per pair is
//     exempted = has_class && (never || (prio < min_prio && until > now))
// and a missing class among the lower-priority pods is the node's error.
//
// The node's pod list arrives through wave-uniform (scalar) loads and every lane walks the same trip count under its own predicate.
// Per lane, in registers: the node's Requested (8 int64) and three 256-bit sets (potential victims, PDB-violating, victims); the PDB
// budgets are 32 int16 per lane in LDS.  Integer vector code only; every sum is bounded by the upload's 2^62 check.
//
// The refit (RunFilterPluginsWithNominatedPods, :250 and :268) is NodeResourcesFit and whatever the Refit policy adds to it
// (preempt_device.h states the three calls): FitOnly nothing, nrt_refit.h's NrtRefit NodeResourceTopologyMatch's Filter, which sees the
// pods removed so far.
#pragma once

#include "preempt_device.h"

namespace spx {

namespace {

// fields of the row record (k_ptol_rows writes it)
constexpr int kFit = 0, kMeta = 8, kRow = 9;
static_assert(kRow + 1 == kPtolRowFields, "row record layout");
constexpr int64_t kNever = int64_t{1} << 32;  // kMeta: the priority in the low 32 bits, PreemptNever above them,
constexpr int64_t kHold = int64_t{1} << 33;   // and "not eligible" (the sequential loop: evaluated at its step, nothing applied)

__device__ __forceinline__ int prio_of(int64_t meta) { return static_cast<int>(static_cast<uint32_t>(meta)); }

// One cell per lane: row rr of the list on `node`, for the lanes with want set.  budget: the wave's [kPdbs][64] int16 in LDS.  vict
// is all zero unless the cell is a CANDIDATE.
// kOverlay off: the uploaded state; q (NULL) and frozen are not read.
// kOverlay on: the sequential loop's state (kernels_ptol_seq.hip) from q->o: Requested is the working copy, cleared nominations are not
// charged, the loop's own nominations are, and the positions in `gone` are skipped in every pass.  frozen (wave-uniform) switches all
// of that off at run time: the untouched state, which a PreemptNever row sees.  A skipped position never reaches move_pod, so the
// refit policy never hears of a pod that left at an earlier step.
template <bool kOverlay, class Refit = FitOnly>
__device__ __forceinline__ PreemptCell ptol_cell(const PtolArgs& a, const PtolSeqArgs* q, int64_t node, int64_t rr, bool want, bool frozen, int16_t (*budget)[64], int lane,
                                                 uint32_t* vict, Refit rf = Refit{}) {
  const int64_t R = a.row_stride;
  int64_t fit[S];
#pragma unroll
  for (int s = 0; s < S; ++s) fit[s] = a.row_rec[(kFit + s) * R + rr];
  const int64_t meta = a.row_rec[kMeta * R + rr];
  const int prio = prio_of(meta);
  const bool never = meta & kNever;
  const int64_t pod_row = a.row_rec[kRow * R + rr];
  const int64_t now = a.now;

  PreemptCell out{0, 0, 0, 0, 0, SPX_PREEMPT_ST_SKIPPED};
#pragma unroll
  for (int i = 0; i < kWords; ++i) vict[i] = 0;
  const PreemptNode& nd = a.nodes[node];
  const PreemptPod* pods = a.pods + nd.pod_begin;  // position in the node's list -> record
  const PtolPod* tol = a.tol + nd.pod_begin;
  const bool overlay = kOverlay && !frozen;  // false at compile time with the switch off: nothing below reads q then
  auto left = [&](int k) { return overlay && seq_left(q->o.gone, node, k); };
  bool live = want && nd.present && (!a.node_mask || a.node_mask[rr * a.n_nodes + node]);

  if (__any(live)) {
    const int L = nd.pod_end - nd.pod_begin;
    rf.begin(node, rr, lane);
    // the lane's copy of the node, the nominated pods that outrank the preemptor charged once: they are re-added before every Filter run
    int64_t alloc[S], requested[S];
#pragma unroll
    for (int s = 0; s < S; ++s) alloc[s] = in_vgpr(nd.alloc[s]), requested[s] = overlay ? q->o.requested[node * S + s] : nd.requested[s];
    for (int j = nd.nom_begin; j < nd.nom_end; ++j) {
      if (overlay && q->o.nom_cleared[j]) continue;
      const bool add = a.noms[j].prio >= prio && a.noms[j].row != pod_row;
#pragma unroll
      for (int s = 0; s < S; ++s) requested[s] += add ? a.noms[j].fit[s] : 0;
    }
    if (overlay) {
      for (int k = q->o.head[node]; k >= 0; k = q->o.row_next[k]) {  // the loop's own nominations: earlier rows, so never the lane's own
        if (q->o.row_cleared[k]) continue;
        const bool add = prio_of(a.row_rec[kMeta * R + k]) >= prio;
#pragma unroll
        for (int s = 0; s < S; ++s) requested[s] += add ? (s == 3 ? 1 : a.row_rec[(kFit + s) * R + k]) : 0;  // a pod counts once
      }
    }
    // NodeInfo.RemovePod / AddPod of the pod at position k on the lane's copy
    auto move_pod = [&](int k, bool pred, bool add) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int64_t f = pods[k].fit[s];
        requested[s] += pred ? (add ? f : -f) : 0;
      }
      rf.moved(nd.pod_begin + k, pred, add);
    };

    // step 1 (:218-236): every lower-priority pod still on the node that is not exempted is a potential victim and is removed
    uint32_t pot[kWords], viol[kWords];
#pragma unroll
    for (int i = 0; i < kWords; ++i) pot[i] = viol[i] = 0;
    int n_pot = 0;
    bool class_error = false;
    for (int k = 0; k < L; ++k) {
      if (left(k)) continue;
      const int jprio = pods[k].prio;
      const PtolPod t = tol[k];
      const bool lower = live && jprio < prio;
      const bool exempted = (t.flags & SPX_PTOL_POD_HAS_CLASS) && (never || (prio < t.min_prio && t.until > now));
      class_error |= lower && (t.flags & SPX_PTOL_POD_CLASS_MISSING);
      const bool pv = lower && !exempted;
      if (!__any(pv)) continue;
      set_bit(pot, k, pv);
      n_pot += pv;
      move_pod(k, pv, false);
    }
    // steps 2, 3 (:239-252), after the error of the class lookup (:225-228)
    if (live) {
      if (class_error) out.status = SPX_PREEMPT_ST_CLASS_ERROR, live = false;
      else if (n_pot == 0) out.status = SPX_PREEMPT_ST_NO_VICTIMS, live = false;
      else if (!fits(fit, alloc, requested) || !rf.ok()) out.status = SPX_PREEMPT_ST_NOT_FIT, live = false;
    }
    if (__any(live)) {
      // step 4: filterPodsWithPDBViolation over the potential victims, most important first; the budgets are the uploaded ones, in the
      // sequential loop at every step
      const int b0 = nd.pdb_begin, n_pdb = nd.pdb_end - b0;
      if (n_pdb > 0) {
        for (int i = 0; i < n_pdb; ++i) budget[i][lane] = static_cast<int16_t>(max(-1, min(32767, a.pdb_allowed[b0 + i])));  // 256 decrements at most
        for (int k = 0; k < L; ++k) {
          const int pos = pods[k].hi_order;
          uint32_t bits = pods[pos].pdb_mask;
          if (!bits || left(pos)) continue;
          const bool pv = live && get_bit(pot, pos);
          bool hit = false;
          while (bits) {
            const int i = __builtin_ctz(bits);
            bits &= bits - 1;
            if (pv) {
              const int16_t rest = budget[i][lane] - 1;
              budget[i][lane] = rest;
              hit |= rest < 0;
            }
          }
          set_bit(viol, pos, hit);
        }
      }
      // step 5: reprieve, the violating pods first, each list most important first
      int n_vict = 0, n_viol = 0, hi = INT32_MIN;
      int64_t sum = 0, start = INT64_MAX;
      for (int pass = n_pdb > 0 ? 0 : 1; pass < 2; ++pass) {
        for (int k = 0; k < L; ++k) {
          const int pos = pods[k].hi_order;
          if (left(pos)) continue;
          const bool pv = live && get_bit(pot, pos) && (get_bit(viol, pos) == (pass == 0));
          if (!__any(pv)) continue;
          move_pod(pos, pv, true);
          const bool victim = pv && !(fits(fit, alloc, requested) && rf.ok());
          move_pod(pos, victim, false);
          set_bit(vict, pos, victim);
          if (victim) {
            const int jprio = pods[pos].prio;
            const int64_t jstart = pods[pos].start;
            ++n_vict;
            n_viol += pass == 0;
            sum += static_cast<int64_t>(jprio) + (int64_t{1} << 31);
            start = jprio > hi ? jstart : (jprio == hi && jstart < start) ? jstart : start;
            hi = jprio > hi ? jprio : hi;
          }
        }
      }
      if (live) {
        if (n_vict == 0) out.status = SPX_PREEMPT_ST_ALL_REPRIEVED;
        else out = PreemptCell{sum, start, hi, n_vict, n_viol, SPX_PREEMPT_ST_CANDIDATE};
      }
    }
  }
  if (out.status != SPX_PREEMPT_ST_CANDIDATE) {
#pragma unroll
    for (int i = 0; i < kWords; ++i) vict[i] = 0;
  }
  return out;
}

// The end of step i in the apply kernel of a PreemptionToleration loop (k_ptol_seq_apply, k_pnrt_seq_apply), called by all lanes of its
// one wave once the picked cell (i, n) is computed again: the victim set is stored (32 B per row); then T4, T1, T3 + T2 and the ids of
// the nodes whose state moved (the picked node and the nodes a dropped nomination sat on; -1 = unused slot).  n: the pick, -1 = no
// candidate; meta: row i's kMeta field; vict: all zero without a pick.
__device__ __forceinline__ void ptol_seq_apply_tail(const PtolSeqArgs& q, int32_t n, int64_t i, int64_t meta, const uint32_t* vict, int lane) {
  const PtolArgs& a = q.t;
  const SeqOverlay& o = q.o;
  const int64_t R = a.row_stride;
  const int prio = prio_of(meta);
  int32_t* const dirty = q.dirty + i * q.n_dirty;
  seq_store_victims(o, i, vict, lane);
  if (meta & (kNever | kHold)) {  // nothing moves
    for (int k = lane; k < q.n_dirty; k += 64) dirty[k] = -1;
    return;
  }
  if (lane == 0) {
    // T4: the nominations row i came with are dropped wherever they sit; with T1-T3 below, these are the nodes whose cells are stale
    int n_dirty = 0;
    if (n >= 0) dirty[n_dirty++] = n;
    for (int32_t t = o.row_nom_ptr[i]; t < o.row_nom_ptr[i + 1]; ++t) {
      const int32_t j = o.row_nom[t], m = q.row_nom_node[t];
      if (o.nom_cleared[j]) continue;
      o.nom_cleared[j] = 1;
      bool listed = false;
      for (int k = 0; k < n_dirty; ++k) listed |= dirty[k] == m;
      if (!listed) dirty[n_dirty++] = m;
    }
    for (; n_dirty < q.n_dirty; ++n_dirty) dirty[n_dirty] = -1;
  }
  if (n < 0) return;
  const PreemptNode& nd = a.nodes[n];
  // T1: the victims leave the node and its Requested
  seq_evict(o, n, vict, lane);
  if (lane < S) {
    const PreemptPod* pods = a.pods + nd.pod_begin;
    int64_t sub = 0;
    for (int k = 0; k < nd.pod_end - nd.pod_begin; ++k) sub += get_bit(vict, k) ? pods[k].fit[lane] : 0;
    o.requested[static_cast<int64_t>(n) * S + lane] -= sub;
  }
  seq_nominate(o, nd, a.noms, n, i, prio, lane, a.row_rec + kMeta * R);  // T3, T2
}

}  // namespace

}  // namespace spx
