// cap_cell.h — CapacityScheduling's SelectVictimsOnNode (pkg/capacityscheduling/capacity_scheduling.go:486-677) for one (preemptor,
// node) cell per lane, the borrowed marks of a node's pods, and the row record both read: the one copy of the walk that
// kernels_preempt.hip (k_preempt_cells and k_preempt_marks, on the uploaded state) and kernels_preempt_seq.hip (the sequential loop,
// on the state its earlier rows left) run, and with nrt_refit.h's Filter in the refit kernels_preempt_nrt.hip and
// kernels_preempt_nrt_seq.hip; and the end of a loop's step (cap_seq_apply_tail), which k_cnrt_seq_apply calls and k_cap_seq_apply keeps
// written out, so that its machine code stays what it was.
//
// The node's pod list arrives through wave-uniform (scalar) loads and every lane walks the same trip count under its own predicate.
// Per lane, in registers: the node's Requested, the preemptor quota's Used, the aggregate Used (8 int64 each) with their scalar-key
// masks, and three 256-bit sets (potential victims, PDB-violating, victims); the PDB budgets are 32 int16 per lane in LDS.
//
// The `pods` set of a quota (addPodIfNotPresent / deletePodIfPresent, elasticquota.go:155-187) needs no per-lane state beyond the
// table's bit: a pod's membership changes only through its own removal and add-back, so after step b's removal it is out of the set
// (the removal shrank Used iff the bit was set), after the reprieve's add-back it is in (Used grows in any case), and a second
// removal always shrinks Used.  Key presence of a scalar in Used only grows (SetScalar).
//
// The refit (RunFilterPluginsWithNominatedPods, :607 and :636) is NodeResourcesFit and whatever the Refit policy adds to it
// (preempt_device.h states the three calls): FitOnly nothing, nrt_refit.h's NrtRefit NodeResourceTopologyMatch's Filter, which sees the
// pods removed so far (kernels_preempt_nrt.hip).  The borrowed marks depend on no Filter.
//
// cmp2 is restated from kernels_capacity.hip, whose machine code stays as it is.  Integer vector code only; every sum is bounded by the
// upload's 2^62 check.
#pragma once

#include "preempt_device.h"

namespace spx {

namespace {

// fields of the row record
constexpr int kReq = 0, kInEq = 8, kTotal = 16, kFit = 24, kPrio = 32, kNs = 33, kFlags = 34, kRow = 35;
static_assert(kRow + 1 == kPreemptRowFields, "row record layout");
// kFlags: bits 0-7 podReq's scalar keys, 8-15 nominatedPodsReqInEQWithPodReq's, 16-23 nominatedPodsReqWithPodReq's
constexpr uint32_t kHasQuota = 1u << 24, kMoreThanMin = 1u << 25;
constexpr uint32_t kHold = 1u << 26;  // the sequential loop: "not eligible", evaluated at its step, nothing applied
constexpr uint8_t kMarkInSet = 1, kMarkQuota = 2, kMarkBorrowed = 4;

__device__ __forceinline__ int64_t wadd(int64_t a, int64_t b) { return static_cast<int64_t>(static_cast<uint64_t>(a) + static_cast<uint64_t>(b)); }
__device__ __forceinline__ int64_t wsub(int64_t a, int64_t b) { return static_cast<int64_t>(static_cast<uint64_t>(a) - static_cast<uint64_t>(b)); }

// cmp2 elasticquota.go:193-221 (x2 == nullptr: cmp)
__device__ __forceinline__ bool cmp2(const int64_t* x1, uint32_t x1p, const int64_t* x2, const int64_t* y, uint32_t yp, int64_t bound) {
  bool over = false;
#pragma unroll
  for (int s = 0; s < 4; ++s) over |= wadd(x1[s], x2 ? x2[s] : 0) > y[s];
#pragma unroll
  for (int s = 4; s < S; ++s) {
    const int64_t yq = ((yp >> s) & 1u) ? y[s] : bound;
    over |= ((x1p >> s) & 1u) && wadd(x1[s], x2 ? x2[s] : 0) > yq;
  }
  return over;
}

// The marks of one node's pods: which of them a preemptor of ANOTHER namespace removes when it borrows back (:572).  A pod goes iff its
// quota is usedOverMin() when the walk reaches it, and that depends only on the removals of its own namespace's earlier pods.
// kOverlay off: from the uploaded Used, into the pod records.  kOverlay on: from the loop's working Used, skipping the pods that left,
// into the loop's working mark bytes; the uploaded marks are only read for the in-set bit.
template <bool kOverlay>
__device__ __forceinline__ void cap_marks(const PreemptArgs& a, const CapSeqArgs* q, int64_t node) {
  const int p0 = a.nodes[node].pod_begin, p1 = a.nodes[node].pod_end;
  const int64_t* const used_tab = kOverlay ? q->used : a.used;
  const uint8_t* const usedp_tab = kOverlay ? q->used_present : a.used_present;
  auto left = [&](int j) { return kOverlay && seq_left(q->gone, node, j - p0); };
  auto mark_of = [&](int j) -> uint8_t { return kOverlay ? q->marks[j] : a.pods[j].marks; };
  for (int j = p0; j < p1; ++j) {
    if (left(j)) continue;
    const int ns = a.pods[j].ns;
    uint8_t m = a.pods[j].marks & kMarkInSet;
    if (ns >= 0 && ns < a.n_namespaces && a.has_quota[ns]) {
      m |= kMarkQuota;
      // the quota's Used when the walk reaches pod j: what the earlier removed pods of the namespace (on this node) took out of it
      int64_t used[S];
      uint32_t up = usedp_tab[ns];
#pragma unroll
      for (int s = 0; s < S; ++s) used[s] = used_tab[static_cast<int64_t>(ns) * S + s];
      for (int k = p0; k < j; ++k) {
        if (left(k) || a.pods[k].ns != ns || (mark_of(k) & (kMarkBorrowed | kMarkInSet)) != (kMarkBorrowed | kMarkInSet)) continue;
#pragma unroll
        for (int s = 0; s < S; ++s) used[s] = wsub(used[s], a.pods[k].qreq[s]);
        up |= a.pods[k].qreq_present;
      }
      if (cmp2(used, up, nullptr, a.min + static_cast<int64_t>(ns) * S, a.min_present[ns], 0)) m |= kMarkBorrowed;  // usedOverMin()
    }
    if (kOverlay) q->marks[j] = m;
    else a.pods[j].marks = m;
  }
}

// One cell per lane: row rr of the list on `node`, for the lanes with want set.  budget: the wave's [kPdbs][64] int16 in LDS.  vict
// is all zero unless the cell is a CANDIDATE.
// kOverlay off: the uploaded state; q (NULL) is not read.
// kOverlay on: the sequential loop's state (kernels_preempt_seq.hip) from *q: Requested, every quota's Used, the aggregate and the marks
// are the working copies, cleared nominations are not charged, the loop's own nominations are, and the positions in `gone` are
// skipped in every pass.  A skipped position never reaches move_pod, so the refit policy never hears of a pod that left at an earlier
// step.
template <bool kOverlay, class Refit = FitOnly>
__device__ __forceinline__ PreemptCell cap_cell(const PreemptArgs& a, const CapSeqArgs* q, int64_t node, int64_t rr, bool want, int16_t (*budget)[64], int lane, uint32_t* vict,
                                                Refit rf = Refit{}) {
  const int64_t R = a.row_stride;
  // the preemptor
  int64_t req[S], in_eq[S], total[S], fit[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    req[s] = a.row_rec[(kReq + s) * R + rr];
    in_eq[s] = a.row_rec[(kInEq + s) * R + rr];
    total[s] = a.row_rec[(kTotal + s) * R + rr];
    fit[s] = a.row_rec[(kFit + s) * R + rr];
  }
  const int prio = static_cast<int>(a.row_rec[kPrio * R + rr]);
  const int ns = static_cast<int>(a.row_rec[kNs * R + rr]);
  const uint32_t flags = static_cast<uint32_t>(a.row_rec[kFlags * R + rr]);
  const int64_t pod_row = a.row_rec[kRow * R + rr];
  const bool pq = flags & kHasQuota, more = flags & kMoreThanMin;
  const uint32_t req_p = flags & 0xffu, in_p = (flags >> 8) & 0xffu, total_p = (flags >> 16) & 0xffu;

  PreemptCell out{0, 0, 0, 0, 0, SPX_PREEMPT_ST_SKIPPED};
#pragma unroll
  for (int i = 0; i < kWords; ++i) vict[i] = 0;
  const PreemptNode& nd = a.nodes[node];
  const PreemptPod* pods = a.pods + nd.pod_begin;  // position in the node's list -> record
  auto left = [&](int k) { return kOverlay && seq_left(q->gone, node, k); };
  auto mark_at = [&](int k) -> uint8_t { return kOverlay ? q->marks[nd.pod_begin + k] : pods[k].marks; };
  bool live = want && nd.present && (!a.node_mask || a.node_mask[rr * a.n_nodes + node]);

  if (__any(live)) {
    const int L = nd.pod_end - nd.pod_begin;
    rf.begin(node, rr, lane);
    // the lane's copy of the node, the nominated pods that outrank the preemptor charged once: they are re-added before every Filter run
    int64_t alloc[S], requested[S];
#pragma unroll
    for (int s = 0; s < S; ++s) alloc[s] = in_vgpr(nd.alloc[s]), requested[s] = kOverlay ? q->requested[node * S + s] : nd.requested[s];
    for (int j = nd.nom_begin; j < nd.nom_end; ++j) {
      if (kOverlay && q->nom_cleared[j]) continue;
      const bool add = a.noms[j].prio >= prio && a.noms[j].row != pod_row;
#pragma unroll
      for (int s = 0; s < S; ++s) requested[s] += add ? a.noms[j].fit[s] : 0;
    }
    if (kOverlay) {
      for (int k = q->head[node]; k >= 0; k = q->row_next[k]) {  // the loop's own nominations: earlier rows, so never the lane's own
        if (q->row_cleared[k]) continue;
        const bool add = static_cast<int>(a.row_rec[kPrio * R + k]) >= prio;
#pragma unroll
        for (int s = 0; s < S; ++s) requested[s] += add ? (s == 3 ? 1 : a.row_rec[(kFit + s) * R + k]) : 0;  // a pod counts once
      }
    }
    // the lane's copy of the ElasticQuotaInfos: the preemptor's quota and the aggregate
    const int qn = pq ? ns : 0;
    int64_t own[S], agg[S], mx[S], agg_min[S];
    uint32_t own_p = 0, agg_p = kOverlay ? *q->agg_used_present : a.agg_used_present, mx_p = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) own[s] = 0, mx[s] = 0, agg[s] = kOverlay ? q->agg_used[s] : a.agg_used[s], agg_min[s] = in_vgpr(a.agg_min[s]);
    if (pq) {
#pragma unroll
      for (int s = 0; s < S; ++s) own[s] = (kOverlay ? q->used : a.used)[static_cast<int64_t>(qn) * S + s], mx[s] = a.max[static_cast<int64_t>(qn) * S + s];
      own_p = (kOverlay ? q->used_present : a.used_present)[qn], mx_p = a.max_present[qn];
    }
    // usedOverMaxWith(x) || aggregatedUsedOverMinWith(y)
    auto quota_over = [&](const int64_t* x, uint32_t xp, const int64_t* y, uint32_t yp) {
      int64_t sum[S];
#pragma unroll
      for (int s = 0; s < S; ++s) sum[s] = wadd(agg[s], y[s]);
      return cmp2(x, xp, own, mx, mx_p, INT64_MAX) || cmp2(sum, agg_p | yp, nullptr, agg_min, a.agg_min_present, 0);
    };
    // RemovePod / AddPod of the pod at position k on the lane's copies; `quota`: the pod's ElasticQuotaInfo moves too.  Every one of them
    // runs the PreFilter extensions (:513, :523), the removal for the quota (:646-649) included: that pod is on the policy's stack from then on.
    auto move_pod = [&](int k, bool pred, bool quota, bool add) {
      const uint32_t qp = pods[k].qreq_present;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int64_t f = pods[k].fit[s], qq = pods[k].qreq[s];
        requested[s] += pred ? (add ? f : -f) : 0;
        const int64_t dq = (pred && quota) ? (add ? qq : -qq) : 0;
        agg[s] += dq;
        own[s] += more ? dq : 0;  // a victim shares the preemptor's quota exactly when the preemptor is over its min (:558)
      }
      if (pred && quota) agg_p |= qp, own_p |= more ? qp : 0u;
      rf.moved(nd.pod_begin + k, pred, add);
    };

    // step b: the potential victims, least important first, each removed
    uint32_t pot[kWords], viol[kWords];
#pragma unroll
    for (int i = 0; i < kWords; ++i) pot[i] = viol[i] = 0;
    int n_pot = 0;
    for (int k = 0; k < L; ++k) {
      if (left(k)) continue;
      const int jns = pods[k].ns, jprio = pods[k].prio;
      const uint8_t m = mark_at(k);
      const bool with_eq = m & kMarkQuota;
      const bool pv = live && (!pq ? (!with_eq && jprio < prio)
                                   : more ? (with_eq && jns == ns && jprio < prio) : (with_eq && jns != ns && (m & kMarkBorrowed)));
      if (!__any(pv)) continue;
      set_bit(pot, k, pv);
      n_pot += pv;
      move_pod(k, pv, pq && (m & kMarkInSet), false);
    }
    // steps c, d, e
    if (live) {
      if (n_pot == 0) out.status = SPX_PREEMPT_ST_NO_VICTIMS, live = false;
      else if (!fits(fit, alloc, requested) || !rf.ok()) out.status = SPX_PREEMPT_ST_NOT_FIT, live = false;
      else if (pq && quota_over(req, req_p, req, req_p)) out.status = SPX_PREEMPT_ST_QUOTA, live = false;
    }
    if (__any(live)) {
      // step f: filterPodsWithPDBViolation over the potential victims, most important first; the budgets are the uploaded ones, in the
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
      // step g: reprieve, the violating pods first, each list most important first
      int n_vict = 0, n_viol = 0, hi = INT32_MIN;
      int64_t sum = 0, start = INT64_MAX;
      for (int pass = n_pdb > 0 ? 0 : 1; pass < 2; ++pass) {
        for (int k = 0; k < L; ++k) {
          const int pos = pods[k].hi_order;
          if (left(pos)) continue;
          const bool pv = live && get_bit(pot, pos) && (get_bit(viol, pos) == (pass == 0));
          if (!__any(pv)) continue;
          move_pod(pos, pv, pq, true);
          const bool gone = pv && !(fits(fit, alloc, requested) && rf.ok());
          move_pod(pos, gone, pq, false);
          const bool over = pv && pq && quota_over(in_eq, in_p, total, total_p);
          if (over && gone) out.status = SPX_PREEMPT_ST_REMOVE_TWICE, live = false;
          const bool again = over && !gone;
          move_pod(pos, again, pq, false);
          const bool victim = (gone || again) && live;
          set_bit(vict, pos, victim);
          if (victim) {
            const int jprio = pods[pos].prio;
            const int64_t jstart = pods[pos].start;
            ++n_vict;
            n_viol += (pass == 0 && gone);
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

// The end of step i in the apply kernel of a CapacityScheduling loop (k_cnrt_seq_apply; k_cap_seq_apply ends with the same lines, written
// out there: DESIGN.md 3.9j says why), called by all lanes of its one wave once the picked cell (i, n) is computed again: the victim set
// is stored (32 B per row); then T4, T1 with the movement of the victims' quotas' Used and of the aggregate, T3 and T2.  n: the pick,
// -1 = no candidate; flags, prio: row i's kFlags and kPrio fields; vict: all zero without a pick.  Whatever the refit kept a victim
// for, it leaves its quota here like any other.
__device__ __forceinline__ void cap_seq_apply_tail(const CapSeqArgs& q, int32_t n, int64_t i, uint32_t flags, int prio, const uint32_t* vict, int lane) {
  const PreemptArgs& a = q.t;
  const SeqOverlay o = q.overlay();
  const int64_t R = a.row_stride;
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

}  // namespace spx
