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
// The `pods` set of a quota (addPodIfNotPresent / deletePodIfPresent, elasticquota.go:155-187) needs no per-lane state beyond the
// table's bit: a pod's membership changes only through its own removal and add-back, so after step b's removal it is out of the set
// (the removal shrank Used iff the bit was set), after the reprieve's add-back it is in (Used grows in any case), and a second
// removal always shrinks Used.  Key presence of a scalar in Used only grows (SetScalar).
//
// NodeResourcesFit (default args), "no victims left: no candidate" and pickOneNodeForPreemption restate upstream kube-scheduler code
// that is not in the reference tree.  The launch constants, in_vgpr, the bit-set select chains, fits and the pick's key are
// preempt_device.h's, shared with kernels_ptol.hip and kernels_ptol_seq.hip.  cmp2 and the nominated sums are restated from
// kernels_capacity.hip, whose machine code stays as it is.  Integer vector code only; every sum is bounded by the upload's 2^62 check.
#include "preempt_device.h"

namespace spx {

namespace {

// fields of the row record
constexpr int kReq = 0, kInEq = 8, kTotal = 16, kFit = 24, kPrio = 32, kNs = 33, kFlags = 34, kRow = 35;
static_assert(kRow + 1 == kPreemptRowFields, "row record layout");
// kFlags: bits 0-7 podReq's scalar keys, 8-15 nominatedPodsReqInEQWithPodReq's, 16-23 nominatedPodsReqWithPodReq's
constexpr uint32_t kHasQuota = 1u << 24, kMoreThanMin = 1u << 25;
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

__global__ __launch_bounds__(kBlock) void k_preempt_marks(PreemptArgs a) {
  const int64_t node = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (node >= a.n_nodes) return;
  const int p0 = a.nodes[node].pod_begin, p1 = a.nodes[node].pod_end;
  for (int j = p0; j < p1; ++j) {
    const int ns = a.pods[j].ns;
    uint8_t m = a.pods[j].marks & kMarkInSet;
    if (ns >= 0 && ns < a.n_namespaces && a.has_quota[ns]) {
      m |= kMarkQuota;
      // the quota's Used when the walk reaches pod j: what the earlier removed pods of the namespace (on this node) took out of it
      int64_t used[S];
      uint32_t up = a.used_present[ns];
#pragma unroll
      for (int s = 0; s < S; ++s) used[s] = a.used[static_cast<int64_t>(ns) * S + s];
      for (int k = p0; k < j; ++k) {
        if (a.pods[k].ns != ns || (a.pods[k].marks & (kMarkBorrowed | kMarkInSet)) != (kMarkBorrowed | kMarkInSet)) continue;
#pragma unroll
        for (int s = 0; s < S; ++s) used[s] = wsub(used[s], a.pods[k].qreq[s]);
        up |= a.pods[k].qreq_present;
      }
      if (cmp2(used, up, nullptr, a.min + static_cast<int64_t>(ns) * S, a.min_present[ns], 0)) m |= kMarkBorrowed;  // usedOverMin()
    }
    a.pods[j].marks = m;
  }
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
  uint32_t vict[kWords];
#pragma unroll
  for (int i = 0; i < kWords; ++i) vict[i] = 0;
  const PreemptNode& nd = a.nodes[node];
  const PreemptPod* pods = a.pods + nd.pod_begin;  // position in the node's list -> record
  bool live = active && nd.present && (!a.node_mask || a.node_mask[rr * a.n_nodes + node]);

  if (__any(live)) {
    const int L = nd.pod_end - nd.pod_begin;
    // the lane's copy of the node, the nominated pods that outrank the preemptor charged once: they are re-added before every Filter run
    int64_t alloc[S], requested[S];
#pragma unroll
    for (int s = 0; s < S; ++s) alloc[s] = in_vgpr(nd.alloc[s]), requested[s] = nd.requested[s];
    for (int j = nd.nom_begin; j < nd.nom_end; ++j) {
      const bool add = a.noms[j].prio >= prio && a.noms[j].row != pod_row;
#pragma unroll
      for (int s = 0; s < S; ++s) requested[s] += add ? a.noms[j].fit[s] : 0;
    }
    // the lane's copy of the ElasticQuotaInfos: the preemptor's quota and the aggregate
    const int qn = pq ? ns : 0;
    int64_t own[S], agg[S], mx[S], agg_min[S];
    uint32_t own_p = 0, agg_p = a.agg_used_present, mx_p = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) own[s] = 0, mx[s] = 0, agg[s] = a.agg_used[s], agg_min[s] = in_vgpr(a.agg_min[s]);
    if (pq) {
#pragma unroll
      for (int s = 0; s < S; ++s) own[s] = a.used[static_cast<int64_t>(qn) * S + s], mx[s] = a.max[static_cast<int64_t>(qn) * S + s];
      own_p = a.used_present[qn], mx_p = a.max_present[qn];
    }
    // usedOverMaxWith(x) || aggregatedUsedOverMinWith(y)
    auto quota_over = [&](const int64_t* x, uint32_t xp, const int64_t* y, uint32_t yp) {
      int64_t sum[S];
#pragma unroll
      for (int s = 0; s < S; ++s) sum[s] = wadd(agg[s], y[s]);
      return cmp2(x, xp, own, mx, mx_p, INT64_MAX) || cmp2(sum, agg_p | yp, nullptr, agg_min, a.agg_min_present, 0);
    };
    // RemovePod / AddPod of the pod at position k on the lane's copies; `quota`: the pod's ElasticQuotaInfo moves too
    auto move_pod = [&](int k, bool pred, bool quota, bool add) {
      const uint32_t qp = pods[k].qreq_present;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int64_t f = pods[k].fit[s], q = pods[k].qreq[s];
        requested[s] += pred ? (add ? f : -f) : 0;
        const int64_t dq = (pred && quota) ? (add ? q : -q) : 0;
        agg[s] += dq;
        own[s] += more ? dq : 0;  // a victim shares the preemptor's quota exactly when the preemptor is over its min (:558)
      }
      if (pred && quota) agg_p |= qp, own_p |= more ? qp : 0u;
    };

    // step b: the potential victims, least important first, each removed
    uint32_t pot[kWords], viol[kWords];
#pragma unroll
    for (int i = 0; i < kWords; ++i) pot[i] = viol[i] = 0;
    int n_pot = 0;
    for (int k = 0; k < L; ++k) {
      const int jns = pods[k].ns, jprio = pods[k].prio;
      const uint8_t m = pods[k].marks;
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
      else if (!fits(fit, alloc, requested)) out.status = SPX_PREEMPT_ST_NOT_FIT, live = false;
      else if (pq && quota_over(req, req_p, req, req_p)) out.status = SPX_PREEMPT_ST_QUOTA, live = false;
    }
    if (__any(live)) {
      // step f: filterPodsWithPDBViolation over the potential victims, most important first
      const int b0 = nd.pdb_begin, n_pdb = nd.pdb_end - b0;
      if (n_pdb > 0) {
        for (int i = 0; i < n_pdb; ++i) s_budget[wave][i][lane] = static_cast<int16_t>(max(-1, min(32767, a.pdb_allowed[b0 + i])));  // 256 decrements at most
        for (int k = 0; k < L; ++k) {
          const int pos = pods[k].hi_order;
          uint32_t bits = pods[pos].pdb_mask;
          if (!bits) continue;
          const bool pv = live && get_bit(pot, pos);
          bool hit = false;
          while (bits) {
            const int i = __builtin_ctz(bits);
            bits &= bits - 1;
            if (pv) {
              const int16_t left = s_budget[wave][i][lane] - 1;
              s_budget[wave][i][lane] = left;
              hit |= left < 0;
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
          const bool pv = live && get_bit(pot, pos) && (get_bit(viol, pos) == (pass == 0));
          if (!__any(pv)) continue;
          move_pod(pos, pv, pq, true);
          const bool gone = pv && !fits(fit, alloc, requested);
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
  if (!active) return;
  if (out.status != SPX_PREEMPT_ST_CANDIDATE) {
#pragma unroll
    for (int i = 0; i < kWords; ++i) vict[i] = 0;
  }
  a.cells[static_cast<int64_t>(blockIdx.x) * R + r] = out;
  if (a.victims_out) {
#pragma unroll
    for (int i = 0; i < kWords; ++i) a.victims_out[i] = vict[i];
  }
}

__global__ __launch_bounds__(kBlock) void k_preempt_pick(PreemptArgs a) {
  __shared__ PickKey s_key[kWaves][64];
  __shared__ int32_t s_node[kWaves][64], s_cand[kWaves][64], s_ties[kWaves][64];
  const int slice = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t R = a.row_stride, r = static_cast<int64_t>(blockIdx.x) * 64 + lane;  // r < R: the cells of the padding rows are never read below
  PickKey best{0, 0, 0, 0, 0};
  int32_t node = -1, cand = 0, ties = 0;
  if (r < a.n_rows) {
    for (int64_t n = slice; n < a.n_nodes; n += kWaves) {
      const PreemptCell c = a.cells[n * R + r];
      if (c.status != SPX_PREEMPT_ST_CANDIDATE) continue;
      const PickKey key{c.n_violations, c.hi_prio, c.n_victims, c.prio_sum, -c.start};
      const int o = cand ? cmp_key(key, best) : -1;
      ++cand;
      if (o < 0) best = key, node = static_cast<int32_t>(n), ties = 1;
      else if (o == 0) ++ties;  // nodes ascend within a slice: the first one stays
    }
  }
  s_key[slice][lane] = best, s_node[slice][lane] = node, s_cand[slice][lane] = cand, s_ties[slice][lane] = ties;
  __syncthreads();
  if (slice != 0 || r >= a.n_rows) return;
  for (int w = 1; w < kWaves; ++w) {
    if (s_cand[w][lane] == 0) continue;
    const int o = cand ? cmp_key(s_key[w][lane], best) : -1;
    cand += s_cand[w][lane];
    if (o < 0) best = s_key[w][lane], node = s_node[w][lane], ties = s_ties[w][lane];
    else if (o == 0) ties += s_ties[w][lane], node = min(node, s_node[w][lane]);
  }
  a.pick[0 * R + r] = node;
  a.pick[1 * R + r] = node >= 0 ? best.n_vict : 0;
  a.pick[2 * R + r] = node >= 0 ? best.viol : 0;
  a.pick[3 * R + r] = cand;
  a.pick[4 * R + r] = ties;
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

void launch_preempt_pick(const PreemptArgs& a, hipStream_t s) {
  if (a.n_rows > 0) hipLaunchKernelGGL(k_preempt_pick, dim3(blocks_for(a.n_rows, 64)), dim3(kBlock), 0, s, a);
}

}  // namespace spx
