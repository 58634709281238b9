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
//   k_ptol_seq_cells   dirty slots x ceil(rows / 256): the column of each dirty node for the rows after i, k_ptol_cells' walk with
//                      the overlay applied.  Rows <= i store nothing, so the cells of row i stay what row i saw at its own step.
//
// A PreemptNever row keeps the cells of the untouched state (the full sweep of k_ptol_cells before step 0): no step stores to them, and
// its victim set is computed with the overlay switched off.
//
// The walk, NodeResourcesFit with default args and the bit-set helpers are restated from kernels_ptol.hip, whose machine code stays as it
// is.  Integer vector code only; every sum is bounded by the upload's 2^62 check (the loop only ever moves requests between sums).
#include "spx_internal.h"

namespace spx {

namespace {

constexpr int S = SPX_QUOTA_SLOTS;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kWords = SPX_PREEMPT_MAX_NODE_PODS / 32;
constexpr int kPdbs = SPX_PREEMPT_MAX_NODE_PDBS;
// fields of the row record (k_ptol_rows writes it)
constexpr int kFit = 0, kMeta = 8, kRow = 9;
static_assert(kRow + 1 == kPtolRowFields, "row record layout");
constexpr int64_t kNever = int64_t{1} << 32;  // kMeta: the priority in the low 32 bits, PreemptNever above them,
constexpr int64_t kHold = int64_t{1} << 33;   // and "not eligible": evaluated at its step, nothing applied

__device__ __forceinline__ int64_t in_vgpr(int64_t x) {
  asm volatile("" : "+v"(x));
  return x;
}

// bit k of a 256-bit set kept as eight registers; k is wave-uniform, so every index below is a compile-time one
__device__ __forceinline__ bool get_bit(const uint32_t* m, int k) {
  uint32_t w = 0;
#pragma unroll
  for (int i = 0; i < kWords; ++i) w = (k >> 5) == i ? m[i] : w;
  return (w >> (k & 31)) & 1u;
}
__device__ __forceinline__ void set_bit(uint32_t* m, int k, bool pred) {
#pragma unroll
  for (int i = 0; i < kWords; ++i) m[i] |= (pred && (k >> 5) == i) ? (1u << (k & 31)) : 0u;
}

__device__ __forceinline__ bool fits(const int64_t* fit, const int64_t* alloc, const int64_t* requested) {
  bool ok = requested[3] + 1 <= alloc[3];
#pragma unroll
  for (int s = 0; s < S; ++s)
    if (s != 3) ok &= !(fit[s] > 0 && fit[s] > alloc[s] - requested[s]);
  return ok;
}

__device__ __forceinline__ int prio_of(int64_t meta) { return static_cast<int>(static_cast<uint32_t>(meta)); }

// One cell per lane: row rr of the list on `node`, for the lanes with want set.  frozen (wave-uniform): the untouched state, as
// k_ptol_cells sees it.  budget: the wave's [kPdbs][64] int16 in LDS.  vict is all zero unless the cell is a CANDIDATE.
__device__ __forceinline__ PreemptCell seq_cell(const PtolSeqArgs& q, int64_t node, int64_t rr, bool want, bool frozen, int16_t (*budget)[64], int lane, uint32_t* vict) {
  const PtolArgs& a = q.t;
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
  const uint32_t* gone = q.gone + node * kWords;
  auto left = [&](int k) { return !frozen && ((gone[k >> 5] >> (k & 31)) & 1u); };  // wave-uniform: the skips below are branches of the wave
  bool live = want && nd.present && (!a.node_mask || a.node_mask[rr * a.n_nodes + node]);

  if (__any(live)) {
    const int L = nd.pod_end - nd.pod_begin;
    // the lane's copy of the node, the nominated pods that outrank the preemptor charged once
    int64_t alloc[S], requested[S];
#pragma unroll
    for (int s = 0; s < S; ++s) alloc[s] = in_vgpr(nd.alloc[s]), requested[s] = frozen ? nd.requested[s] : q.requested[node * S + s];
    for (int j = nd.nom_begin; j < nd.nom_end; ++j) {
      if (!frozen && q.nom_cleared[j]) continue;
      const bool add = a.noms[j].prio >= prio && a.noms[j].row != pod_row;
#pragma unroll
      for (int s = 0; s < S; ++s) requested[s] += add ? a.noms[j].fit[s] : 0;
    }
    if (!frozen) {
      for (int k = q.head[node]; k >= 0; k = q.row_next[k]) {  // the loop's own nominations: earlier rows, so never the lane's own
        if (q.row_cleared[k]) continue;
        const bool add = prio_of(a.row_rec[kMeta * R + k]) >= prio;
#pragma unroll
        for (int s = 0; s < S; ++s) requested[s] += add ? (s == 3 ? 1 : a.row_rec[(kFit + s) * R + k]) : 0;  // a pod counts once
      }
    }
    auto move_pod = [&](int k, bool pred, bool add) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int64_t f = pods[k].fit[s];
        requested[s] += pred ? (add ? f : -f) : 0;
      }
    };

    // step 1: every lower-priority pod still on the node that is not exempted is a potential victim and is removed
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
    if (live) {
      if (class_error) out.status = SPX_PREEMPT_ST_CLASS_ERROR, live = false;
      else if (n_pot == 0) out.status = SPX_PREEMPT_ST_NO_VICTIMS, live = false;
      else if (!fits(fit, alloc, requested)) out.status = SPX_PREEMPT_ST_NOT_FIT, live = false;
    }
    if (__any(live)) {
      // filterPodsWithPDBViolation over the potential victims, most important first; the budgets are the uploaded ones at every step
      const int b0 = nd.pdb_begin, n_pdb = nd.pdb_end - b0;
      if (n_pdb > 0) {
        for (int i = 0; i < n_pdb; ++i) budget[i][lane] = static_cast<int16_t>(max(-1, min(32767, a.pdb_allowed[b0 + i])));
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
      // reprieve, the violating pods first, each list most important first
      int n_vict = 0, n_viol = 0, hi = INT32_MIN;
      int64_t sum = 0, start = INT64_MAX;
      for (int pass = n_pdb > 0 ? 0 : 1; pass < 2; ++pass) {
        for (int k = 0; k < L; ++k) {
          const int pos = pods[k].hi_order;
          if (left(pos)) continue;
          const bool pv = live && get_bit(pot, pos) && (get_bit(viol, pos) == (pass == 0));
          if (!__any(pv)) continue;
          move_pod(pos, pv, true);
          const bool victim = pv && !fits(fit, alloc, requested);
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

// the working copy of Requested; the other parts of the overlay start as all zero / all -1 bytes (launch_ptol_seq_init)
__global__ __launch_bounds__(kBlock) void k_ptol_seq_init(PtolSeqArgs q) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= q.t.n_nodes * S) return;
  q.requested[t] = q.t.nodes[t / S].requested[t % S];
}

// a candidate's keys in the order pickOneNodeForPreemption compares them; smaller is better
struct PickKey {
  int32_t viol, hi, n_vict;
  int64_t sum, neg_start;
};
__device__ __forceinline__ int cmp_key(const PickKey& x, const PickKey& y) {
  if (x.viol != y.viol) return x.viol < y.viol ? -1 : 1;
  if (x.hi != y.hi) return x.hi < y.hi ? -1 : 1;
  if (x.sum != y.sum) return x.sum < y.sum ? -1 : 1;
  if (x.n_vict != y.n_vict) return x.n_vict < y.n_vict ? -1 : 1;
  if (x.neg_start != y.neg_start) return x.neg_start < y.neg_start ? -1 : 1;
  return 0;
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
  if (n >= 0) (void)seq_cell(q, n, i, true, never, s_budget, lane, vict);
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
  const PreemptCell out = seq_cell(q, node, rr, want, false, s_budget[wave], lane, vict);
  if (want) a.cells[node * R + r] = out;
}

inline unsigned blocks_for(int64_t n, int per) { return static_cast<unsigned>((n + per - 1) / per); }

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

}  // namespace spx
