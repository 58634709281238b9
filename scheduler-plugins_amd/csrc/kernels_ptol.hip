// kernels_ptol.hip — PreemptionToleration.PostFilter's preemption dry run: SelectVictimsOnNode (pkg/preemptiontoleration/
// preemption_toleration.go:188-299) for every (preemptor, node) cell.  The pick per preemptor is k_preempt_pick of
// kernels_preempt.hip on the cells written here.
//
//   k_ptol_rows   a thread per preemptor: its NodeResourcesFit vector, priority, PreemptNever and pod row into a [field][row] record
//   k_ptol_cells  a wave per node, a lane per preemptor, as k_preempt_cells: the node's pod list arrives through wave-uniform (scalar)
//                 loads and every lane walks the same trip count under its own predicate.  Per lane, in registers: the node's Requested
//                 (8 int64) and three 256-bit sets (potential victims, PDB-violating, victims); the PDB budgets are 32 int16 per lane
//                 in LDS.  There is no quota state.
//
// The walk is DefaultPreemption's with one more predicate per (preemptor, lower-priority pod) pair, ExemptedFromPreemption (:129-181).
// What of it depends on the pod alone is folded into the PtolPod record by the host (flatten_ptol.cc): the class lookup, the parsed
// policy, and scheduledAt + TolerationSeconds as one instant.  What is left per pair is
//     exempted = has_class && (never || (prio < min_prio && until > now))
// and a missing class among the lower-priority pods is the node's error.
//
// NodeResourcesFit (default args), "no victims left: no candidate" and the helpers below (the bit-set select chains, fits, in_vgpr)
// are restated from kernels_preempt.hip, whose machine code stays as it is.  Integer vector code only; every sum is bounded by the
// upload's 2^62 check.
#include "spx_internal.h"

namespace spx {

namespace {

constexpr int S = SPX_QUOTA_SLOTS;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kWords = SPX_PREEMPT_MAX_NODE_PODS / 32;
constexpr int kPdbs = SPX_PREEMPT_MAX_NODE_PDBS;
// fields of the row record
constexpr int kFit = 0, kMeta = 8, kRow = 9;
static_assert(kRow + 1 == kPtolRowFields, "row record layout");
constexpr int64_t kNever = int64_t{1} << 32;  // kMeta: the priority in the low 32 bits, PreemptNever above them

// A wave-uniform value the whole cell keeps reading (the node's Allocatable) would sit in scalar registers for the length of the
// kernel, next to the pod records the walk streams through them; a vector register per lane is what this kernel has to spare.
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

// NodeResourcesFit.fitsRequest with default args on the lane's copy of the node (nominated pods already charged): the pod count, then per
// resource "insufficient iff req > 0 && req > allocatable - requested".  A pod whose requests are all zero fails none of those.
__device__ __forceinline__ bool fits(const int64_t* fit, const int64_t* alloc, const int64_t* requested) {
  bool ok = requested[3] + 1 <= alloc[3];
#pragma unroll
  for (int s = 0; s < S; ++s)
    if (s != 3) ok &= !(fit[s] > 0 && fit[s] > alloc[s] - requested[s]);
  return ok;
}

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

  // the preemptor
  int64_t fit[S];
#pragma unroll
  for (int s = 0; s < S; ++s) fit[s] = a.row_rec[(kFit + s) * R + rr];
  const int64_t meta = a.row_rec[kMeta * R + rr];
  const int prio = static_cast<int>(static_cast<uint32_t>(meta));
  const bool never = meta & kNever;
  const int64_t pod_row = a.row_rec[kRow * R + rr];
  const int64_t now = a.now;

  PreemptCell out{0, 0, 0, 0, 0, SPX_PREEMPT_ST_SKIPPED};
  uint32_t vict[kWords];
#pragma unroll
  for (int i = 0; i < kWords; ++i) vict[i] = 0;
  const PreemptNode& nd = a.nodes[node];
  const PreemptPod* pods = a.pods + nd.pod_begin;  // position in the node's list -> record
  const PtolPod* tol = a.tol + nd.pod_begin;
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
    // NodeInfo.RemovePod / AddPod of the pod at position k on the lane's copy
    auto move_pod = [&](int k, bool pred, bool add) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int64_t f = pods[k].fit[s];
        requested[s] += pred ? (add ? f : -f) : 0;
      }
    };

    // step 1 (:218-236): every lower-priority pod that is not exempted is a potential victim and is removed
    uint32_t pot[kWords], viol[kWords];
#pragma unroll
    for (int i = 0; i < kWords; ++i) pot[i] = viol[i] = 0;
    int n_pot = 0;
    bool class_error = false;
    for (int k = 0; k < L; ++k) {
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
      else if (!fits(fit, alloc, requested)) out.status = SPX_PREEMPT_ST_NOT_FIT, live = false;
    }
    if (__any(live)) {
      // step 4: filterPodsWithPDBViolation over the potential victims, most important first
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
      // step 5: reprieve, the violating pods first, each list most important first
      int n_vict = 0, n_viol = 0, hi = INT32_MIN;
      int64_t sum = 0, start = INT64_MAX;
      for (int pass = n_pdb > 0 ? 0 : 1; pass < 2; ++pass) {
        for (int k = 0; k < L; ++k) {
          const int pos = pods[k].hi_order;
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

inline unsigned blocks_for(int64_t n, int per) { return static_cast<unsigned>((n + per - 1) / per); }

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
