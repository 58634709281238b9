// nrt_refit.h — NodeResourceTopologyMatch's Filter as the refit policy of a preemption cell walk: the one copy
// that kernels_ptol_nrt.hip (PreemptionToleration's walk, ptol_cell.h) and kernels_preempt_nrt.hip (CapacityScheduling's, cap_cell.h)
// run, with the preemptors' NRT row record and the kernel that writes it.
// SelectVictimsOnNode runs every Filter after each removal and add-back; NRT's (filter.go:179-245) sees the pods removed so far as its
// preemption stack (prefilter.go:66-102), simulates their eviction on the zone table (preemption.go:39-157) and runs the single-NUMA
// handler on the result.
//
// The simulation is additive, so a lane keeps the sums of what its stack releases, S[zone position][slot], and the Filter reads
// available + S.  Per lane that is up to 64 int64, too much next to the walk's registers: it lives in LDS, [entry][lane] like the PDB
// budgets, sized at launch to the table's most zones x its slots: 512 bytes an entry for the one wave of a workgroup, 32 KiB at 8 x 8.
// The container-scope handler needs a working copy of the zone table while it places containers; it places them in S itself and takes
// them out again, which is exact in integers.  A lane also keeps the size of its stack, how many pods on it contribute, and how many
// entries of S are above their headroom (allocatable - available): a pod entering or leaving the stack touches only its own releases,
// so "available + sum > allocatable anywhere" is a counter, not a scan.
//
// The single-NUMA arithmetic is nrt_ref_device.h's (resourcesAvailableInAnyNUMANodes, subtractResourcesFromNUMANodeList) restated for
// lane = preemptor: there the node is the lane's and the pod wave-uniform, here the node's zone table arrives through wave-uniform loads
// and the pod's requests are the lane's.
//
// Nothing here reads a plugin's own tables: NrtRefitArgs (spx_internal.h) is the side table and the record, and the row list's stride, which
// the plugin's arguments hold, is handed over by the kernel that builds the policy.
#pragma once

#include "preempt_device.h"

namespace spx {

namespace {

constexpr int kZ = SPX_NRT_MAX_ZONES, kR = SPX_NRT_MAX_RES, kC = SPX_NRT_MAX_CTRS;
constexpr int kMeta0 = 0, kKinds = 1, kCtrPresent = 2, kPodReq = 3, kCtrReq = 3 + kR;  // fields of the NRT row record
static_assert(kCtrReq + kC * kR == kPnrtRowFields, "NRT row record layout");

// A thread per preemptor: its NRT record (spx_nrt_pods_soa's columns) into a [field][row] record next to the plugin's own.  Args: a
// plugin's arguments `t` (rows, n_rows, row_stride) with the NrtRefitArgs `n` beside them.
template <class Args>
__global__ __launch_bounds__(256) void k_pnrt_rows(Args a) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (r >= a.t.n_rows) return;
  const int64_t R = a.t.row_stride, pod = a.t.rows[r];
  const int nr = a.n.n_res;
  uint64_t kinds = 0, present = 0;
  for (int c = 0; c < kC; ++c) {
    kinds |= static_cast<uint64_t>(a.n.ctr_kind[pod * kC + c]) << (8 * c);
    present |= static_cast<uint64_t>(a.n.ctr_present[pod * kC + c]) << (8 * c);
  }
  a.n.nrt_rec[kMeta0 * R + r] = static_cast<int64_t>(a.n.qos[pod]) | (a.n.non_native[pod] ? 1 << 8 : 0) | (static_cast<int64_t>(a.n.n_ctr[pod]) << 16) |
                                (static_cast<int64_t>(a.n.pod_present[pod]) << 24);
  a.n.nrt_rec[kKinds * R + r] = static_cast<int64_t>(kinds);
  a.n.nrt_rec[kCtrPresent * R + r] = static_cast<int64_t>(present);
  for (int s = 0; s < kR; ++s) a.n.nrt_rec[(kPodReq + s) * R + r] = s < nr ? a.n.pod_req[pod * nr + s] : 0;
  for (int c = 0; c < kC; ++c)
    for (int s = 0; s < kR; ++s) a.n.nrt_rec[(kCtrReq + c * kR + s) * R + r] = s < nr ? a.n.ctr_req[(pod * kC + c) * nr + s] : 0;
}

template <class Args>
void launch_nrt_rows(const Args& a, hipStream_t s) {
  if (a.t.n_rows > 0) hipLaunchKernelGGL(k_pnrt_rows<Args>, dim3(blocks_for(a.t.n_rows, 256)), dim3(256), 0, s, a);
}

// the dynamic LDS of a cell kernel: the wave's release sums
inline size_t pnrt_lds_bytes(const NrtRefitArgs& n) { return static_cast<size_t>(max(1, n.max_zones * n.n_res)) * 64 * sizeof(int64_t); }

// NRT's Filter as a walk's refit policy (preempt_device.h states the three calls).
struct NrtRefit {
  const NrtRefitArgs* a;
  int64_t R;           // the row list's stride: the NRT record is [field][R]
  int64_t* sum;        // the wave's [zones x n_res][64] in LDS
  const PnrtNode* nd;
  int64_t rr;
  int lane;
  uint32_t meta;       // the lane's qos, non_native, n_ctr, pod_present
  int max_ctr;         // the most containers any lane's preemptor has
  int stack, contrib, over;
  int cached;          // without a simulation F does not depend on the stack: -1 = not asked yet, else the answer
  bool sim;            // wave-uniform: this node's Filter simulates evictions (mode on, a fresh NRT, placement info with containers)

  // zone position z, slot r of the lane
  __device__ __forceinline__ int64_t& at(int z, int r) const { return sum[(z * a->n_res + r) * 64 + lane]; }

  __device__ __forceinline__ void begin(int64_t node, int64_t row, int l) {
    nd = a->nodes + node, rr = row, lane = l;
    meta = static_cast<uint32_t>(a->nrt_rec[kMeta0 * R + rr]);
    const uint32_t f = nd->flags;
    // a wave whose preemptors are all BestEffort without a non-native request never reads the table (filter.go:183-186): it keeps no state
    const bool table = (f & SPX_NRT_F_HAS_NRT) && (f & SPX_NRT_F_FRESH) && __any(!((meta & 0xff) == SPX_QOS_BESTEFFORT && !((meta >> 8) & 1u)));
    sim = a->mode && table && (f & SPX_PNRT_F_PLACEMENT);
    stack = contrib = over = 0, cached = -1;
    max_ctr = 0;
    const int n_ctr = (meta >> 16) & 0xff;
    for (int c = 1; c <= kC; ++c) max_ctr = __any(n_ctr >= c) ? c : max_ctr;
    if (table && (sim || (f & SPX_NRT_F_SINGLE_NUMA))) {
      const int nz = nd->n_zones;
      for (int z = 0; z < nz; ++z)
        for (int r = 0; r < a->n_res; ++r) at(z, r) = 0;
    }
  }

  // RemovePod pushes the pod onto the stack, AddPod pops it (prefilter.go:66-102)
  __device__ __forceinline__ void moved(int j, bool pred, bool add) {
    if (!sim) return;
    const int d = add ? -1 : 1;
    stack += pred ? d : 0;
    contrib += pred && a->contributes[j] ? d : 0;
    for (int k = a->rel_ptr[j]; k < a->rel_ptr[j + 1]; ++k) {
      const int e = a->rel[k].entry;
      const int64_t q = a->rel[k].qty, room = nd->headroom[e >> 3][e & 7];
      if (pred) {
        const int64_t was = at(e >> 3, e & 7), now = add ? was - q : was + q;
        at(e >> 3, e & 7) = now;
        over += static_cast<int>(now > room) - static_cast<int>(was > room);
      }
    }
  }

  __device__ __forceinline__ bool slot_is(int r, int flag) const { return (a->slot_flags >> (8 * r)) & static_cast<uint64_t>(flag); }

  // resourcesAvailableInAnyNUMANodes (filter.go:93-163) for the requests at fields [base, base + n_res) of the lane's record
  __device__ __forceinline__ bool fits_any(uint32_t present, int base, bool non_g, uint32_t* numa_id) const {
    const int nz = nd->n_zones;
    uint64_t bitmask = ~0ull;
    bool ok = true;
    for (int r = 0; r < a->n_res; ++r) {
      const int64_t q = a->nrt_rec[(base + r) * R + rr];
      const bool use = ((present >> r) & 1u) && q != 0;  // "ignoring zero-qty resource request"
      const bool always = non_g && slot_is(r, SPX_NRT_SLOT_AFFINE);  // isResourceSetSuitable
      ok &= !(use && !((nd->node_present >> r) & 1u));  // not reported at node level: cannot meet the request
      bool has_affinity = false;
      uint64_t rb = 0;
      for (int z = 0; z < nz; ++z) {
        if (!((nd->zone_present[z] >> r) & 1u)) continue;
        has_affinity = true;
        const int64_t have = nd->avail[z][r] + at(z, r);
        rb |= (always || have >= q) ? 1ull << nd->zone_id[z] : 0ull;
      }
      if (use && !(!has_affinity && slot_is(r, SPX_NRT_SLOT_HOST_LEVEL))) bitmask &= rb;
    }
    *numa_id = bitmask ? static_cast<uint32_t>(__builtin_ctzll(bitmask)) : 0u;
    return ok && bitmask != 0;
  }

  // subtractResourcesFromNUMANodeList (numaresources.go:145-182) on the lane's table (sign -1), and its exact inverse (+1).  True when
  // a charge leaves a zone below zero (two zones share the id, only one holds the request): the reference returns an error there
  // (:172-175) and the Filter fwk.Error (filter.go:73-77), which is a Filter that did not succeed.  The whole charge is applied all the
  // same, so that the inverse restores the table.
  __device__ __forceinline__ bool adjust(uint32_t present, int base, bool non_g, uint32_t numa_id, bool apply, int sign) const {
    const int nz = nd->n_zones;
    bool negative = false;
    for (int r = 0; r < a->n_res; ++r) {
      const int64_t q = a->nrt_rec[(base + r) * R + rr];
      const bool take = apply && ((present >> r) & 1u) && !(non_g && slot_is(r, SPX_NRT_SLOT_AFFINE)) && q != 0;
      for (int z = 0; z < nz; ++z) {
        if (!((nd->zone_present[z] >> r) & 1u)) continue;
        if (take && nd->zone_id[z] == numa_id) {
          const int64_t now = at(z, r) + sign * q;
          at(z, r) = now;
          negative |= sign < 0 && nd->avail[z][r] + now < 0;
        }
      }
    }
    return negative;
  }

  // filter.go:179-245 on the lane's stack
  __device__ __forceinline__ bool filter() const {
    const uint32_t f = nd->flags;
    const int qos = meta & 0xff, n_ctr = (meta >> 16) & 0xff;
    const bool non_g = qos != SPX_QOS_GUARANTEED;
    if (qos == SPX_QOS_BESTEFFORT && !((meta >> 8) & 1u)) return true;
    if (!(f & SPX_NRT_F_FRESH)) return false;
    if (!(f & SPX_NRT_F_HAS_NRT)) return true;
    if (sim && stack > 0 && (contrib == 0 || over > 0)) return false;  // "no resources to add" / "exceeds NUMA allocatable"
    if (!(f & SPX_NRT_F_SINGLE_NUMA)) return true;
    uint32_t id;
    if (f & SPX_NRT_F_POD_SCOPE) return fits_any((meta >> 24) & 0xff, kPodReq, non_g, &id);
    const uint64_t kinds = static_cast<uint64_t>(a->nrt_rec[kKinds * R + rr]), present = static_cast<uint64_t>(a->nrt_rec[kCtrPresent * R + rr]);
    bool pass = true;
    for (int c = 0; c < max_ctr; ++c) {  // init and sidecar containers: must fit, never subtracted
      const bool mine = c < n_ctr && ((kinds >> (8 * c)) & 0xff) != SPX_CTR_APP;
      const bool ok = fits_any((present >> (8 * c)) & 0xff, kCtrReq + c * kR, non_g, &id);
      pass &= !(mine && !ok);
    }
    uint64_t chosen = 0;  // the NUMA id taken per app container, 8 bits each, for the undo
    uint32_t placed = 0;
    for (int c = 0; c < max_ctr; ++c) {
      const bool mine = c < n_ctr && ((kinds >> (8 * c)) & 0xff) == SPX_CTR_APP;
      const uint32_t cp = (present >> (8 * c)) & 0xff;
      const bool ok = fits_any(cp, kCtrReq + c * kR, non_g, &id);
      const bool apply = mine && pass && ok;
      pass &= !(mine && !ok);
      pass &= !adjust(cp, kCtrReq + c * kR, non_g, id, apply, -1);  // "inconsistent resource accounting": no later container is placed
      chosen |= static_cast<uint64_t>(apply ? id : 0u) << (8 * c);
      placed |= (apply ? 1u : 0u) << c;
    }
    for (int c = 0; c < max_ctr; ++c)  // the reference's Filter works on a private copy
      adjust((present >> (8 * c)) & 0xff, kCtrReq + c * kR, non_g, static_cast<uint32_t>((chosen >> (8 * c)) & 0xff), (placed >> c) & 1u, +1);
    return pass;
  }

  __device__ __forceinline__ bool ok() {
    if (sim || cached < 0) cached = filter();
    return cached != 0;
  }
};

}  // namespace

}  // namespace spx
