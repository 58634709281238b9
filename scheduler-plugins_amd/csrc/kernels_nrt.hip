// kernels_nrt.hip — gfx950 kernel for NodeResourceTopologyMatch Filter + Score (NUMA-zone fit).
//
// Decomposition: lane = node, pod record = wave-uniform.  One wavefront owns 64 consecutive nodes and a
// chunk of pod rows.  A node's NUMA table (up to 8 zones x RM resources of int64 "available", presence
// bitmasks, NUMA ids) is loaded once into VGPRs — node columns are stored zone/resource-major
// ([z][r][node]) so that those loads are coalesced — and every pod of the chunk is then evaluated
// against it with the pod's container requests arriving through scalar (wave-uniform) loads, so the
// container/resource loops and the QoS branches are uniform; only per-node properties (scope, policy,
// zone count) diverge.  Container-scope Filter mutates the table exactly like the reference
// (subtractResourcesFromNUMANodeList) and undoes it before scoring; LeastNUMANodes' greedy subtraction
// is undone by re-reading the lane's table.
//
// This path is VALU-bound integer work (C x R x Z compares, subtractions, small divisions per cell),
// not HBM-bound: per (pod,node) it writes 2 bytes and reads nothing from HBM.
//
// Reference: pkg/noderesourcetopology/filter.go:42-258, score.go:62-191, least_numa.go:35-233,
// least_allocated.go, most_allocated.go, balanced_allocation.go, numaresources.go:105-215.
//
// The reference's arithmetic itself — the node record and every helper over it — is in nrt_ref_device.h, shared with
// kernels_nrt_long.hip and kernels_nrt_wide.hip; here are the grid, the dense [P][8] container columns and the ladder over them.
#include <cstdlib>

#include "nrt_ref_device.h"

namespace spx {

namespace {

constexpr int kC = SPX_NRT_MAX_CTRS;
constexpr int kPodsPerUnit = 16;

// NodeState (nrt_ref_device.h) with the node's flags and its max_numa inside, where this kernel has always kept them: the
// committed profiles are stamped with this unit's machine code, and the record's layout is part of it (numa_nodes_required
// reads it through memory)
template <int RM>
struct SweepNode {
  int64_t avail[kZ][RM];
  ZoneIds ids;
  uint32_t zp_lo, zp_hi;
  int nz;
  uint32_t flags;
  uint32_t node_present;
  int max_numa;
  __device__ __forceinline__ uint32_t id(int z) const { return ids.id(z); }
  __device__ __forceinline__ uint32_t zp(int z) const { return ((z < 4 ? zp_lo >> (8 * z) : zp_hi >> (8 * (z - 4))) & 0xffu); }
};

template <int RM, int SG>
__global__ __launch_bounds__(256, 2) void k_nrt(NrtArgs a, int n_tiles) {
  SPX_RESOLVE_ROWS(a);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t unit = static_cast<int64_t>(blockIdx.x) * 4 + wave;
  const int tile = static_cast<int>(unit % n_tiles);
  const int64_t chunk = unit / n_tiles;
  const int64_t pod0 = a.row_begin + chunk * kPodsPerUnit;
  if (pod0 >= a.row_end) return;
  const int64_t pod1 = pod0 + kPodsPerUnit < a.row_end ? pod0 + kPodsPerUnit : a.row_end;
  const int64_t n = static_cast<int64_t>(tile) * 64 + lane;
  const bool in = n < a.n_nodes;
  const int R = a.n_res;

  SweepNode<RM> ns;
  ns.flags = in ? a.flags[n] : 0u;
  ns.nz = in ? a.n_zones[n] : 0;
  ns.node_present = in ? a.node_present[n] : 0u;
  ns.max_numa = in ? a.max_numa[n] : 8;
  ns.ids.lo = ns.ids.hi = ns.zp_lo = ns.zp_hi = 0;
#pragma unroll
  for (int z = 0; z < kZ; ++z) {
    const uint32_t idv = in ? a.zone_id[static_cast<int64_t>(z) * a.n_nodes + n] : 0u;
    const uint32_t zpv = in ? a.zone_present[static_cast<int64_t>(z) * a.n_nodes + n] : 0u;
    ns.ids.set(z, idv);
    if (z < 4) ns.zp_lo |= zpv << (8 * z);
    else ns.zp_hi |= zpv << (8 * (z - 4));
  }
  load_avail(ns, a, n, in);
  const bool fresh = ns.flags & SPX_NRT_F_FRESH;
  const bool has_nrt = ns.flags & SPX_NRT_F_HAS_NRT;
  const bool single = ns.flags & SPX_NRT_F_SINGLE_NUMA;
  const bool pod_scope = ns.flags & SPX_NRT_F_POD_SCOPE;

  for (int64_t pod = pod0; pod < pod1; ++pod) {
    // ---- wave-uniform pod record
    const int qos = a.qos[pod];
    const bool non_native = a.non_native[pod] != 0;
    const int n_ctr = a.n_ctr[pod];
    const uint32_t pod_present = a.pod_present[pod];
    const int64_t* __restrict__ preq = a.pod_req + pod * R;
    const uint8_t* __restrict__ ckind = a.ctr_kind + pod * kC;
    const uint8_t* __restrict__ cpres = a.ctr_present + pod * kC;
    const int64_t* __restrict__ creq = a.ctr_req + pod * kC * R;
    const bool non_g = qos != SPX_QOS_GUARANTEED;

    // ================= Filter (filter.go:179-245)
    uint32_t status = 0;
    if (!(qos == SPX_QOS_BESTEFFORT && !non_native)) {  // uniform
      if (!fresh) {
        status = SPX_NRT_ST_INVALID_TOPOLOGY;
      } else if (has_nrt && single) {
        if (pod_scope) {  // singleNUMAPodLevelHandler
          uint32_t id;
          if (!fits_any(ns, a, non_g, pod_present, preq, &id)) status = SPX_NRT_ST_POD;
        } else {  // singleNUMAContainerLevelHandler
          for (int c = 0; c < n_ctr; ++c) {  // init containers: must fit, never subtracted
            if (ckind[c] == SPX_CTR_APP) continue;
            uint32_t id;
            const bool ok = fits_any(ns, a, non_g, cpres[c], creq + c * R, &id);
            if (status == 0 && !ok) status = ckind[c] == SPX_CTR_SIDECAR ? SPX_NRT_ST_SIDECAR_CONTAINER : SPX_NRT_ST_INIT_CONTAINER;
          }
          uint64_t chosen = 0;   // NUMA id picked per app container (for the undo), 8 bits each
          uint32_t placed = 0;   // bit c: container c was subtracted on this lane
          for (int c = 0; c < n_ctr; ++c) {
            if (ckind[c] != SPX_CTR_APP) continue;
            uint32_t id;
            bool negative;
            const bool ok = fits_any(ns, a, non_g, cpres[c], creq + c * R, &id, &negative);
            const bool live = status == 0;
            if (live && !ok) status = SPX_NRT_ST_CONTAINER;
            if (live && negative) status = SPX_NRT_ST_ERROR;  // ends the walk (fwk.Error); its charge is applied and undone like any other
            const bool apply = live && ok;
            adjust_numa(ns, a, non_g, cpres[c], creq + c * R, id, apply, -1);
            chosen |= static_cast<uint64_t>(apply ? id : 0u) << (8 * c);
            placed |= (apply ? 1u : 0u) << c;
          }
          for (int c = 0; c < n_ctr; ++c) {  // undo: Filter works on a private copy in the reference
            if (ckind[c] != SPX_CTR_APP) continue;
            adjust_numa(ns, a, non_g, cpres[c], creq + c * R, static_cast<uint32_t>((chosen >> (8 * c)) & 0xffu),
                        (placed >> c) & 1u, +1);
          }
        }
      }
    }

    // ================= Score (score.go:62-102)
    int64_t score;
    if (non_g) {
      score = 100;
    } else if (!fresh || !has_nrt) {
      score = 0;
    } else if constexpr (SG == kSgLeastNuma) {
      if (pod_scope) {  // leastNUMAPodScopeScore
        if (only_non_numa(ns, pod_present)) {
          score = 100;
        } else {
          bool is_min;
          const uint32_t m = numa_nodes_required(ns, a, n, pod_present, preq, &is_min);
          score = m ? normalize_score(__builtin_popcountll(ids_of(ns, m)), is_min, ns.max_numa) : 0;  // (the count is of NUMA ids)
        }
      } else {  // leastNUMAContainerScopeScore
        int max_count = 0;
        bool all_min = true, failed = false, dirty = false;
        for (int c = 0; c < n_ctr; ++c) {
          if (failed || only_non_numa(ns, cpres[c])) continue;
          bool is_min;
          const uint32_t m = numa_nodes_required(ns, a, n, cpres[c], creq + c * R, &is_min);
          if (!m) {
            failed = true;
            continue;
          }
          all_min &= is_min;
          const uint64_t ids = ids_of(ns, m);
          const int cnt = __builtin_popcountll(ids);  // numaNodes.Count(): distinct NUMA ids, not zones
          max_count = cnt > max_count ? cnt : max_count;
          subtract_from_numas(ns, a, cpres[c], creq + c * R, ids);
          dirty = true;
        }
        score = failed ? 0 : (max_count == 0 ? 100 : normalize_score(max_count, all_min, ns.max_numa));
        if (dirty) load_avail(ns, a, n, in);  // the reference scored on a private NUMANodeList
      }
    } else if (!single) {
      score = 0;
    } else if (pod_scope) {
      score = score_each_numa<RM, SG>(ns, a, pod_present, preq);
    } else {  // containerScopeScore: int64(mean) over init + app containers
      int64_t sum = 0;
      for (int c = 0; c < n_ctr; ++c) sum += score_each_numa<RM, SG>(ns, a, cpres[c], creq + c * R);
      score = n_ctr > 0 ? sum / n_ctr : 0;
    }

    if (in && a.out_raw != nullptr) {  // parity harness: the int64 Score() value, one row
      a.out_raw[n] = score;
    } else if (in) {
      const int64_t cell = pod * a.row_stride + n;
      a.out_status[cell] = static_cast<uint8_t>(status);
      score = score < 0 ? 0 : (score > 255 ? 255 : score);
      a.out_score[cell] = static_cast<uint8_t>(score);
    }
  }
}

}  // namespace

namespace {
__global__ __launch_bounds__(256) void k_nrt_creq_from_items(const uint32_t* __restrict__ items, int n_res, int64_t n_pods, int64_t* __restrict__ out) {
  const int iw = n_res <= 4 ? 16 : 32;  // dwords per item; items 2.. of a pod's 10 are its containers (spx_engine.hip: nrt_pod_items)
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;  // (pod, container, resource)
  if (i >= n_pods * SPX_NRT_MAX_CTRS * n_res) return;
  const int r = static_cast<int>(i % n_res);
  const int64_t pc = i / n_res;
  const int c = static_cast<int>(pc % SPX_NRT_MAX_CTRS);
  const int64_t pod = pc / SPX_NRT_MAX_CTRS;
  const uint32_t* w = items + (pod * 10 + 2 + c) * iw + 2 * r;
  out[i] = static_cast<int64_t>(__hiloint2double(static_cast<int>(w[1]), static_cast<int>(w[0])));
}
}  // namespace

void launch_nrt_creq_from_items(const uint32_t* pod_items, int n_res, int64_t n_pods, int64_t* ctr_req, hipStream_t s) {
  const int64_t n = n_pods * SPX_NRT_MAX_CTRS * n_res;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_nrt_creq_from_items, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, pod_items, n_res, n_pods, ctr_req);
}

// true = the sweep ran as the fused Filter + Score launch (kernels_nrt_fused.hip)
bool launch_nrt(const NrtArgs& a, hipStream_t s) {
  if (a.row_end <= a.row_begin) return false;
  const bool generic_only = (a.opts & kOptNrtGeneric) != 0;  // SPX_OPT_REFERENCE_KERNELS
  if (!generic_only && launch_nrt_fused(a, s)) return true;
  if (!generic_only && launch_nrt_fast(a, s)) return false;
  const int n_tiles = static_cast<int>((a.n_nodes + 63) / 64);
  const int64_t chunks = (a.row_end - a.row_begin + kPodsPerUnit - 1) / kPodsPerUnit;
  const unsigned blocks = static_cast<unsigned>((chunks * n_tiles + 3) / 4);
  const int sg = strategy_group(a.strategy);
#define SPX_NRT_CASE(RMV, SGV)                                                               \
  if ((a.n_res <= 4) == (RMV == 4) && sg == SGV) {                                           \
    hipLaunchKernelGGL((k_nrt<RMV, SGV>), dim3(blocks), dim3(256), 0, s, a, n_tiles);       \
    return false;                                                                            \
  }
  SPX_NRT_CASE(4, kSgAlloc)
  SPX_NRT_CASE(4, kSgBalanced)
  SPX_NRT_CASE(4, kSgLeastNuma)
  SPX_NRT_CASE(8, kSgAlloc)
  SPX_NRT_CASE(8, kSgBalanced)
  SPX_NRT_CASE(8, kSgLeastNuma)
#undef SPX_NRT_CASE
  return false;
}

}  // namespace spx
