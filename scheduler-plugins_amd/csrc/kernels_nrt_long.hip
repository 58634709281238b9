// kernels_nrt_long.hip — gfx950 kernel for NodeResourceTopologyMatch Filter + Score of the batch's long rows: pods with more
// containers than the dense pod table holds (SPX_NRT_MAX_CTRS), whose containers travel in CSR (spx_upload_nrt_long_pods).
//
// The engine runs it after the dense sweep, which saw such a row as a pod without containers; it overwrites the row's status and
// score cells.  Decomposition as the reference-arithmetic kernel (kernels_nrt.hip): lane = node, one long row per wave, the row's
// containers read through scalar (wave-uniform) loads, the node's NUMA table (int64 availability, ids, presence) held in VGPRs.
// Container-scope Filter subtracts each app container from the zone it fits (subtractResourcesFromNUMANodeList) and, as
// LeastNUMANodes' greedy subtraction, restores the lane's table by re-reading it: any number of containers, no per-container undo
// record.  Score in int64 reference arithmetic; container scope divides the sum over all containers by their count (integer part
// of the float64 mean: the sum is at most 100 x n_ctr, far inside float64's exact range).
//
// Reference: pkg/noderesourcetopology/filter.go:42-258, score.go:62-191, least_numa.go:35-233, least_allocated.go,
// most_allocated.go, balanced_allocation.go, numaresources.go:105-215.
//
// The reference's arithmetic itself — the node record and every helper over it — is in nrt_ref_device.h, shared with kernels_nrt.hip
// and kernels_nrt_wide.hip; here are the grid, the CSR container source and the ladder over it.
#include "nrt_ref_device.h"

namespace spx {

namespace {

// grid: 1-D, (long row, group of four 64-node tiles); block = four waves, wave w of block b -> tile 4 (b % groups) + w
template <int RM, int SG>
__global__ __launch_bounds__(256, 2) void k_nrt_long(NrtLongArgs a, int groups) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t tile = static_cast<int64_t>(blockIdx.x % groups) * 4 + wave;
  int64_t k = a.long_begin + blockIdx.x / groups;
  if (a.row_ptr) {  // sequential commit: the row lives on the device; nothing to do unless it is a long row
    const int64_t row = *a.row_ptr;
    if (row < 0 || row >= a.n_pods) return;
    k = a.long_of_row[row];
    if (k < 0) return;
  } else if (k >= a.long_end) {
    return;
  }
  k = __builtin_amdgcn_readfirstlane(static_cast<int>(k));
  const int64_t n = tile * 64 + lane;
  const bool in = n < a.n_nodes;
  if (__ballot(in) == 0) return;
  const int R = a.n_res;

  NodeState<RM> ns;
  const uint32_t nflags = in ? a.flags[n] : 0u;
  ns.nz = in ? a.n_zones[n] : 0;
  ns.node_present = in ? a.node_present[n] : 0u;
  const int max_numa = in ? a.max_numa[n] : 8;
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
  const bool fresh = nflags & SPX_NRT_F_FRESH;
  const bool has_nrt = nflags & SPX_NRT_F_HAS_NRT;
  const bool single = nflags & SPX_NRT_F_SINGLE_NUMA;
  const bool pod_scope = nflags & SPX_NRT_F_POD_SCOPE;

  // ---- wave-uniform pod record: pod-level columns of the dense table, containers of the CSR
  const int64_t pod = a.pod_row[k];
  const int qos = a.qos[pod];
  const bool non_native = a.non_native[pod] != 0;
  const uint32_t pod_present = a.pod_present[pod];
  const int64_t* __restrict__ preq = a.pod_req + pod * R;
  const int32_t c0 = a.ctr_ptr[k], c1 = a.ctr_ptr[k + 1];
  const int n_ctr = c1 - c0;
  const uint8_t* __restrict__ ckind = a.ctr_kind + c0;
  const uint8_t* __restrict__ cpres = a.ctr_present + c0;
  const int64_t* __restrict__ creq = a.ctr_req + static_cast<int64_t>(c0) * R;
  const bool non_g = qos != SPX_QOS_GUARANTEED;

  // ================= Filter (filter.go:179-245)
  uint32_t status = 0;
  if (!(qos == SPX_QOS_BESTEFFORT && !non_native)) {
    if (!fresh) {
      status = SPX_NRT_ST_INVALID_TOPOLOGY;
    } else if (has_nrt && single) {
      if (pod_scope) {  // singleNUMAPodLevelHandler
        uint32_t id;
        if (!fits_any(ns, a, non_g, pod_present, preq, &id)) status = SPX_NRT_ST_POD;
      } else {  // singleNUMAContainerLevelHandler
        for (int c = 0; c < n_ctr; ++c) {  // init and sidecar containers: must fit, never subtracted
          if (ckind[c] == SPX_CTR_APP) continue;
          uint32_t id;
          const bool ok = fits_any(ns, a, non_g, cpres[c], creq + static_cast<int64_t>(c) * R, &id);
          if (status == 0 && !ok) status = ckind[c] == SPX_CTR_SIDECAR ? SPX_NRT_ST_SIDECAR_CONTAINER : SPX_NRT_ST_INIT_CONTAINER;
        }
        bool dirty = false;
        for (int c = 0; c < n_ctr; ++c) {  // app containers: each charged to the zone it fits before the next is tested
          if (ckind[c] != SPX_CTR_APP) continue;
          uint32_t id;
          bool negative;
          const bool ok = fits_any(ns, a, non_g, cpres[c], creq + static_cast<int64_t>(c) * R, &id, &negative);
          const bool live = status == 0;
          if (live && !ok) status = SPX_NRT_ST_CONTAINER;
          if (live && negative) status = SPX_NRT_ST_ERROR;  // ends the walk (fwk.Error)
          const bool apply = live && ok;
          adjust_numa(ns, a, non_g, cpres[c], creq + static_cast<int64_t>(c) * R, id, apply, -1);
          dirty |= apply;
        }
        if (dirty) load_avail(ns, a, n, in);  // Filter works on a private copy in the reference
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
        score = m ? normalize_score(__builtin_popcountll(ids_of(ns, m)), is_min, max_numa) : 0;  // (the count is of NUMA ids)
      }
    } else {  // leastNUMAContainerScopeScore
      int max_count = 0;
      bool all_min = true, failed = false;
      for (int c = 0; c < n_ctr; ++c) {
        if (failed || only_non_numa(ns, cpres[c])) continue;
        bool is_min;
        const int64_t* q = creq + static_cast<int64_t>(c) * R;
        const uint32_t m = numa_nodes_required(ns, a, n, cpres[c], q, &is_min);
        if (!m) {
          failed = true;
          continue;
        }
        all_min &= is_min;
        const uint64_t ids = ids_of(ns, m);
        const int cnt = __builtin_popcountll(ids);  // numaNodes.Count(): distinct NUMA ids, not zones
        max_count = cnt > max_count ? cnt : max_count;
        subtract_from_numas(ns, a, cpres[c], q, ids);
      }
      score = failed ? 0 : (max_count == 0 ? 100 : normalize_score(max_count, all_min, max_numa));
    }
  } else if (!single) {
    score = 0;
  } else if (pod_scope) {
    score = score_each_numa<RM, SG>(ns, a, pod_present, preq);
  } else {  // containerScopeScore: int64(mean) over init + app containers
    int64_t sum = 0;
    for (int c = 0; c < n_ctr; ++c) sum += score_each_numa<RM, SG>(ns, a, cpres[c], creq + static_cast<int64_t>(c) * R);
    score = n_ctr > 0 ? sum / n_ctr : 0;
  }

  write_cell(a, in, pod, n, status, score);
}

}  // namespace

void launch_nrt_long(const NrtLongArgs& a, hipStream_t s) {
  const int64_t rows = a.row_ptr ? 1 : a.long_end - a.long_begin;
  if (rows <= 0 || a.n_nodes <= 0) return;
  const int groups = static_cast<int>((a.n_nodes + 255) / 256);
  const unsigned blocks = static_cast<unsigned>(rows * groups);
  const int sg = strategy_group(a.strategy);
#define SPX_NRT_LONG_CASE(RMV, SGV)                                                          \
  if ((a.n_res <= 4) == (RMV == 4) && sg == SGV) {                                           \
    hipLaunchKernelGGL((k_nrt_long<RMV, SGV>), dim3(blocks), dim3(256), 0, s, a, groups);   \
    return;                                                                                  \
  }
  SPX_NRT_LONG_CASE(4, kSgAlloc)
  SPX_NRT_LONG_CASE(4, kSgBalanced)
  SPX_NRT_LONG_CASE(4, kSgLeastNuma)
  SPX_NRT_LONG_CASE(8, kSgAlloc)
  SPX_NRT_LONG_CASE(8, kSgBalanced)
  SPX_NRT_LONG_CASE(8, kSgLeastNuma)
#undef SPX_NRT_LONG_CASE
}

}  // namespace spx
