// kernels_nrt_tall.hip — gfx950 kernel for NodeResourceTopologyMatch Filter + Score over the snapshot's tall nodes: nodes with more
// NUMA zones than the dense node table holds (SPX_NRT_MAX_ZONES), whose zones travel in a side table (spx_upload_nrt_tall_nodes).
//
// The engine runs it after the dense sweep and the long rows, which saw such a node as one without an NRT object; it overwrites the
// status and score cells of the tall nodes' columns for every row of the range.  Decomposition: lane = tall node (compacted, so the
// lanes are dense over the side table), one pod row per wave at a time, the pod record and its containers — the dense [P][8]
// columns, or the CSR of the long rows — read through wave-uniform loads.  The node's NUMA table stays in memory (nrt_tall_device.h),
// node-major, so that a wave's loads coalesce and the few tall nodes' columns stay in L2.
//
// Container scope needs a table that changes while the containers are walked: the Filter charges each app container to the zone
// it fits, LeastNUMANodes subtracts each container greedily from the subset it chose.  Each wave owns a working copy in an
// engine-owned buffer ([zone][slot][64 lanes], sized by the grid); a lane copies its node's column there before the first charge
// and reads through it from then on.  A lane touches only its own column of its own wave's copy: no inter-wave traffic, no waiting.
// The grid is bounded by that buffer; a wave walks (row, tile) items with the grid's stride.
//
// Int64 reference arithmetic throughout, for all four strategies and both scopes; with SPX_OPT_REFERENCE_KERNELS the same launch.
//
// Reference: pkg/noderesourcetopology/filter.go:42-258, score.go:62-191, least_numa.go:35-233, least_allocated.go,
// most_allocated.go, balanced_allocation.go, numaresources.go:105-215.
#include "nrt_tall_device.h"

namespace spx {

namespace {

template <int SG>
__global__ __launch_bounds__(256) void k_nrt_tall(NrtTallArgs a, int tiles) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t wid = static_cast<int64_t>(blockIdx.x) * 4 + wave;
  const int R = a.n_res;
  const int64_t T = a.n_tall;
  int64_t* const work = a.work + wid * static_cast<int64_t>(a.zone_stride) * R * 64 + lane;
  const int64_t items = (a.row_end - a.row_begin) * tiles;
  for (int64_t w = wid; w < items; w += a.n_waves) {
    const int64_t pod = a.row_begin + w / tiles;
    TallNode nd;
    nd.t = (w % tiles) * 64 + lane;
    const bool in = nd.t < T;
    if (!in) nd.t = T - 1;  // (reads stay inside the table; nothing is written for the lane)
    const uint32_t nflags = a.flags[nd.t];
    nd.nz = in ? a.n_zones[nd.t] : 0;
    if (nd.nz > a.zone_stride) nd.nz = a.zone_stride;
    nd.node_present = a.node_present[nd.t];
    const int max_numa = a.max_numa[nd.t];
    const int64_t n = a.node_idx[nd.t];
    const bool fresh = nflags & SPX_NRT_F_FRESH;
    const bool has_nrt = nflags & SPX_NRT_F_HAS_NRT;
    const bool single = nflags & SPX_NRT_F_SINGLE_NUMA;
    const bool pod_scope = nflags & SPX_NRT_F_POD_SCOPE;
    const AvView table{a.zone_avail + nd.t, T};
    const AvView mine{work, 64};

    // ---- wave-uniform pod record: the dense columns, or the long rows' CSR
    const int qos = a.qos[pod];
    const bool non_native = a.non_native[pod] != 0;
    const uint32_t pod_present = a.pod_present[pod];
    const int64_t* __restrict__ preq = a.pod_req + pod * R;
    int n_ctr = a.n_ctr[pod];
    const uint8_t* __restrict__ ckind = a.ctr_kind + pod * SPX_NRT_MAX_CTRS;
    const uint8_t* __restrict__ cpres = a.ctr_present + pod * SPX_NRT_MAX_CTRS;
    const int64_t* __restrict__ creq = a.ctr_req + pod * SPX_NRT_MAX_CTRS * R;
    const int32_t k_long = a.long_of_row ? a.long_of_row[pod] : -1;
    if (k_long >= 0) {
      const int32_t c0 = a.long_ptr[k_long];
      n_ctr = a.long_ptr[k_long + 1] - c0;
      ckind = a.long_kind + c0;
      cpres = a.long_present + c0;
      creq = a.long_req + static_cast<int64_t>(c0) * R;
    }
    const bool non_g = qos != SPX_QOS_GUARANTEED;

    // ================= Filter (filter.go:179-245)
    uint32_t status = 0;
    if (!(qos == SPX_QOS_BESTEFFORT && !non_native)) {
      if (!fresh) {
        status = SPX_NRT_ST_INVALID_TOPOLOGY;
      } else if (has_nrt && single) {
        if (pod_scope) {  // singleNUMAPodLevelHandler
          uint32_t id;
          if (!tall_fits_any(a, nd, table, non_g, pod_present, preq, &id)) status = SPX_NRT_ST_POD;
        } else {  // singleNUMAContainerLevelHandler
          for (int c = 0; c < n_ctr && status == 0; ++c) {  // init and sidecar containers: must fit, never subtracted
            if (ckind[c] == SPX_CTR_APP) continue;
            uint32_t id;
            if (!tall_fits_any(a, nd, table, non_g, cpres[c], creq + static_cast<int64_t>(c) * R, &id))
              status = ckind[c] == SPX_CTR_SIDECAR ? SPX_NRT_ST_SIDECAR_CONTAINER : SPX_NRT_ST_INIT_CONTAINER;
          }
          bool copied = false;
          for (int c = 0; c < n_ctr && status == 0; ++c) {  // app containers: each charged to the zone it fits before the next
            if (ckind[c] != SPX_CTR_APP) continue;
            const int64_t* q = creq + static_cast<int64_t>(c) * R;
            uint32_t id;
            if (!tall_fits_any(a, nd, copied ? mine : table, non_g, cpres[c], q, &id)) {
              status = SPX_NRT_ST_CONTAINER;
              break;
            }
            if (!copied) {
              for (int e = 0; e < nd.nz * R; ++e) work[static_cast<int64_t>(e) * 64] = table.p[static_cast<int64_t>(e) * T];
              copied = true;
            }
            if (!tall_charge(a, nd, work, non_g, cpres[c], q, id)) status = SPX_NRT_ST_ERROR;  // (ends the walk: fwk.Error)
          }
        }
      }
    }

    // ================= Score (score.go:62-102): on the table as uploaded (the Filter worked on a private copy)
    int64_t score;
    if (non_g) {
      score = 100;
    } else if (!fresh || !has_nrt) {
      score = 0;
    } else if constexpr (SG == kSgLeastNuma) {
      if (pod_scope) {  // leastNUMAPodScopeScore
        if (tall_only_non_numa(a, nd, pod_present)) {
          score = 100;
        } else {
          bool is_min;
          const uint32_t m = tall_numa_nodes_required(a, nd, table, pod_present, preq, &is_min);
          score = m ? normalize_score(__builtin_popcountll(tall_ids_of(a, nd, m)), is_min, max_numa) : 0;
        }
      } else {  // leastNUMAContainerScopeScore
        int max_count = 0;
        bool all_min = true, failed = false, copied = false;
        for (int c = 0; c < n_ctr && !failed; ++c) {
          if (tall_only_non_numa(a, nd, cpres[c])) continue;
          bool is_min;
          const int64_t* q = creq + static_cast<int64_t>(c) * R;
          const uint32_t m = tall_numa_nodes_required(a, nd, copied ? mine : table, cpres[c], q, &is_min);
          if (!m) {
            failed = true;
            break;
          }
          all_min &= is_min;
          const uint64_t ids = tall_ids_of(a, nd, m);
          const int cnt = __builtin_popcountll(ids);
          max_count = cnt > max_count ? cnt : max_count;
          if (!copied) {
            for (int e = 0; e < nd.nz * R; ++e) work[static_cast<int64_t>(e) * 64] = table.p[static_cast<int64_t>(e) * T];
            copied = true;
          }
          tall_subtract_from_numas(a, nd, work, cpres[c], q, ids);
        }
        score = failed ? 0 : (max_count == 0 ? 100 : normalize_score(max_count, all_min, max_numa));
      }
    } else if (!single) {
      score = 0;
    } else if (pod_scope) {
      score = tall_score_each_numa<SG>(a, nd, table, pod_present, preq);
    } else {  // containerScopeScore: int64(mean) over init + app containers
      int64_t sum = 0;
      for (int c = 0; c < n_ctr; ++c) sum += tall_score_each_numa<SG>(a, nd, table, cpres[c], creq + static_cast<int64_t>(c) * R);
      score = n_ctr > 0 ? sum / n_ctr : 0;
    }

    write_cell(a, in, pod, n, status, score);
  }
}

}  // namespace

int64_t nrt_tall_work_bytes(int32_t zone_stride, int32_t n_res, int n_waves) {
  return static_cast<int64_t>(n_waves) * zone_stride * (n_res > 0 ? n_res : 1) * 64 * static_cast<int64_t>(sizeof(int64_t));
}

// the grid: one wave per (row, tile of 64 tall nodes) item, held to what kNrtTallWorkBytes of working copies allow
int nrt_tall_waves(int64_t rows, int32_t n_tall, int32_t zone_stride, int32_t n_res) {
  const int64_t tiles = (n_tall + 63) / 64;
  const int64_t per_wave = nrt_tall_work_bytes(zone_stride, n_res, 1);
  int64_t waves = kNrtTallWorkBytes / per_wave;
  waves = waves < 4 ? 4 : (waves > kNrtTallMaxWaves ? kNrtTallMaxWaves : waves);
  const int64_t items = rows * tiles;
  if (waves > items) waves = items;
  return static_cast<int>((waves + 3) / 4 * 4);
}

void launch_nrt_tall(const NrtTallArgs& a, hipStream_t s) {
  const int64_t rows = a.row_end - a.row_begin;
  if (rows <= 0 || a.n_tall <= 0 || a.n_waves <= 0) return;
  const int tiles = (a.n_tall + 63) / 64;
  const unsigned blocks = static_cast<unsigned>(a.n_waves / 4);
  switch (strategy_group(a.strategy)) {
    case kSgAlloc: hipLaunchKernelGGL((k_nrt_tall<kSgAlloc>), dim3(blocks), dim3(256), 0, s, a, tiles); break;
    case kSgBalanced: hipLaunchKernelGGL((k_nrt_tall<kSgBalanced>), dim3(blocks), dim3(256), 0, s, a, tiles); break;
    default: hipLaunchKernelGGL((k_nrt_tall<kSgLeastNuma>), dim3(blocks), dim3(256), 0, s, a, tiles); break;
  }
}

}  // namespace spx
