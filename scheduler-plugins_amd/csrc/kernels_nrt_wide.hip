// kernels_nrt_wide.hip — gfx950 kernel for NodeResourceTopologyMatch Filter + Score over the wide tables: snapshots with up to
// SPX_NRT_MAX_RES_WIDE resource slots (spx_nrt_nodes_wide / spx_nrt_pods_wide).
//
// Every reference loop that touches a resource walks the pod's or the container's request (filter.go:93-163, score.go:110-124,
// least_numa.go:156-215): resources nobody requests are never read.  The kernel is therefore sparse in the requested slots.  Lane =
// node, one pod row per wave (wave-uniform): the row's (slot, quantity) lists are read through uniform loads, and a lane reads a zone
// quantity from the node-major column [Z][n_res][N] only for a slot the current list names.  No per-lane table of every slot: the cost
// follows the slots a pod requests, not the snapshot's slot count.
//
// Container scope charges each app container to the NUMA id it fits (subtractResourcesFromNUMANodeList) and LeastNUMANodes charges each
// container to its chosen subset (subtractFromNUMAs).  A lane records each container's choice as one byte in LDS (rec[c][lane]: the
// chosen id | 0x80, or the subset's position mask); the quantity of slot s a later container sees is the table's, replayed through the
// earlier containers' records that name s.  Every slot evolves on its own, so the replay is exact.  Integer arithmetic in int64;
// container scope divides the sum over all containers by their count.
//
// A different algorithm from the dense kernels' (lists, not a table per lane), so fits_any / zone_score / numa_nodes_required here are its
// own.  What is the same — the subset table, div_le100, value_of, normalize_score, the packed NUMA ids, the strategy groups and the write
// of a cell — comes from nrt_ref_device.h.
//
// Reference: pkg/noderesourcetopology/filter.go:42-258, score.go:62-191, least_numa.go:35-233, least_allocated.go,
// most_allocated.go, balanced_allocation.go, numaresources.go:105-215.
#include "nrt_ref_device.h"

namespace spx {

namespace {

constexpr int kMaxCtrs = SPX_NRT_WIDE_MAX_CTRS;
constexpr int kBlock = 256;
constexpr int kCache = 4;        // LeastNUMANodes: requested slots whose zone quantities a lane holds during the subset search
constexpr int kNoReplay = 0;     // the table's quantities
constexpr int kFilterReplay = 1; // less the app containers charged before (Filter, container scope)
constexpr int kGreedyReplay = 2; // less the subsets the containers before took (LeastNUMANodes, container scope)
constexpr uint32_t kApplied = 0x80u;

// a wave-uniform request list: entries in ascending slot order
struct WList {
  const uint8_t* __restrict__ slot;
  const int64_t* __restrict__ qty;
  int n;
};

__device__ __forceinline__ uint32_t list_mask(const WList& l) {
  uint32_t m = 0;
  for (int e = 0; e < l.n; ++e) m |= 1u << l.slot[e];
  return m;
}

// the lane's node: NUMA ids and per-zone presence masks (the zone quantities stay in memory)
struct WideNode {
  int64_t n;
  ZoneIds ids;
  uint32_t zp[kZ];  // per-zone resource-presence mask
  int nz;
  uint32_t node_present;
  __device__ __forceinline__ uint32_t id(int z) const { return ids.id(z); }
  __device__ __forceinline__ bool reports(int z, int s) const { return z < nz && ((zp[z] >> s) & 1u); }
};

__device__ __forceinline__ int64_t avail_of(const WideNode& ns, const NrtWideArgs& a, int z, int s) {
  return ns.reports(z, s) ? a.zone_avail[(static_cast<int64_t>(z) * a.n_res + s) * a.n_nodes + ns.n] : 0;
}

// the earlier containers of the row whose records change the quantities a list sees
struct Hist {
  int32_t cbase;  // the row's first container (absolute)
  int upto;       // containers 0 .. upto-1 of the row
  bool non_g;
};

// quantity of slot s in container c's list (wave-uniform), 0 when it does not name s
__device__ __forceinline__ int64_t ctr_qty(const NrtWideArgs& a, int32_t c, int s) {
  for (int32_t e = a.ent_ptr[c], e1 = a.ent_ptr[c + 1]; e < e1; ++e) {
    const int es = a.ent_slot[e];
    if (es == s) return a.ent_qty[e];
    if (es > s) break;
  }
  return 0;
}

// the zone quantities of slot s as the lane sees them before container h.upto of the row
template <int MODE>
__device__ __forceinline__ void cur_avail(int64_t (&v)[kZ], const WideNode& ns, const NrtWideArgs& a, int s, const Hist& h,
                                          const uint8_t (*rec)[kBlock]) {
#pragma unroll
  for (int z = 0; z < kZ; ++z) v[z] = avail_of(ns, a, z, s);
  if constexpr (MODE == kNoReplay) {
    return;
  } else {
    if (MODE == kFilterReplay && h.non_g && (a.slot_flags[s] & SPX_NRT_SLOT_AFFINE)) return;  // never charged for such a pod
    for (int c = 0; c < h.upto; ++c) {
      if (MODE == kFilterReplay && a.ctr_kind[h.cbase + c] != SPX_CTR_APP) continue;
      const int64_t q = ctr_qty(a, h.cbase + c, s);
      if (q == 0) continue;
      const uint32_t r = rec[c][threadIdx.x];
      if constexpr (MODE == kFilterReplay) {  // subtractResourcesFromNUMANodeList numaresources.go:145-182
        const bool applied = r & kApplied;
        const uint32_t id = r & 63u;
#pragma unroll
        for (int z = 0; z < kZ; ++z) v[z] -= (applied && ns.reports(z, s) && ns.id(z) == id) ? q : 0;
      } else {  // subtractFromNUMAs numaresources.go:184-215: the bitmask holds NUMA ids but indexes list positions
        int64_t quantity = q;
#pragma unroll
        for (int z = 0; z < kZ; ++z) {
          const bool member = ((r >> z) & 1u) && ns.reports(z, s) && quantity != 0;
          const int64_t available = v[z];
          const int64_t take = quantity >= available ? available : quantity;
          v[z] = member ? available - take : available;
          quantity = member ? quantity - take : quantity;
        }
      }
    }
  }
}

// resourcesAvailableInAnyNUMANodes filter.go:93-163.  *negative (kFilterReplay): charging the list to the id it fits, as
// subtractResourcesFromNUMANodeList does to every zone that carries the id, would leave one of them below zero — a twin of the zone
// that fits holds less than the request (numaresources.go:172-175: an error, filter.go:73-77: fwk.Error).  The quantities are the ones
// the fit was decided on, so the sign test costs no second replay.
template <int MODE>
__device__ __forceinline__ bool fits_any(const WideNode& ns, const NrtWideArgs& a, const WList& l, const Hist& h, const uint8_t (*rec)[kBlock],
                                         uint32_t* numa_id, bool* negative = nullptr) {
  uint64_t bitmask = ~0ull;
  uint64_t short_ids = 0;  // ids of reporting zones that hold less than a quantity the charge takes
  bool ok = true;
  for (int e = 0; e < l.n; ++e) {
    const int s = l.slot[e];
    const int64_t q = l.qty[e];
    if (q == 0) continue;  // "ignoring zero-qty resource request"
    const uint8_t sf = a.slot_flags[s];
    const bool always = h.non_g && (sf & SPX_NRT_SLOT_AFFINE);  // isResourceSetSuitable
    const bool host_level = sf & SPX_NRT_SLOT_HOST_LEVEL;
    if (!((ns.node_present >> s) & 1u)) ok = false;  // not reported at node level -> cannot meet request
    int64_t v[kZ];
    if (always) {
#pragma unroll
      for (int z = 0; z < kZ; ++z) v[z] = 0;
    } else {
      cur_avail<MODE>(v, ns, a, s, h, rec);
    }
    bool has_affinity = false;
    uint64_t rb = 0;
#pragma unroll
    for (int z = 0; z < kZ; ++z) {
      const bool rep = ns.reports(z, s);
      has_affinity |= rep;
      if (rep && (always || v[z] >= q)) rb |= 1ull << ns.id(z);
      else if (MODE == kFilterReplay && rep) short_ids |= 1ull << ns.id(z);  // (never under `always`: such a slot is not charged)
    }
    if (!(!has_affinity && host_level)) bitmask &= rb;
  }
  *numa_id = bitmask ? static_cast<uint32_t>(__builtin_ctzll(bitmask)) : 0u;
  if constexpr (MODE == kFilterReplay) *negative = ok && bitmask != 0 && ((short_ids >> *numa_id) & 1ull);
  return ok && bitmask != 0;
}

__device__ __forceinline__ double balanced_fraction(const WideNode& ns, const NrtWideArgs& a, int z, int s, int64_t q) {
  const bool is_cpu = a.slot_flags[s] & SPX_NRT_SLOT_CPU;
  const int64_t cap_v = value_of(is_cpu, avail_of(ns, a, z, s));
  return cap_v == 0 ? 1.0 : static_cast<double>(value_of(is_cpu, q)) / static_cast<double>(cap_v);
}

// one NUMA zone's strategy score over the list (least/most: least_allocated.go:25-55, most_allocated.go:25-54; balanced:
// balanced_allocation.go:27-54, the fractions in ascending slot = ascending resource id order)
template <int SG>
__device__ __forceinline__ int64_t zone_score(const WideNode& ns, const NrtWideArgs& a, int z, const WList& l, uint64_t weight_sum) {
  if constexpr (SG == kSgBalanced) {
    bool over = false;
    double sum = 0.0;
    for (int e = 0; e < l.n; ++e) {
      const double f = balanced_fraction(ns, a, z, l.slot[e], l.qty[e]);
      over |= f > 1.0;
      sum += f;
    }
    if (over) return 0;
    // gonum stat.Variance (corrected two-pass, unbiased); the fractions are recomputed rather than held
    const double mean = sum / static_cast<double>(l.n);
    double ss = 0.0, comp = 0.0;
    for (int e = 0; e < l.n; ++e) {
      const double d = balanced_fraction(ns, a, z, l.slot[e], l.qty[e]) - mean;
      ss += d * d;
      comp += d;
    }
    const double variance = (ss - comp * comp / static_cast<double>(l.n)) / (static_cast<double>(l.n) - 1.0);
    return static_cast<int64_t>((1.0 - variance) * 100.0);
  } else {
    const bool least = a.strategy == SPX_NRT_LEAST_ALLOCATED;
    uint64_t acc = 0;
    for (int e = 0; e < l.n; ++e) {
      const int s = l.slot[e];
      const bool is_cpu = a.slot_flags[s] & SPX_NRT_SLOT_CPU;
      const int64_t q = l.qty[e];
      const int64_t cap = avail_of(ns, a, z, s);
      int64_t rs = 0;
      if (cap != 0 && q <= cap) {
        const uint64_t cap_v = static_cast<uint64_t>(value_of(is_cpu, cap));
        const uint64_t req_v = static_cast<uint64_t>(value_of(is_cpu, q));
        rs = div_le100((least ? cap_v - req_v : req_v) * 100u, cap_v);
      }
      acc += static_cast<uint64_t>(rs) * static_cast<uint64_t>(a.slot_weight[s]);
    }
    if (weight_sum == 0) return 0;
    return div_le100(acc, weight_sum);
  }
}

// scoreForEachNUMANode score.go:110-124
template <int SG>
__device__ __forceinline__ int64_t score_each_numa(const WideNode& ns, const NrtWideArgs& a, const WList& l) {
  uint64_t weight_sum = 0;
  for (int e = 0; e < l.n; ++e) weight_sum += static_cast<uint64_t>(a.slot_weight[l.slot[e]]);
  int64_t min_score = 0;
#pragma unroll
  for (int z = 0; z < kZ; ++z) {
    if (z < ns.nz) {
      const int64_t s = zone_score<SG>(ns, a, z, l, weight_sum);
      if (min_score == 0 || (s != 0 && s < min_score)) min_score = s;
    }
  }
  return min_score;
}

// onlyNonNUMAResources pluginhelpers.go:163-173
__device__ __forceinline__ bool only_non_numa(const WideNode& ns, uint32_t present) {
  uint32_t any = 0;
#pragma unroll
  for (int z = 0; z < kZ; ++z) any |= z < ns.nz ? ns.zp[z] : 0u;
  return (any & present) == 0;
}

// numaNodesRequired + findSuitableCombination (least_numa.go:156-208): the chosen subset as a bitmask over LIST POSITIONS (0 = nil) and
// whether it has the minimal average distance for its size.  The first kCache requested slots with a non-zero quantity keep their
// zone quantities in registers for the subset walk; further ones (rare) are recomputed per subset.
template <int MODE>
__device__ uint32_t numa_nodes_required(const WideNode& ns, const NrtWideArgs& a, const WList& l, const Hist& h, const uint8_t (*rec)[kBlock],
                                        bool* is_min) {
  *is_min = false;
  if (ns.nz == 0) return 0;
  const uint32_t present = list_mask(l);
  int64_t cv[kCache][kZ], cq[kCache];
  int e = 0;
#pragma unroll
  for (int k = 0; k < kCache; ++k) {
    while (e < l.n && l.qty[e] == 0) ++e;
    cq[k] = 0;
    if (e < l.n) {
      cq[k] = l.qty[e];
      cur_avail<MODE>(cv[k], ns, a, l.slot[e], h, rec);
      ++e;
    } else {
#pragma unroll
      for (int z = 0; z < kZ; ++z) cv[k][z] = 0;
    }
  }
  const int e_rest = e;
  const uint8_t* masks = kCombo.mask[ns.nz - 1];
  const uint8_t* start = kCombo.start[ns.nz - 1];
  for (int k = 1; k <= ns.nz; ++k) {
    const float min_avg = a.min_avg[static_cast<int64_t>(k - 1) * a.n_nodes + ns.n];
    uint32_t best = 0;
    float min_distance = 256.0f;
    for (int ci = start[k - 1]; ci < start[k]; ++ci) {
      const uint32_t m = masks[ci];
      // isValidCombineResources: every member reports every requested name
      uint32_t all_present = ~0u;
#pragma unroll
      for (int z = 0; z < kZ; ++z) all_present &= ((m >> z) & 1u) ? ns.zp[z] : ~0u;
      if ((all_present & present) != present) continue;
      // combineResources + checkResourcesFit (Guaranteed only reaches here: isResourceSetSuitable = sum >= qty)
      bool fit = true;
#pragma unroll
      for (int kk = 0; kk < kCache; ++kk) {
        int64_t sum = 0;
#pragma unroll
        for (int z = 0; z < kZ; ++z) sum += ((m >> z) & 1u) ? cv[kk][z] : 0;
        fit &= cq[kk] == 0 || sum >= cq[kk];
      }
      for (int er = e_rest; fit && er < l.n; ++er) {
        const int64_t q = l.qty[er];
        if (q == 0) continue;
        int64_t v[kZ];
        cur_avail<MODE>(v, ns, a, l.slot[er], h, rec);
        int64_t sum = 0;
#pragma unroll
        for (int z = 0; z < kZ; ++z) sum += ((m >> z) & 1u) ? v[z] : 0;
        fit &= sum >= q;
      }
      if (!fit) continue;
      // nodesAvgDistance (float32)
      int accu = 0;
      for (int i = 0; i < ns.nz; ++i)
        if ((m >> i) & 1u)
          for (int j = 0; j < ns.nz; ++j)
            if ((m >> j) & 1u) accu += a.zone_cost[(static_cast<int64_t>(i) * kZ + j) * a.n_nodes + ns.n];
      const float distance = static_cast<float>(accu) / static_cast<float>(k * k);
      if (distance == min_avg) {
        *is_min = true;
        return m;
      }
      if (distance < min_distance) {
        min_distance = distance;
        best = m;
      }
    }
    if (best) return best;
  }
  return 0;
}

__device__ __forceinline__ uint32_t ids_of(const WideNode& ns, uint32_t pos_mask) {  // the low 8 bits: list positions < 8
  uint32_t bits = 0;
#pragma unroll
  for (int z = 0; z < kZ; ++z) {
    const uint32_t id = ns.id(z);
    if (((pos_mask >> z) & 1u) && id < 8) bits |= 1u << id;
  }
  return bits;
}

// numaNodes.Count() of a chosen subset: the distinct NUMA ids its zones carry (twins count once)
__device__ __forceinline__ int id_count(const WideNode& ns, uint32_t pos_mask) {
  uint64_t bits = 0;
#pragma unroll
  for (int z = 0; z < kZ; ++z)
    if ((pos_mask >> z) & 1u) bits |= 1ull << ns.id(z);
  return __builtin_popcountll(bits);
}

__device__ __forceinline__ WList ctr_list(const NrtWideArgs& a, int32_t c) {
  const int32_t e0 = a.ent_ptr[c];
  return WList{a.ent_slot + e0, a.ent_qty + e0, a.ent_ptr[c + 1] - e0};
}

// grid: 1-D, (pod row, group of four 64-node tiles); block = four waves of one row, wave w of block b -> tile 4 (b % groups) + w
template <int SG>
__global__ __launch_bounds__(kBlock, 2) void k_nrt_wide(NrtWideArgs a, int groups) {
  __shared__ uint8_t rec[kMaxCtrs][kBlock];  // per lane, per container of the row: its Filter charge / LeastNUMANodes subset
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t tile = static_cast<int64_t>(blockIdx.x % groups) * 4 + wave;
  const int64_t pod = a.row_begin + blockIdx.x / groups;
  if (pod >= a.row_end) return;
  const int64_t n = tile * 64 + lane;
  const bool in = n < a.n_nodes;
  if (__ballot(in) == 0) return;

  WideNode ns;
  ns.n = in ? n : 0;
  const uint32_t nflags = in ? a.flags[n] : 0u;
  ns.nz = in ? a.n_zones[n] : 0;
  ns.node_present = in ? a.node_present[n] : 0u;
  const int max_numa = in ? a.max_numa[n] : 8;
  ns.ids.lo = ns.ids.hi = 0;
#pragma unroll
  for (int z = 0; z < kZ; ++z) {
    const uint32_t idv = in ? a.zone_id[static_cast<int64_t>(z) * a.n_nodes + n] : 0u;
    ns.zp[z] = in ? a.zone_present[static_cast<int64_t>(z) * a.n_nodes + n] : 0u;
    ns.ids.set(z, idv);
  }
  const bool fresh = nflags & SPX_NRT_F_FRESH;
  const bool has_nrt = nflags & SPX_NRT_F_HAS_NRT;
  const bool single = nflags & SPX_NRT_F_SINGLE_NUMA;
  const bool pod_scope = nflags & SPX_NRT_F_POD_SCOPE;

  // ---- wave-uniform pod record
  const int qos = a.qos[pod];
  const bool non_native = a.non_native[pod] != 0;
  const int32_t r0 = a.req_ptr[pod];
  const WList preq{a.req_slot + r0, a.req_qty + r0, a.req_ptr[pod + 1] - r0};
  const int32_t c0 = a.ctr_ptr[pod];
  const int n_ctr = a.ctr_ptr[pod + 1] - c0;
  const bool non_g = qos != SPX_QOS_GUARANTEED;
  const Hist none{c0, 0, non_g};

  // ================= Filter (filter.go:179-245)
  uint32_t status = 0;
  if (!(qos == SPX_QOS_BESTEFFORT && !non_native)) {
    if (!fresh) {
      status = SPX_NRT_ST_INVALID_TOPOLOGY;
    } else if (has_nrt && single) {
      if (pod_scope) {  // singleNUMAPodLevelHandler
        uint32_t id;
        if (!fits_any<kNoReplay>(ns, a, preq, none, rec, &id)) status = SPX_NRT_ST_POD;
      } else {  // singleNUMAContainerLevelHandler
        for (int c = 0; c < n_ctr; ++c) {  // init and sidecar containers: must fit, never charged
          const int kind = a.ctr_kind[c0 + c];
          if (kind == SPX_CTR_APP) continue;
          uint32_t id;
          const bool ok = fits_any<kNoReplay>(ns, a, ctr_list(a, c0 + c), none, rec, &id);
          if (status == 0 && !ok) status = kind == SPX_CTR_SIDECAR ? SPX_NRT_ST_SIDECAR_CONTAINER : SPX_NRT_ST_INIT_CONTAINER;
        }
        for (int c = 0; c < n_ctr; ++c) {  // app containers: each charged to the NUMA id it fits before the next is tested
          if (a.ctr_kind[c0 + c] != SPX_CTR_APP) continue;
          uint32_t id;
          bool negative;
          const bool ok = fits_any<kFilterReplay>(ns, a, ctr_list(a, c0 + c), Hist{c0, c, non_g}, rec, &id, &negative);
          const bool live = status == 0;
          if (live && !ok) status = SPX_NRT_ST_CONTAINER;
          if (live && negative) status = SPX_NRT_ST_ERROR;  // ends the walk: no later container is charged on this lane
          rec[c][threadIdx.x] = static_cast<uint8_t>(live && ok ? (kApplied | id) : 0u);
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
      if (only_non_numa(ns, list_mask(preq))) {
        score = 100;
      } else {
        bool is_min;
        const uint32_t m = numa_nodes_required<kNoReplay>(ns, a, preq, none, rec, &is_min);
        score = m ? normalize_score(id_count(ns, m), is_min, max_numa) : 0;
      }
    } else {  // leastNUMAContainerScopeScore
      int max_count = 0;
      bool all_min = true, failed = false;
      for (int c = 0; c < n_ctr; ++c) {
        const WList l = ctr_list(a, c0 + c);
        uint32_t r = 0;
        if (!failed && !only_non_numa(ns, list_mask(l))) {
          bool is_min;
          const uint32_t m = numa_nodes_required<kGreedyReplay>(ns, a, l, Hist{c0, c, non_g}, rec, &is_min);
          if (!m) {
            failed = true;
          } else {
            all_min &= is_min;
            const int cnt = id_count(ns, m);
            max_count = cnt > max_count ? cnt : max_count;
            r = ids_of(ns, m);
          }
        }
        rec[c][threadIdx.x] = static_cast<uint8_t>(r);
      }
      score = failed ? 0 : (max_count == 0 ? 100 : normalize_score(max_count, all_min, max_numa));
    }
  } else if (!single) {
    score = 0;
  } else if (pod_scope) {
    score = score_each_numa<SG>(ns, a, preq);
  } else {  // containerScopeScore: int64(mean) over init + app containers
    int64_t sum = 0;
    for (int c = 0; c < n_ctr; ++c) sum += score_each_numa<SG>(ns, a, ctr_list(a, c0 + c));
    score = n_ctr > 0 ? sum / n_ctr : 0;
  }

  write_cell(a, in, pod, n, status, score);
}

}  // namespace

void launch_nrt_wide(const NrtWideArgs& a, hipStream_t s) {
  const int64_t rows = a.row_end - a.row_begin;
  if (rows <= 0 || a.n_nodes <= 0) return;
  const int groups = static_cast<int>((a.n_nodes + kBlock - 1) / kBlock);
  const unsigned blocks = static_cast<unsigned>(rows * groups);
  if (a.strategy == SPX_NRT_LEAST_NUMA_NODES)
    hipLaunchKernelGGL((k_nrt_wide<kSgLeastNuma>), dim3(blocks), dim3(kBlock), 0, s, a, groups);
  else if (a.strategy == SPX_NRT_BALANCED_ALLOCATION)
    hipLaunchKernelGGL((k_nrt_wide<kSgBalanced>), dim3(blocks), dim3(kBlock), 0, s, a, groups);
  else
    hipLaunchKernelGGL((k_nrt_wide<kSgAlloc>), dim3(blocks), dim3(kBlock), 0, s, a, groups);
}

}  // namespace spx
