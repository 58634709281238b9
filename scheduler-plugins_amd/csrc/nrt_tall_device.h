// nrt_tall_device.h — what kernels_nrt_tall.hip needs beyond nrt_ref_device.h: NodeResourceTopologyMatch over a node whose NUMA
// table does not fit a lane's registers (9 to 64 zones; 64 zones x 8 slots of int64 would be 1 024 VGPRs).
//
// The node record stays in memory.  A lane names its node by the compacted index t into the tall side table (spx_nrt_tall_nodes,
// node-major on the device: element e of node t at [e * n_tall + t], so the 64 lanes of a wave read consecutive addresses), and
// reads the zone quantities through an AvView: the side table itself, or the wave's working copy ([e * 64 + lane]) once a container
// has been charged to a zone.  Everything that does not depend on the record (div_le100, value_of, normalize_score, the strategy
// groups, write_cell) is nrt_ref_device.h's; the walks below restate its helpers over the record with loops bounded by the node's
// zone count instead of unrolled over 8 positions.
//
// Reference: pkg/noderesourcetopology/filter.go:93-163, numaresources.go:145-215, score.go:110-124, least_numa.go:102-233.
#pragma once

#include "nrt_ref_device.h"

namespace spx {

namespace {

constexpr int kTallR = SPX_NRT_MAX_RES;

// a lane's node: index into the side table, zone count, node-level key set
struct TallNode {
  int64_t t;
  int nz;
  uint32_t node_present;
};

// zone quantities of one node: element (z, r) at p[(z * n_res + r) * stride]
struct AvView {
  const int64_t* p;
  int64_t stride;
  __device__ __forceinline__ int64_t at(int z, int r, int R) const { return p[(static_cast<int64_t>(z) * R + r) * stride]; }
};

template <class A>
__device__ __forceinline__ uint32_t tall_id(const A& a, const TallNode& nd, int z) {
  return a.zone_id[static_cast<int64_t>(z) * a.n_tall + nd.t];
}
template <class A>
__device__ __forceinline__ uint32_t tall_zp(const A& a, const TallNode& nd, int z) {
  return a.zone_present[static_cast<int64_t>(z) * a.n_tall + nd.t];
}

// resourcesAvailableInAnyNUMANodes filter.go:93-163 (ids 0..63: the shift is at most 63 whatever the zone count)
template <class A>
__device__ bool tall_fits_any(const A& a, const TallNode& nd, const AvView& av, bool non_guaranteed, uint32_t present,
                              const int64_t* __restrict__ req, uint32_t* numa_id) {
  const int R = a.n_res;
  uint64_t bitmask = ~0ull;
  bool ok = true;
  for (int r = 0; r < R; ++r) {
    if (!((present >> r) & 1u)) continue;
    const int64_t q = req[r];
    if (q == 0) continue;
    const bool always = non_guaranteed && (a.slot_flags[r] & SPX_NRT_SLOT_AFFINE);
    const bool host_level = a.slot_flags[r] & SPX_NRT_SLOT_HOST_LEVEL;
    if (!((nd.node_present >> r) & 1u)) ok = false;
    bool has_affinity = false;
    uint64_t rb = 0;
    for (int z = 0; z < nd.nz; ++z) {
      if (!((tall_zp(a, nd, z) >> r) & 1u)) continue;
      has_affinity = true;
      if (always || av.at(z, r, R) >= q) rb |= 1ull << (tall_id(a, nd, z) & 63u);
    }
    if (!(!has_affinity && host_level)) bitmask &= rb;
  }
  *numa_id = bitmask ? static_cast<uint32_t>(__builtin_ctzll(bitmask)) : 0u;
  return ok && bitmask != 0;
}

// Where the reference returns fwk.Error instead of Unschedulable the Filter's status cell holds SPX_NRT_ST_ERROR (spx.h: the oracle's
// -1 as a byte; the value NetworkOverhead's PreFilter error travels as).

// subtractResourcesFromNUMANodeList numaresources.go:145-182 on the wave's working copy: every zone that carries the id is charged.
// False when a charge leaves a zone below zero — two zones share the id and only one of them holds the request; the reference stops
// there with "inconsistent resource accounting" (numaresources.go:172-175, filter.go:73-77)
template <class A>
__device__ bool tall_charge(const A& a, const TallNode& nd, int64_t* work, bool non_guaranteed, uint32_t present,
                            const int64_t* __restrict__ req, uint32_t numa_id) {
  const int R = a.n_res;
  bool ok = true;
  for (int z = 0; z < nd.nz; ++z) {
    if (tall_id(a, nd, z) != numa_id) continue;
    const uint32_t zp = tall_zp(a, nd, z);
    for (int r = 0; r < R; ++r) {
      if (!((present >> r) & 1u) || !((zp >> r) & 1u)) continue;
      if (non_guaranteed && (a.slot_flags[r] & SPX_NRT_SLOT_AFFINE)) continue;
      const int64_t q = req[r];
      if (q == 0) continue;
      int64_t* cell = work + (static_cast<int64_t>(z) * R + r) * 64;
      const int64_t left = *cell - q;
      ok &= left >= 0;
      *cell = left;
    }
  }
  return ok;
}

// one zone's strategy score, as nrt_ref_device.h's zone_score
template <int SG, class A>
__device__ int64_t tall_zone_score(const A& a, const TallNode& nd, const AvView& av, int z, uint32_t present,
                                   const int64_t* __restrict__ req, uint64_t weight_sum) {
  const int R = a.n_res;
  const uint32_t zp = tall_zp(a, nd, z);
  if constexpr (SG == kSgBalanced) {
    double fr[kTallR];
    bool over = false;
    int n = 0;
#pragma unroll
    for (int r = 0; r < kTallR; ++r) {
      fr[r] = 0.0;
      if (r >= R || !((present >> r) & 1u)) continue;
      const bool is_cpu = a.slot_flags[r] & SPX_NRT_SLOT_CPU;
      const int64_t cap = ((zp >> r) & 1u) ? av.at(z, r, R) : 0;
      const int64_t cap_v = value_of(is_cpu, cap);
      const double f = cap_v == 0 ? 1.0 : static_cast<double>(value_of(is_cpu, req[r])) / static_cast<double>(cap_v);
      over |= f > 1.0;
      fr[r] = f;
      ++n;
    }
    if (over) return 0;
    double sum = 0.0;
#pragma unroll
    for (int r = 0; r < kTallR; ++r) sum += fr[r];
    const double mean = sum / static_cast<double>(n);
    double ss = 0.0, comp = 0.0;
#pragma unroll
    for (int r = 0; r < kTallR; ++r) {
      const bool used = r < R && ((present >> r) & 1u);
      const double d = used ? fr[r] - mean : 0.0;
      ss += d * d;
      comp += d;
    }
    const double variance = (ss - comp * comp / static_cast<double>(n)) / (static_cast<double>(n) - 1.0);
    return static_cast<int64_t>((1.0 - variance) * 100.0);
  } else {
    const bool least = a.strategy == SPX_NRT_LEAST_ALLOCATED;
    uint64_t acc = 0;
    for (int r = 0; r < R; ++r) {
      if (!((present >> r) & 1u)) continue;
      const bool is_cpu = a.slot_flags[r] & SPX_NRT_SLOT_CPU;
      const int64_t q = req[r];
      const int64_t cap = ((zp >> r) & 1u) ? av.at(z, r, R) : 0;
      int64_t rs = 0;
      if (cap != 0 && q <= cap) {
        const uint64_t cap_v = static_cast<uint64_t>(value_of(is_cpu, cap));
        const uint64_t req_v = static_cast<uint64_t>(value_of(is_cpu, q));
        rs = div_le100((least ? cap_v - req_v : req_v) * 100u, cap_v);
      }
      acc += static_cast<uint64_t>(rs) * static_cast<uint64_t>(a.slot_weight[r]);
    }
    if (weight_sum == 0) return 0;
    return div_le100(acc, weight_sum);
  }
}

// scoreForEachNUMANode score.go:110-124
template <int SG, class A>
__device__ int64_t tall_score_each_numa(const A& a, const TallNode& nd, const AvView& av, uint32_t present,
                                        const int64_t* __restrict__ req) {
  uint64_t weight_sum = 0;
  for (int r = 0; r < a.n_res; ++r)
    if ((present >> r) & 1u) weight_sum += static_cast<uint64_t>(a.slot_weight[r]);
  int64_t min_score = 0;
  for (int z = 0; z < nd.nz; ++z) {
    const int64_t s = tall_zone_score<SG>(a, nd, av, z, present, req, weight_sum);
    if (min_score == 0 || (s != 0 && s < min_score)) min_score = s;
  }
  return min_score;
}

// onlyNonNUMAResources pluginhelpers.go:163-173
template <class A>
__device__ bool tall_only_non_numa(const A& a, const TallNode& nd, uint32_t present) {
  uint32_t any = 0;
  for (int z = 0; z < nd.nz; ++z) any |= tall_zp(a, nd, z);
  return (any & present) == 0;
}

// numaNodesRequired + findSuitableCombination (least_numa.go:156-208) for 9 to 16 zones: the chosen subset as a bitmask over list
// positions (0 = nil) and whether it has the minimal average distance for its size.  Subsets come from the host-built table
// (size-major, lexicographic over positions: combin.Combinations' order).  Two exact short cuts, taken only while every quantity
// in play is non-negative: a subset can hold only zones that report every requested name (isValidCombineResources), so when the
// sum over those zones misses a request no subset fits; and k zones hold at most k times the largest of them, so sizes below
// ceil(request / largest) have no fitting subset and are skipped.
template <class A>
__device__ uint32_t tall_numa_nodes_required(const A& a, const TallNode& nd, const AvView& av, uint32_t present,
                                             const int64_t* __restrict__ req, bool* is_min) {
  *is_min = false;
  const int R = a.n_res;
  const int nz = nd.nz;
  if (nz < 9 || nz > SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA) return 0;  // (the engine refuses such a node with this strategy)
  uint32_t valid = 0;
  for (int z = 0; z < nz; ++z)
    if ((tall_zp(a, nd, z) & present) == present) valid |= 1u << z;
  if (!valid) return 0;
  int kmin = 1;
  for (int r = 0; r < R; ++r) {
    if (!((present >> r) & 1u)) continue;
    const int64_t q = req[r];
    if (q <= 0) continue;
    int64_t sum = 0, most = 0;
    bool negative = false;
    for (uint32_t m = valid; m; m &= m - 1) {
      const int64_t v = av.at(__builtin_ctz(m), r, R);
      negative |= v < 0;
      sum += v;
      most = v > most ? v : most;
    }
    if (negative) continue;
    if (sum < q) return 0;
    const int64_t need = q / most + (q % most != 0 ? 1 : 0);  // (most > 0: the sum of non-negative values reached q > 0)
    if (need > kmin) kmin = need > nz ? nz : static_cast<int>(need);
  }
  const uint32_t* start = a.combo_start + (nz - 9) * (SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA + 1);
  const int64_t T = a.n_tall, zs = a.zone_stride;
  for (int k = kmin; k <= nz; ++k) {
    const float min_avg = a.min_avg[static_cast<int64_t>(k - 1) * T + nd.t];
    uint32_t best = 0;
    float min_distance = 256.0f;
    for (uint32_t ci = start[k - 1]; ci < start[k]; ++ci) {
      const uint32_t m = a.combo_mask[ci];
      if (m & ~valid) continue;
      bool fit = true;
      for (int r = 0; r < R && fit; ++r) {
        if (!((present >> r) & 1u)) continue;
        const int64_t q = req[r];
        if (q == 0) continue;
        int64_t sum = 0;
        for (uint32_t b = m; b; b &= b - 1) sum += av.at(__builtin_ctz(b), r, R);
        fit = sum >= q;
      }
      if (!fit) continue;
      int accu = 0;
      for (uint32_t bi = m; bi; bi &= bi - 1) {
        const int64_t i = __builtin_ctz(bi);
        for (uint32_t bj = m; bj; bj &= bj - 1) accu += a.zone_cost[(i * zs + __builtin_ctz(bj)) * T + nd.t];
      }
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

template <class A>
__device__ uint64_t tall_ids_of(const A& a, const TallNode& nd, uint32_t pos_mask) {
  uint64_t bits = 0;
  for (uint32_t m = pos_mask; m; m &= m - 1) bits |= 1ull << (tall_id(a, nd, __builtin_ctz(m)) & 63u);
  return bits;
}

// subtractFromNUMAs numaresources.go:184-215 on the working copy: the bitmask holds NUMA ids but indexes list positions
// (appendix B.1); a position at or beyond the node's zone count is skipped, as the oracle does
template <class A>
__device__ void tall_subtract_from_numas(const A& a, const TallNode& nd, int64_t* work, uint32_t present,
                                         const int64_t* __restrict__ req, uint64_t id_bits) {
  const int R = a.n_res;
  for (int r = 0; r < R; ++r) {
    if (!((present >> r) & 1u)) continue;
    int64_t quantity = req[r];
    for (uint64_t m = id_bits; m && quantity != 0; m &= m - 1) {
      const int pos = __builtin_ctzll(m);
      if (pos >= nd.nz || !((tall_zp(a, nd, pos) >> r) & 1u)) continue;
      int64_t* cell = work + (static_cast<int64_t>(pos) * R + r) * 64;
      const int64_t available = *cell;
      if (quantity >= available) {
        quantity -= available;
        *cell = 0;
      } else {
        *cell = available - quantity;
        quantity = 0;
      }
    }
  }
}

}  // namespace

}  // namespace spx
