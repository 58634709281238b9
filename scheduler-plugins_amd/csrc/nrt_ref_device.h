// nrt_ref_device.h — NodeResourceTopologyMatch in the reference's own int64 arithmetic: the one copy of the device code that
// kernels_nrt.hip (k_nrt), kernels_nrt_long.hip (k_nrt_long) and kernels_nrt_wide.hip (k_nrt_wide) evaluate Filter and Score
// with, and that every fast form is tested against.
//
// The two dense kernels share every helper over the node record (a lane's NUMA table in VGPRs); what is theirs is the grid, the
// source of a pod's containers and the Filter / Score ladder over them.  The wide kernel walks sparse request lists
// and takes what does not depend on the node record: the subset table, div_le100, value_of, normalize_score, the packed NUMA
// ids, the strategy groups and write_cell.
//
// k_nrt's machine code is what the committed profiles are stamped with (build.device_code_hash), and gfx950 code generation is
// sensitive to how this code is cut: moving k_nrt's node load, its Filter / Score ladder or its cell write into a function here
// changes its registers and block layout, and so does taking the node's flags and max_numa out of its record, while putting
// them into k_nrt_long's record grows that kernel's scratch.  So the ladders stay in the two kernels, k_nrt writes its cell
// itself, and the helpers take the record type as a parameter: NodeState below, or k_nrt's with the two members more.
//
// Everything is in the anonymous namespace: each translation unit gets its own copy, the __constant__ table included.
//
// Reference: pkg/noderesourcetopology/filter.go:42-258, score.go:62-191, least_numa.go:35-233, least_allocated.go,
// most_allocated.go, balanced_allocation.go, numaresources.go:105-215.
#pragma once

#include "spx_internal.h"

namespace spx {

namespace {

constexpr int kZ = SPX_NRT_MAX_ZONES;
// strategy groups (one kernel instantiation each, so that a launch carries only the code it runs)
constexpr int kSgAlloc = 0;      // LeastAllocated / MostAllocated
constexpr int kSgBalanced = 1;   // BalancedAllocation
constexpr int kSgLeastNuma = 2;  // LeastNUMANodes

constexpr int strategy_group(int strategy) {
  return strategy == SPX_NRT_LEAST_NUMA_NODES ? kSgLeastNuma : (strategy == SPX_NRT_BALANCED_ALLOCATION ? kSgBalanced : kSgAlloc);
}

// combin.Combinations(n, k) for n <= 8 as bitmasks over list positions, size-major then lexicographic
struct ComboTable {
  uint8_t mask[kZ][256];
  uint8_t start[kZ][kZ + 2];  // start[n-1][k-1] .. start[n-1][k]: subsets of size k
};

constexpr ComboTable make_combos() {
  ComboTable t{};
  for (int n = 1; n <= kZ; ++n) {
    int idx = 0;
    for (int k = 1; k <= n; ++k) {
      t.start[n - 1][k - 1] = static_cast<uint8_t>(idx);
      idx += nrt_combinations(n, k, t.mask[n - 1] + idx);
    }
    t.start[n - 1][n] = static_cast<uint8_t>(idx);  // 255 for n == 8
  }
  return t;
}

__constant__ ComboTable kCombo = make_combos();

static_assert(make_combos().mask[7][254] == make_combo8().mask[254] && make_combos().start[7][8] == make_combo8().start[8],
              "Combo8 is row n = 8 of the table");

// floor(num / den) for 0 <= num <= 101 * den (quotient <= 101): float estimate + exact fix-up (a 64-bit integer division per
// zone, resource and container would dominate the launch)
__device__ __forceinline__ int64_t div_le100(uint64_t num, uint64_t den) {
  const float qf = static_cast<float>(num) * __frcp_rn(static_cast<float>(den));
  uint64_t q = static_cast<uint64_t>(static_cast<uint32_t>(qf));
  const uint64_t prod = q * den;
  if (prod > num) --q;
  else if (num - prod >= den) ++q;
  return static_cast<int64_t>(q);
}

__device__ __forceinline__ int64_t value_of(bool is_cpu, int64_t q) {  // Quantity.Value(): cpu is in millicores
  return is_cpu ? (q + 999) / 1000 : q;
}

__device__ __forceinline__ int64_t normalize_score(int count, bool is_min, int max_numa) {  // least_numa.go:90-100
  const int64_t numa_node_score = 100 / static_cast<int64_t>(max_numa);
  const int64_t score = 100 - static_cast<int64_t>(count) * numa_node_score;
  return is_min ? score + numa_node_score / 2 : score;
}

// the write of one cell: the raw int64 Score() row of the parity harness, or the status and the clamped score
template <class A>
__device__ __forceinline__ void write_cell(const A& a, bool in, int64_t pod, int64_t n, uint32_t status, int64_t score) {
  if (in && a.out_raw != nullptr) {
    a.out_raw[n] = score;
  } else if (in) {
    const int64_t cell = pod * a.row_stride + n;
    a.out_status[cell] = static_cast<uint8_t>(status);
    score = score < 0 ? 0 : (score > 255 ? 255 : score);
    a.out_score[cell] = static_cast<uint8_t>(score);
  }
}

// ---------------------------------------------------------------- the dense node record and the helpers over it
// A = the kernel's argument struct (NrtArgs, NrtLongArgs): read for n_res, slot_flags, slot_weight, strategy, n_nodes and the
// node columns only.  N = NodeState, or k_nrt's record of the same members with two more between them (kernels_nrt.hip).

// NUMA id per list position, 8 bits each
struct ZoneIds {
  uint32_t lo, hi;
  __device__ __forceinline__ uint32_t id(int z) const { return ((z < 4 ? lo >> (8 * z) : hi >> (8 * (z - 4))) & 0xffu); }
  __device__ __forceinline__ void set(int z, uint32_t v) {  // on a zeroed pair
    if (z < 4) lo |= v << (8 * z);
    else hi |= v << (8 * (z - 4));
  }
};

template <int RM>
struct NodeState {
  int64_t avail[kZ][RM];
  ZoneIds ids;
  uint32_t zp_lo, zp_hi;  // per-zone resource-presence bitmask, 8 bits each
  int nz;
  uint32_t node_present;
  __device__ __forceinline__ uint32_t id(int z) const { return ids.id(z); }
  __device__ __forceinline__ uint32_t zp(int z) const { return ((z < 4 ? zp_lo >> (8 * z) : zp_hi >> (8 * (z - 4))) & 0xffu); }
};

template <int RM, template <int> class N, class A>
__device__ __forceinline__ void load_avail(N<RM>& ns, const A& a, int64_t n, bool in) {
#pragma unroll
  for (int z = 0; z < kZ; ++z)
#pragma unroll
    for (int r = 0; r < RM; ++r)
      ns.avail[z][r] = (in && r < a.n_res) ? a.zone_avail[(static_cast<int64_t>(z) * a.n_res + r) * a.n_nodes + n] : 0;
}

// resourcesAvailableInAnyNUMANodes filter.go:93-163.  req/present are wave-uniform.
// negative (asked for by the app containers' walk only): charging the request to the id it fits — which
// subtractResourcesFromNUMANodeList does to EVERY zone that carries the id — would leave one of them below zero: a twin of the zone
// that fits reports the resource and holds less than the quantity.  The reference stops there with an error (numaresources.go:172-175)
// that filter.go:73-77 turns into fwk.Error; the caller ends the row with SPX_NRT_ST_ERROR.  The test reads the quantities the fit
// is decided on, in the loop that decides it: folded into the charge loop (adjust_numa) it cost k_nrt scratch, here it costs none.
template <int RM, template <int> class N, class A>
__device__ __forceinline__ bool fits_any(const N<RM>& ns, const A& a, bool non_guaranteed, uint32_t present,
                                         const int64_t* __restrict__ req, uint32_t* numa_id, bool* negative = nullptr) {
  uint64_t bitmask = ~0ull;
  uint64_t short_ids = 0;  // ids of reporting zones that hold less than a quantity the charge takes
  bool ok = true;
#pragma unroll
  for (int r = 0; r < RM; ++r) {
    if (r >= a.n_res || !((present >> r) & 1u)) continue;  // uniform
    const int64_t q = req[r];
    if (q == 0) continue;                                   // uniform: "ignoring zero-qty resource request"
    const bool always = non_guaranteed && (a.slot_flags[r] & SPX_NRT_SLOT_AFFINE);  // isResourceSetSuitable, uniform
    const bool host_level = a.slot_flags[r] & SPX_NRT_SLOT_HOST_LEVEL;
    if (!((ns.node_present >> r) & 1u)) ok = false;  // not reported at node level -> cannot meet request
    bool has_affinity = false;
    uint64_t rb = 0;
#pragma unroll
    for (int z = 0; z < kZ; ++z) {
      const bool rep = z < ns.nz && ((ns.zp(z) >> r) & 1u);
      has_affinity |= rep;
      if (rep && (always || ns.avail[z][r] >= q)) rb |= 1ull << ns.id(z);
      else if (negative && rep) short_ids |= 1ull << ns.id(z);  // (never under `always`: such a slot is not charged)
    }
    if (!(!has_affinity && host_level)) bitmask &= rb;
  }
  *numa_id = bitmask ? static_cast<uint32_t>(__builtin_ctzll(bitmask)) : 0u;
  if (negative) *negative = ok && bitmask != 0 && ((short_ids >> *numa_id) & 1ull);
  return ok && bitmask != 0;
}

// subtractResourcesFromNUMANodeList numaresources.go:145-182 (sign = -1) and its exact inverse (+1).  Every zone that carries the id
// is charged, also where fits_any reports that one of them goes below zero: the whole charge is applied, so that the inverse
// restores the table whatever the outcome.
template <int RM, template <int> class N, class A>
__device__ __forceinline__ void adjust_numa(N<RM>& ns, const A& a, bool non_guaranteed, uint32_t present,
                                            const int64_t* __restrict__ req, uint32_t numa_id, bool apply, int sign) {
#pragma unroll
  for (int r = 0; r < RM; ++r) {
    if (r >= a.n_res || !((present >> r) & 1u)) continue;
    if (non_guaranteed && (a.slot_flags[r] & SPX_NRT_SLOT_AFFINE)) continue;
    const int64_t q = req[r];
    if (q == 0) continue;
#pragma unroll
    for (int z = 0; z < kZ; ++z) {
      const bool hit = apply && z < ns.nz && ns.id(z) == numa_id && ((ns.zp(z) >> r) & 1u);
      ns.avail[z][r] += hit ? sign * q : 0;
    }
  }
}

// one NUMA zone's strategy score (least/most: least_allocated.go:25-55, most_allocated.go:25-54;
// balanced: balanced_allocation.go:27-54); zero when the request set is empty (the reference panics)
template <int RM, int SG, template <int> class N, class A>
__device__ __forceinline__ int64_t zone_score(const N<RM>& ns, const A& a, int z, uint32_t present,
                                              const int64_t* __restrict__ req, uint64_t weight_sum) {
  if constexpr (SG == kSgBalanced) {
    double fr[RM];
    bool over = false;
    int n = 0;
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      fr[r] = 0.0;
      if (r >= a.n_res || !((present >> r) & 1u)) continue;
      const bool is_cpu = a.slot_flags[r] & SPX_NRT_SLOT_CPU;
      const int64_t cap = ((ns.zp(z) >> r) & 1u) ? ns.avail[z][r] : 0;
      const int64_t cap_v = value_of(is_cpu, cap);
      const double f = cap_v == 0 ? 1.0 : static_cast<double>(value_of(is_cpu, req[r])) / static_cast<double>(cap_v);
      over |= f > 1.0;
      fr[r] = f;
      ++n;
    }
    if (over) return 0;
    // gonum stat.Variance (corrected two-pass, unbiased), fractions taken in ascending resource id
    double sum = 0.0;
#pragma unroll
    for (int r = 0; r < RM; ++r) sum += fr[r];  // absent slots hold +0.0: x + 0.0 == x
    const double mean = sum / static_cast<double>(n);
    double ss = 0.0, comp = 0.0;
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      const bool used = r < a.n_res && ((present >> r) & 1u);
      const double d = used ? fr[r] - mean : 0.0;
      ss += d * d;
      comp += d;
    }
    const double variance = (ss - comp * comp / static_cast<double>(n)) / (static_cast<double>(n) - 1.0);
    return static_cast<int64_t>((1.0 - variance) * 100.0);
  } else {
    const bool least = a.strategy == SPX_NRT_LEAST_ALLOCATED;
    uint64_t acc = 0;
#pragma unroll
    for (int r = 0; r < RM; ++r) {
      if (r >= a.n_res || !((present >> r) & 1u)) continue;
      const bool is_cpu = a.slot_flags[r] & SPX_NRT_SLOT_CPU;
      const int64_t q = req[r];
      const int64_t cap = ((ns.zp(z) >> r) & 1u) ? ns.avail[z][r] : 0;
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
template <int RM, int SG, template <int> class N, class A>
__device__ __forceinline__ int64_t score_each_numa(const N<RM>& ns, const A& a, uint32_t present,
                                                   const int64_t* __restrict__ req) {
  uint64_t weight_sum = 0;
#pragma unroll
  for (int r = 0; r < RM; ++r)
    if (r < a.n_res && ((present >> r) & 1u)) weight_sum += static_cast<uint64_t>(a.slot_weight[r]);
  int64_t min_score = 0;
#pragma unroll
  for (int z = 0; z < kZ; ++z) {
    if (z < ns.nz) {
      const int64_t s = zone_score<RM, SG>(ns, a, z, present, req, weight_sum);
      if (min_score == 0 || (s != 0 && s < min_score)) min_score = s;
    }
  }
  return min_score;
}

// ---------------------------------------------------------------- LeastNUMANodes (least_numa.go)

// onlyNonNUMAResources pluginhelpers.go:163-173
template <int RM, template <int> class N>
__device__ __forceinline__ bool only_non_numa(const N<RM>& ns, uint32_t present) {
  uint32_t any = 0;
#pragma unroll
  for (int z = 0; z < kZ; ++z) any |= z < ns.nz ? ns.zp(z) : 0u;
  return (any & present) == 0;
}

// numaNodesRequired + findSuitableCombination (least_numa.go:156-208): returns the chosen subset as a
// bitmask over LIST POSITIONS (0 = nil) and whether it has the minimal average distance for its size
template <int RM, template <int> class N, class A>
__device__ uint32_t numa_nodes_required(const N<RM>& ns, const A& a, int64_t n, uint32_t present,
                                        const int64_t* __restrict__ req, bool* is_min) {
  *is_min = false;
  if (ns.nz == 0) return 0;
  const uint8_t* masks = kCombo.mask[ns.nz - 1];
  const uint8_t* start = kCombo.start[ns.nz - 1];
  for (int k = 1; k <= ns.nz; ++k) {
    const float min_avg = a.min_avg[static_cast<int64_t>(k - 1) * a.n_nodes + n];
    uint32_t best = 0;
    float min_distance = 256.0f;
    for (int ci = start[k - 1]; ci < start[k]; ++ci) {
      const uint32_t m = masks[ci];
      // isValidCombineResources: every member reports every requested name
      uint32_t all_present = 0xffu;
#pragma unroll
      for (int z = 0; z < kZ; ++z) all_present &= ((m >> z) & 1u) ? ns.zp(z) : 0xffu;
      if ((all_present & present) != present) continue;
      // combineResources + checkResourcesFit (Guaranteed only reaches here: isResourceSetSuitable = sum >= qty)
      bool fit = true;
#pragma unroll
      for (int r = 0; r < RM; ++r) {
        if (r >= a.n_res || !((present >> r) & 1u)) continue;
        const int64_t q = req[r];
        if (q == 0) continue;
        int64_t sum = 0;
#pragma unroll
        for (int z = 0; z < kZ; ++z) sum += ((m >> z) & 1u) ? ns.avail[z][r] : 0;
        fit &= sum >= q;
      }
      if (!fit) continue;
      // nodesAvgDistance (float32)
      int accu = 0;
      for (int i = 0; i < ns.nz; ++i)
        if ((m >> i) & 1u)
          for (int j = 0; j < ns.nz; ++j)
            if ((m >> j) & 1u) accu += a.zone_cost[(static_cast<int64_t>(i) * kZ + j) * a.n_nodes + n];
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

// subtractFromNUMAs numaresources.go:184-215: the bitmask holds NUMA ids but indexes list positions (appendix B.1)
template <int RM, template <int> class N, class A>
__device__ __forceinline__ void subtract_from_numas(N<RM>& ns, const A& a, uint32_t present,
                                                    const int64_t* __restrict__ req, uint64_t id_bits) {
#pragma unroll
  for (int r = 0; r < RM; ++r) {
    if (r >= a.n_res || !((present >> r) & 1u)) continue;
    int64_t quantity = req[r];
#pragma unroll
    for (int z = 0; z < kZ; ++z) {  // positions >= nz cannot hold resources; ids >= 8 would index out of range in the reference
      const bool member = ((id_bits >> z) & 1ull) && z < ns.nz && ((ns.zp(z) >> r) & 1u) && quantity != 0;
      const int64_t available = ns.avail[z][r];
      const int64_t take = quantity >= available ? available : quantity;
      ns.avail[z][r] = member ? available - take : available;
      quantity = member ? quantity - take : quantity;
    }
  }
}

template <int RM, template <int> class N>
__device__ __forceinline__ uint64_t ids_of(const N<RM>& ns, uint32_t pos_mask) {
  uint64_t bits = 0;
#pragma unroll
  for (int z = 0; z < kZ; ++z)
    if ((pos_mask >> z) & 1u) bits |= 1ull << ns.id(z);
  return bits;
}

}  // namespace

}  // namespace spx
