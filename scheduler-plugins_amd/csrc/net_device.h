// net_device.h — NetworkOverhead's per-pair arithmetic and the per-node kernel, once for both accumulator widths.
//
// kernels_network.hip instantiates everything here with T = int (cost entries and a node's accumulated cost fit 31 bits: the
// engine checks (largest entry) x (most pairs of a workload key) < 2^31), kernels_network_wide.hip with T = int64_t (the reference's
// own width, networkoverhead.go:576-638).  What differs between the two beyond the type:
//   - the cost matrices are read as NetArgs::region_cost / zone_cost or as NetArgs::region_cost64 / zone_cost64;
//   - NormalizeScore (net_norm.h): the narrow form replaces int64(100.0*float64(d)/float64(r)) by integer division while 100*d
//     fits 32 bits (r < 2^31/100) and runs the reference's float64 sequence above that; the quotients are equal for every r < 2^31.
//     The wide form always runs the float64 sequence (norm_cost_f64).
//
// Everything is in the anonymous namespace: each translation unit gets its own copy.
#pragma once

#include <limits>

#include "net_norm.h"
#include "spx_internal.h"

namespace spx {

namespace {

constexpr int kNpl = 4;  // nodes per lane
constexpr int kSameZone = SPX_NET_SAME_ZONE;
constexpr int kMaxCost = SPX_NET_MAX_COST;

template <typename T>
struct AccT {
  int sat, vio;
  T cost;
};

template <typename T>
__device__ __forceinline__ const T* zone_costs(const NetArgs& g) {
  if constexpr (sizeof(T) == 8) return g.zone_cost64;
  else return g.zone_cost;
}
template <typename T>
__device__ __forceinline__ const T* region_costs(const NetArgs& g) {
  if constexpr (sizeof(T) == 8) return g.region_cost64;
  else return g.region_cost;
}

// contribution of one (scheduled pod on `host`, dependency with `max_cost`) pair to a node with labels
// (region, zone) that is NOT the host — checkMaxNetworkCostRequirements :536-567 + getAccumulatedCost :605-633
template <typename T>
__device__ __forceinline__ void add_pair(AccT<T>& a, const NetArgs& g, int region, int zone, int host_region, int host_zone, int64_t max_cost) {
  if (host_region < 0 && host_zone < 0) {  // placed node carries neither label
    a.vio += 1;
    a.cost += kMaxCost;
  } else if (region == host_region) {
    if (zone == host_zone) {
      a.sat += 1;
      a.cost += kSameZone;
    } else {
      const T c = (zone >= 0 && host_zone >= 0) ? zone_costs<T>(g)[static_cast<int64_t>(zone) * g.n_zones + host_zone] : -1;
      if (c >= 0) {
        if (c <= max_cost) a.sat += 1;
        else a.vio += 1;
        a.cost += c;
      } else {
        a.cost += kMaxCost;  // missing entry: not counted, but charged MaxCost
      }
    }
  } else {
    const T c = (region >= 0 && host_region >= 0) ? region_costs<T>(g)[static_cast<int64_t>(region) * g.n_regions + host_region] : -1;
    if (c >= 0) {
      if (c <= max_cost) a.sat += 1;
      else a.vio += 1;
      a.cost += c;
    } else {
      a.cost += kMaxCost;
    }
  }
}

// exact per-pair evaluation of one node (host nodes; snapshots without a class table)
template <typename T>
__device__ AccT<T> direct_eval(const NetArgs& g, int64_t node, int lo, int hi) {
  AccT<T> a{0, 0, 0};
  const int region = g.region[node], zone = g.zone[node];
  for (int i = lo; i < hi; ++i) {
    const int host = g.pair_node[i];
    if (host == node) {
      a.sat += 1;  // same hostname: satisfied, cost 0
      continue;
    }
    add_pair(a, g, region, zone, g.region[host], g.zone[host], g.pair_max[i]);
  }
  return a;
}

// the same over a pair list staged in LDS (host, its region and zone, MaxNetworkCost): the single-row launch of the sequential
// commit loop has one workgroup and nothing to hide the two dependent global loads per pair behind (25 us per pod at 20k nodes)
struct StagedPairs {
  const int* host;
  const int* region;
  const int* zone;
  const long long* max_cost;
  int n;
};
template <typename T>
__device__ AccT<T> direct_eval_staged(const NetArgs& g, int64_t node, const StagedPairs& sp) {
  AccT<T> a{0, 0, 0};
  const int region = g.region[node], zone = g.zone[node];
  for (int i = 0; i < sp.n; ++i) {
    if (sp.host[i] == node) {
      a.sat += 1;
      continue;
    }
    add_pair(a, g, region, zone, sp.region[i], sp.zone[i], sp.max_cost[i]);
  }
  return a;
}

template <typename T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const T o = __shfl_xor(v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const T o = __shfl_xor(v, m, 64);
    v = o > v ? o : v;
  }
  return v;
}

// NormalizeScore: norm_cost (T = int) and norm_cost_f64 (T = int64_t), net_norm.h

// One wavefront per pod row, every node evaluated on its own:
//   phase 1  lanes = topology classes: accumulate (satisfied, violated, cost) over the pod's pairs into LDS;
//   phase 2  mark the (<= pairs) host nodes in an LDS bitmap;
//   phase 3  lanes = nodes, 4 consecutive nodes per lane: class lookup from LDS (host nodes and class-less
//            snapshots take the exact per-pair path), Filter = violated > satisfied, wave min/max of the
//            cost over feasible nodes;
//   phase 4  same sweep again, now normalising (100 - 100*(s-min)/(max-min)) and storing one dword of
//            status bytes and one dword of score bytes per lane (256 contiguous bytes per wave per table).
// Dynamic LDS: T = int: 3 ints per class; T = int64_t: the 64-bit costs first, then satisfied and violated (4 ints per class);
// the host bitmap behind them.
template <typename T>
__global__ __launch_bounds__(64) void k_net(NetArgs g) {
  using Acc = AccT<T>;
  constexpr bool kWide = sizeof(T) == 8;
  SPX_RESOLVE_ROWS(g);
  extern __shared__ __align__(16) int lds[];
  int* cls_sat = kWide ? lds + 2 * g.n_classes : lds;
  int* cls_vio = kWide ? lds + 3 * g.n_classes : lds + g.n_classes;
  T* cls_cost = kWide ? reinterpret_cast<T*>(lds) : reinterpret_cast<T*>(lds + 2 * g.n_classes);
  unsigned* host_bits = reinterpret_cast<unsigned*>(lds + (kWide ? 4 : 3) * g.n_classes);
  const int lane = threadIdx.x;
  const int64_t pod = g.row_begin + blockIdx.x;
  if (pod >= g.row_end) return;
  const int key = g.pod_key[pod];
  const int flag = g.key_flag[key];
  const int lo = g.pair_ptr[key], hi = g.pair_end ? g.pair_end[key] : g.pair_ptr[key + 1];  // pair_end: lists that grow (commit loop)
  const int64_t n_words = (g.n_nodes + 31) / 32;
  const bool use_cls = g.n_classes > 0;
  const uint8_t* other0 = g.other_status[0] ? g.other_status[0] + pod * g.row_stride : nullptr;
  const uint8_t* other1 = g.other_status[1] ? g.other_status[1] + pod * g.row_stride : nullptr;
  const int64_t tiles = (g.row_stride + 64 * kNpl - 1) / (64 * kNpl);

  if (flag != 0) {
    // scoreEqually: Filter passes, Score = MinNodeScore, NormalizeScore leaves all-zero rows alone
    // (networkoverhead.go:342-345, :376-379, :400-402); flag 2 = PreFilter returned Error
    const uint32_t st = flag == 2 ? 0xffffffffu : 0u;
    for (int64_t t = 0; t < tiles; ++t) {
      const int64_t n0 = (t * 64 + lane) * kNpl;
      if (n0 >= g.row_stride) continue;
      if (g.out_raw) {
        for (int j = 0; j < kNpl; ++j)
          if (n0 + j < g.n_nodes) g.out_raw[n0 + j] = 0;
      } else {
        *reinterpret_cast<uint32_t*>(g.out_status + pod * g.row_stride + n0) = st;
        *reinterpret_cast<uint32_t*>(g.out_score + pod * g.row_stride + n0) = 0u;
      }
    }
    return;
  }

  // ---- phase 1: per-class accumulation
  if (use_cls) {
    for (int c = lane; c < g.n_classes; c += 64) {
      Acc a{0, 0, 0};
      const int region = g.cls_region[c], zone = g.cls_zone[c];
      for (int i = lo; i < hi; ++i) {
        const int host = g.pair_node[i];  // wave-uniform
        add_pair(a, g, region, zone, g.region[host], g.zone[host], g.pair_max[i]);
      }
      cls_sat[c] = a.sat;
      cls_vio[c] = a.vio;
      cls_cost[c] = a.cost;
    }
    // ---- phase 2: host bitmap
    for (int64_t w = lane; w < n_words; w += 64) host_bits[w] = 0u;
    __syncthreads();
    for (int i = lo + lane; i < hi; i += 64) {
      const int host = g.pair_node[i];
      atomicOr(&host_bits[host >> 5], 1u << (host & 31));
    }
    __syncthreads();
  }

  auto eval = [&](int64_t n) -> Acc {
    if (!use_cls || ((host_bits[n >> 5] >> (n & 31)) & 1u)) return direct_eval<T>(g, n, lo, hi);
    const int c = g.node_class[n];
    return Acc{cls_sat[c], cls_vio[c], cls_cost[c]};
  };

  // ---- phase 3: Filter + min/max of the cost over feasible nodes (upstream scores feasible nodes only)
  T mn = std::numeric_limits<T>::max(), mx = std::numeric_limits<T>::min();
  for (int64_t t = 0; t < tiles; ++t) {
    const int64_t n0 = (t * 64 + lane) * kNpl;
#pragma unroll
    for (int j = 0; j < kNpl; ++j) {
      const int64_t n = n0 + j;
      if (n >= g.n_nodes) continue;
      const Acc a = eval(n);
      const bool feasible = !(a.vio > a.sat) && (!other0 || other0[n] == 0) && (!other1 || other1[n] == 0);
      if (feasible) {
        mn = a.cost < mn ? a.cost : mn;
        mx = a.cost > mx ? a.cost : mx;
      }
    }
  }
  mn = wave_min(mn);
  mx = wave_max(mx);

  // ---- phase 4: NormalizeScore (networkoverhead.go:389-418) + stores
  for (int64_t t = 0; t < tiles; ++t) {
    const int64_t n0 = (t * 64 + lane) * kNpl;
    if (n0 >= g.row_stride) continue;
    uint32_t st_w = 0, sc_w = 0;
#pragma unroll
    for (int j = 0; j < kNpl; ++j) {
      const int64_t n = n0 + j;
      if (n >= g.n_nodes) continue;
      const Acc a = eval(n);
      const bool pass = !(a.vio > a.sat);
      const bool feasible = pass && (!other0 || other0[n] == 0) && (!other1 || other1[n] == 0);
      int score = 0;
      if constexpr (kWide) {
        if (feasible) score = norm_cost_f64(a.cost, mn, mx);
      } else {
        if (feasible) score = norm_cost(a.cost, mn, mx);
      }
      if (g.out_raw) {
        g.out_raw[n] = g.raw_which == SPX_NET_RAW_SATISFIED ? a.sat : (g.raw_which == SPX_NET_RAW_VIOLATED ? a.vio : a.cost);
      } else {
        score = score < 0 ? 0 : (score > 255 ? 255 : score);
        st_w |= (pass ? 0u : static_cast<uint32_t>(SPX_NET_ST_UNSCHEDULABLE)) << (8 * j);
        sc_w |= static_cast<uint32_t>(score) << (8 * j);
      }
    }
    if (!g.out_raw) {
      *reinterpret_cast<uint32_t*>(g.out_status + pod * g.row_stride + n0) = st_w;
      *reinterpret_cast<uint32_t*>(g.out_score + pod * g.row_stride + n0) = sc_w;
    }
  }
}

}  // namespace

}  // namespace spx
