// flatten_nrt.cc — object tables -> SoA for NodeResourceTopologyMatch (host side, once per snapshot).
//
// Hoisted out of the per-(pod,node) path (the reference redoes all of it inside every Filter/Score call):
//   NRT DeepCopy + OverReserve subtraction of assumed pods          cache/store.go:84-91, :315-356
//   TopologyManager config decode                                    nodeconfig/topologymanager.go:78-162
//   createNUMANodeList / extractResources / extractCosts             pluginhelpers.go:105-161
//   util.ResourceList(node allocatable) key set                      pkg/util/resource.go:30-44
//   per-size minimum average NUMA distance                           least_numa.go:102-138
//   pod QoS class, IncludeNonNative, GetPodEffectiveRequest          filter.go:183-186, pkg/util/resource.go:51-85
#include <algorithm>
#include <cstdint>
#include <climits>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include <atomic>

#include "../../include/spx.h"
#include "nrt_release.hpp"
#include "parallel.hpp"

namespace {

constexpr int Z = SPX_NRT_MAX_ZONES;
constexpr int RM = SPX_NRT_MAX_RES;
constexpr int CM = SPX_NRT_MAX_CTRS;

inline bool is_fixed_native(int32_t res) {
  return res == SPX_RES_CPU || res == SPX_RES_MEMORY || res == SPX_RES_EPHEMERAL || res == SPX_RES_PODS || res == SPX_RES_STORAGE;
}
inline bool rc_has(const spx_resource_classes* rc, int32_t res, int flag) {
  if (is_fixed_native(res)) return flag == SPX_RC_NATIVE;
  if (!rc || res < 0 || res >= rc->n_res) return false;
  return (rc->flags[res] & flag) != 0;
}

inline int slot_of(const spx_nrt_slots* s, int32_t res) {
  for (int i = 0; i < s->n_res; ++i)
    if (s->slot_res[i] == res) return i;
  return -1;
}

struct KV {
  int32_t res;
  int64_t qty;
};
inline KV* kv_find(std::vector<KV>& v, int32_t res) {
  for (auto& e : v)
    if (e.res == res) return &e;
  return nullptr;
}

// GetPodEffectiveRequest (pkg/util/resource.go:51-85) with map key presence: pod i's request into `res` (init_res: scratch)
void pod_effective_request(const spx_pod_objects* pods, int64_t i, std::vector<KV>& init_res, std::vector<KV>& res) {
  const int32_t c0 = pods->ctr_ptr[i], c1 = pods->ctr_ptr[i + 1];
  init_res.clear();
  res.clear();
  for (int32_t c = c0; c < c1; ++c) {
    if (pods->ctr_kind[c] == SPX_CTR_APP) continue;
    for (int32_t k = pods->req_ptr[c]; k < pods->req_ptr[c + 1]; ++k) {
      KV* e = kv_find(init_res, pods->req_res[k]);
      if (e && pods->req_qty[k] <= e->qty) continue;
      if (e) e->qty = pods->req_qty[k];
      else init_res.push_back({pods->req_res[k], pods->req_qty[k]});
    }
  }
  for (int32_t c = c0; c < c1; ++c) {
    if (pods->ctr_kind[c] != SPX_CTR_APP) continue;
    for (int32_t k = pods->req_ptr[c]; k < pods->req_ptr[c + 1]; ++k) {
      KV* e = kv_find(res, pods->req_res[k]);
      if (e) e->qty += pods->req_qty[k];
      else res.push_back({pods->req_res[k], pods->req_qty[k]});
    }
  }
  for (const KV& in : init_res) {
    KV* e = kv_find(res, in.res);
    if (e && in.qty <= e->qty) continue;
    if (e) e->qty = in.qty;
    else res.push_back(in);
  }
  if (pods->ovh_ptr)
    for (int32_t k = pods->ovh_ptr[i]; k < pods->ovh_ptr[i + 1]; ++k) {
      KV* e = kv_find(res, pods->ovh_res[k]);
      if (e) e->qty += pods->ovh_qty[k];
      else res.push_back({pods->ovh_res[k], pods->ovh_qty[k]});
    }
}

// the slot numbering for up to `cap` slots; *n_res_out is written first when `count_first` (the wide form reports the count it refuses)
int flatten_slots(const spx_pod_objects* pods, const spx_nrt_objects* nrt, const spx_resource_classes* rc, const spx_nrt_params* p, int cap,
                  bool count_first, int32_t* n_res_out, int32_t* slot_res, uint8_t* slot_flags, int64_t* slot_weight);

}  // namespace

extern "C" int spx_flatten_nrt_slots(const spx_pod_objects* pods, const spx_nrt_objects* nrt, const spx_resource_classes* rc,
                                     const spx_nrt_params* p, int32_t* n_res_out, int32_t* slot_res, uint8_t* slot_flags,
                                     int64_t* slot_weight) {
  return flatten_slots(pods, nrt, rc, p, RM, false, n_res_out, slot_res, slot_flags, slot_weight);
}

extern "C" int spx_flatten_nrt_slots_wide(const spx_pod_objects* pods, const spx_nrt_objects* nrt, const spx_resource_classes* rc,
                                          const spx_nrt_params* p, int32_t cap, int32_t* n_res_out, int32_t* slot_res, uint8_t* slot_flags,
                                          int64_t* slot_weight) {
  if (cap < 0 || cap > SPX_NRT_MAX_RES_WIDE) return SPX_ERR_ARG;
  return flatten_slots(pods, nrt, rc, p, cap, true, n_res_out, slot_res, slot_flags, slot_weight);
}

namespace {
int flatten_slots(const spx_pod_objects* pods, const spx_nrt_objects* nrt, const spx_resource_classes* rc, const spx_nrt_params* p, int cap,
                  bool count_first, int32_t* n_res_out, int32_t* slot_res, uint8_t* slot_flags, int64_t* slot_weight) {
  if (!pods || !nrt || !n_res_out || !slot_res || !slot_flags || !slot_weight) return SPX_ERR_ARG;
  // the distinct resource ids of three long arrays (every container request, every overhead entry, every zone resource: ~0.8 M entries
  // at config #5's share): scanned in pieces on the host threads, each piece's handful of ids merged under a lock
  std::vector<int32_t> ids;
  std::mutex ids_mu;
  auto scan = [&](const int32_t* res, int64_t n) {
    if (!res || n <= 0) return;
    spx_host::parallel_rows(n, [&](int64_t b, int64_t e) {
      int32_t mine[64];
      int n_mine = 0;
      bool spill = false;
      std::vector<int32_t> more;  // (more than 64 distinct ids in one piece: the call fails below anyway, but stay correct)
      for (int64_t i = b; i < e; ++i) {
        const int32_t r = res[i];
        bool seen = false;
        for (int k = 0; k < n_mine && !seen; ++k) seen = mine[k] == r;
        if (seen) continue;
        if (n_mine < 64) mine[n_mine++] = r;
        else if (std::find(more.begin(), more.end(), r) == more.end()) more.push_back(r), spill = true;
      }
      std::lock_guard<std::mutex> g(ids_mu);
      for (int k = 0; k < n_mine; ++k)
        if (std::find(ids.begin(), ids.end(), mine[k]) == ids.end()) ids.push_back(mine[k]);
      if (spill)
        for (const int32_t r : more)
          if (std::find(ids.begin(), ids.end(), r) == ids.end()) ids.push_back(r);
    }, 65536);
  };
  const int64_t n_ctr = pods->ctr_ptr[pods->n_pods];
  scan(pods->req_res, pods->req_ptr[n_ctr]);
  if (pods->ovh_ptr) scan(pods->ovh_res, pods->ovh_ptr[pods->n_pods]);
  const int32_t n_zones = nrt->zone_ptr[nrt->n_nodes];
  scan(nrt->zres_res, nrt->zres_ptr[n_zones]);
  std::sort(ids.begin(), ids.end());
  if (count_first) *n_res_out = static_cast<int32_t>(ids.size());
  if (ids.size() > static_cast<size_t>(cap)) return SPX_ERR_ARG;  // more distinct resources than the caller's table holds
  *n_res_out = static_cast<int32_t>(ids.size());
  for (size_t s = 0; s < ids.size(); ++s) {
    const int32_t r = ids[s];
    slot_res[s] = r;
    uint8_t f = 0;
    if (r == SPX_RES_CPU || r == SPX_RES_MEMORY || rc_has(rc, r, SPX_RC_HUGEPAGE)) f |= SPX_NRT_SLOT_AFFINE;
    if (r == SPX_RES_EPHEMERAL || r == SPX_RES_STORAGE || !rc_has(rc, r, SPX_RC_NATIVE)) f |= SPX_NRT_SLOT_HOST_LEVEL;
    if (r == SPX_RES_CPU) f |= SPX_NRT_SLOT_CPU;
    slot_flags[s] = f;
    int64_t w = 1;  // resourceToWeightMap.weight: missing or < 1 -> defaultWeight (score.go:49-60)
    if (p)
      for (int32_t k = 0; k < p->n_weights; ++k)
        if (p->weight_res[k] == r) w = p->weight[k] < 1 ? 1 : p->weight[k];
    slot_weight[s] = w;
  }
  return SPX_OK;
}

// the zones createNUMANodeList keeps of node i (type Node, id 0..64); *id64: one of them carries id 64, beyond the 64-bit masks
inline int count_zones(const spx_nrt_objects* nrt, int64_t i, bool* id64) {
  int n = 0;
  if (!nrt->has_nrt[i]) return 0;
  for (int32_t z = nrt->zone_ptr[i]; z < nrt->zone_ptr[i + 1]; ++z) {
    if (!nrt->zone_is_node[z]) continue;
    const int id = nrt->zone_numa_id[z];
    if (id < 0 || id > 64) continue;
    if (id == 64) *id64 = true;
    ++n;
  }
  return n;
}

// node i of the object tables -> row j of the SoA columns; PM is the presence mask type (uint8_t: dense, uint32_t: wide)
template <typename PM>
int flatten_nrt_node(const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_nrt_slots* slots, int64_t i, int64_t j,
                     uint8_t* flags, int32_t* max_numa, uint8_t* n_zones, uint8_t* zone_id, PM* zone_present, int64_t* zone_avail,
                     int32_t* zone_cost, float* min_avg_dist, PM* node_present) {
  const int R = slots->n_res;
    // ---- TopologyManager config
    int scope = 0, policy = 0, mx = 8;
    const int lp = nrt->legacy_policy ? nrt->legacy_policy[i] : -1;
    if (lp >= 0) {
      policy = lp >> 1;
      scope = lp & 1;
    }
    if (nrt->attr_scope && nrt->attr_scope[i] >= 0) scope = nrt->attr_scope[i];
    if (nrt->attr_policy && nrt->attr_policy[i] >= 0) policy = nrt->attr_policy[i];
    if (nrt->attr_max_numa && nrt->attr_max_numa[i] > 1) mx = nrt->attr_max_numa[i] > 1024 ? 1024 : nrt->attr_max_numa[i];
    flags[j] = static_cast<uint8_t>((nrt->has_nrt[i] ? SPX_NRT_F_HAS_NRT : 0) | (nrt->fresh[i] ? SPX_NRT_F_FRESH : 0) |
                                    (policy == 3 ? SPX_NRT_F_SINGLE_NUMA : 0) | (scope == 1 ? SPX_NRT_F_POD_SCOPE : 0));
    max_numa[j] = mx;
    // ---- node-level key set of util.ResourceList(allocatable)
    PM np = 0;
    for (int s = 0; s < R; ++s) {
      const int32_t r = slots->slot_res[s];
      bool has = r == SPX_RES_CPU || r == SPX_RES_MEMORY || r == SPX_RES_PODS || r == SPX_RES_EPHEMERAL;
      for (int32_t k = nodes->scalar_ptr[i]; !has && k < nodes->scalar_ptr[i + 1]; ++k) has = nodes->scalar_res[k] == r;
      if (has) np |= static_cast<PM>(1u << s);
    }
    node_present[j] = np;
    // ---- more zones than the dense columns hold: a tall node (its zones go to spx_flatten_nrt_tall_nodes' table).  The dense row is
    // a placeholder the dense sweeps meet in every snapshot: no NRT object, no zones
    {
      bool id64 = false;
      const int total = count_zones(nrt, i, &id64);
      if (total > Z) {
        if (id64 || total > SPX_NRT_TALL_MAX_ZONES || sizeof(PM) != 1) return SPX_ERR_ARG;  // (the wide tables keep their 8 zones)
        flags[j] = static_cast<uint8_t>(flags[j] & ~SPX_NRT_F_HAS_NRT);
        n_zones[j] = SPX_NRT_ZONES_TALL;
        for (int k = 0; k < Z * Z; ++k) zone_cost[j * Z * Z + k] = 255;
        for (int k = 0; k < Z; ++k) min_avg_dist[j * Z + k] = 255.0f;
        return SPX_OK;
      }
    }
    // ---- NUMA node list (list order = zone order), with assumed pods subtracted from every zone
    int nz = 0;
    int32_t zsrc[Z];
    if (nrt->has_nrt[i]) {
      for (int32_t z = nrt->zone_ptr[i]; z < nrt->zone_ptr[i + 1]; ++z) {
        if (!nrt->zone_is_node[z]) continue;
        const int id = nrt->zone_numa_id[z];
        if (id < 0 || id > 64) continue;
        if (nz >= Z || id > 63) {
          return SPX_ERR_ARG;
        }  // beyond this build's limits (8 zones, ids 0..63)
        zsrc[nz] = z;
        zone_id[j * Z + nz] = static_cast<uint8_t>(id);
        PM present = 0;
        for (int32_t k = nrt->zres_ptr[z]; k < nrt->zres_ptr[z + 1]; ++k) {
          const int s = slot_of(slots, nrt->zres_res[k]);
          if (s < 0) {
            return SPX_ERR_ARG;
          }
          int64_t avail = nrt->zres_avail[k];
          if (nrt->assumed_ptr)
            for (int32_t a = nrt->assumed_ptr[i]; a < nrt->assumed_ptr[i + 1]; ++a)
              for (int32_t q = nrt->arl_ptr[a]; q < nrt->arl_ptr[a + 1]; ++q)
                if (nrt->arl_res[q] == nrt->zres_res[k]) avail = avail < nrt->arl_qty[q] ? 0 : avail - nrt->arl_qty[q];
          present |= static_cast<PM>(1u << s);
          zone_avail[(j * Z + nz) * R + s] = avail;
        }
        zone_present[j * Z + nz] = present;
        ++nz;
      }
    }
    n_zones[j] = static_cast<uint8_t>(nz);
    // ---- distance matrix by list position; 255 where Costs has no entry (least_numa.go:127-132)
    {
      // NUMA id -> list position (ids 0..63); an id carried by two zones keeps the slow walk below (every zone with that id takes
      // the entry).  With the map a zone's Costs list is walked once instead of once per column: the last entry for an id wins,
      // as in the column-by-column walk.
      int8_t pos_of[64];
      std::memset(pos_of, -1, sizeof pos_of);
      bool unique = true;
      for (int b = 0; b < nz; ++b) {
        const int id = zone_id[j * Z + b];
        unique &= pos_of[id] < 0;
        pos_of[id] = static_cast<int8_t>(b);
      }
      int32_t* row = zone_cost + j * Z * Z;
      for (int i = 0; i < Z * Z; ++i) row[i] = 255;
      if (nrt->zcost_ptr) {
        if (unique) {
          for (int a = 0; a < nz; ++a)
            for (int32_t k = nrt->zcost_ptr[zsrc[a]]; k < nrt->zcost_ptr[zsrc[a] + 1]; ++k) {
              const int32_t id = nrt->zcost_numa_id[k];
              if (id >= 0 && id < 64 && pos_of[id] >= 0) row[a * Z + pos_of[id]] = static_cast<int32_t>(nrt->zcost_value[k]);
            }
        } else {
          for (int a = 0; a < nz; ++a)
            for (int b = 0; b < nz; ++b) {
              const int want = zone_id[j * Z + b];
              for (int32_t k = nrt->zcost_ptr[zsrc[a]]; k < nrt->zcost_ptr[zsrc[a] + 1]; ++k)
                if (nrt->zcost_numa_id[k] == want) row[a * Z + b] = static_cast<int32_t>(nrt->zcost_value[k]);
            }
        }
      }
    }
    // ---- minAvgDistanceInCombinations for every subset size (float32 exactly as the reference)
    float best[Z];
    for (int k = 0; k < Z; ++k) best[k] = 255.0f;
    // every subset once, filed under its size; the sum over all ordered pairs of a subset grows from the subset without its
    // lowest member z: + cost[z][z] + sum over the others j of (cost[z][j] + cost[j][z])  (same integer as the double loop)
    int pair_sum[1 << Z], least[Z];
    pair_sum[0] = 0;
    for (int k = 0; k < Z; ++k) least[k] = INT32_MAX;
    const int32_t* c = zone_cost + j * Z * Z;
    for (unsigned m = 1; m < (1u << nz); ++m) {
      const int z = __builtin_ctz(m);
      const unsigned rest = m & (m - 1);
      int accu = pair_sum[rest] + c[z * Z + z];
      for (unsigned r = rest; r; r &= r - 1) {
        const int j = __builtin_ctz(r);
        accu += c[z * Z + j] + c[j * Z + z];
      }
      pair_sum[m] = accu;
      const int k = __builtin_popcount(m);
      if (accu < least[k - 1]) least[k - 1] = accu;
    }
    // float32(sum) / float32(k*k) is monotone in the sum: the minimum distance of a size is the distance of its smallest sum
    for (int k = 1; k <= nz; ++k) {
      const float d = static_cast<float>(least[k - 1]) / static_cast<float>(k * k);
      if (d < best[k - 1]) best[k - 1] = d;
    }
    for (int k = 0; k < Z; ++k) min_avg_dist[j * Z + k] = best[k];
  return SPX_OK;
}

template <typename PM>
int flatten_nodes(const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_nrt_slots* slots, uint8_t* flags, int32_t* max_numa,
                  uint8_t* n_zones, uint8_t* zone_id, PM* zone_present, int64_t* zone_avail, int32_t* zone_cost, float* min_avg_dist,
                  PM* node_present) {
  if (!nodes || !nrt || !slots || !flags || !max_numa || !n_zones || !zone_id || !zone_present || !zone_avail || !zone_cost ||
      !min_avg_dist || !node_present)
    return SPX_ERR_ARG;
  const int64_t n = nodes->n_nodes;
  if (nrt->n_nodes != n) return SPX_ERR_ARG;
  const int R = slots->n_res;
  std::memset(zone_id, 0, static_cast<size_t>(n) * Z);
  std::memset(zone_present, 0, static_cast<size_t>(n) * Z * sizeof(PM));
  std::memset(zone_avail, 0, static_cast<size_t>(n) * Z * R * sizeof(int64_t));
  std::atomic<int> err{SPX_OK};
  // nodes are independent: split across host threads (20k nodes x 255 zone subsets for the distance minima alone)
  spx_host::parallel_rows(n, [&](int64_t row0, int64_t row1) {
    for (int64_t i = row0; i < row1; ++i) {
      const int rc = flatten_nrt_node(nodes, nrt, slots, i, i, flags, max_numa, n_zones, zone_id, zone_present, zone_avail, zone_cost, min_avg_dist, node_present);
      if (rc != SPX_OK) {
        err = rc;
        return;
      }
    }
  }, 256);
  return err.load();
}
}  // namespace

extern "C" int spx_flatten_nrt_nodes(const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_nrt_slots* slots,
                                     uint8_t* flags, int32_t* max_numa, uint8_t* n_zones, uint8_t* zone_id,
                                     uint8_t* zone_present, int64_t* zone_avail, int32_t* zone_cost, float* min_avg_dist,
                                     uint8_t* node_present) {
  return flatten_nodes(nodes, nrt, slots, flags, max_numa, n_zones, zone_id, zone_present, zone_avail, zone_cost, min_avg_dist, node_present);
}

extern "C" int spx_flatten_nrt_nodes_wide(const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_nrt_slots* slots,
                                          uint8_t* flags, int32_t* max_numa, uint8_t* n_zones, uint8_t* zone_id,
                                          uint32_t* zone_present, int64_t* zone_avail, int32_t* zone_cost, float* min_avg_dist,
                                          uint32_t* node_present) {
  if (slots && (slots->n_res < 0 || slots->n_res > SPX_NRT_MAX_RES_WIDE)) return SPX_ERR_ARG;
  return flatten_nodes(nodes, nrt, slots, flags, max_numa, n_zones, zone_id, zone_present, zone_avail, zone_cost, min_avg_dist, node_present);
}

// the same columns for the listed nodes only (a snapshot delta: spx_update_nrt_nodes takes these rows): row j describes node idx[j]
extern "C" int spx_flatten_nrt_node_rows(const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_nrt_slots* slots,
                                         const int64_t* idx, int64_t n_rows, uint8_t* flags, int32_t* max_numa, uint8_t* n_zones,
                                         uint8_t* zone_id, uint8_t* zone_present, int64_t* zone_avail, int32_t* zone_cost, float* min_avg_dist,
                                         uint8_t* node_present) {
  if (!nodes || !nrt || !slots || !idx || !flags || !max_numa || !n_zones || !zone_id || !zone_present || !zone_avail || !zone_cost ||
      !min_avg_dist || !node_present || n_rows < 0)
    return SPX_ERR_ARG;
  if (nrt->n_nodes != nodes->n_nodes) return SPX_ERR_ARG;
  const int R = slots->n_res;
  std::memset(zone_id, 0, static_cast<size_t>(n_rows) * Z);
  std::memset(zone_present, 0, static_cast<size_t>(n_rows) * Z);
  std::memset(zone_avail, 0, static_cast<size_t>(n_rows) * Z * R * sizeof(int64_t));
  for (int64_t j = 0; j < n_rows; ++j) {
    if (idx[j] < 0 || idx[j] >= nodes->n_nodes) return SPX_ERR_ARG;
    const int rc = flatten_nrt_node(nodes, nrt, slots, idx[j], j, flags, max_numa, n_zones, zone_id, zone_present, zone_avail, zone_cost, min_avg_dist, node_present);
    if (rc != SPX_OK) return rc;
  }
  return SPX_OK;
}

extern "C" int spx_nrt_first_tall_node(const spx_nrt_objects* nrt, int64_t* node_out, int32_t* n_zones_out) {
  if (!nrt || !node_out || !n_zones_out) return SPX_ERR_ARG;
  *node_out = -1;
  *n_zones_out = 0;
  for (int64_t i = 0; i < nrt->n_nodes; ++i) {
    bool id64 = false;
    const int total = count_zones(nrt, i, &id64);
    if (total > SPX_NRT_TALL_MAX_ZONES || (id64 && total > Z)) {
      *node_out = i, *n_zones_out = total;
      return SPX_ERR_ARG;
    }
    if (total > Z && *node_out < 0) *node_out = i, *n_zones_out = total;
  }
  return SPX_OK;
}

namespace {
// minAvgDistanceInCombinations for every subset size of one (zone count, cost matrix) key of nz <= 16 zones — key = {nz, the nz x nz
// costs by list position} — float32 exactly as the dense flattener: every subset once, its pair sum grown from the subset without
// its lowest member (2^nz ints on the heap).  65 535 subsets at 16 zones, about a millisecond of one host thread.
std::vector<float> tall_min_avg(const std::vector<int32_t>& key) {
  const int nz = key[0];
  const int32_t* c = key.data() + 1;
  std::vector<int> pair_sum(size_t{1} << nz);
  int least[SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA];
  for (int k = 0; k < nz; ++k) least[k] = INT32_MAX;
  pair_sum[0] = 0;
  for (unsigned m = 1; m < (1u << nz); ++m) {
    const int z = __builtin_ctz(m);
    const unsigned rest = m & (m - 1);
    int accu = pair_sum[rest] + c[z * nz + z];
    for (unsigned r = rest; r; r &= r - 1) {
      const int j = __builtin_ctz(r);
      accu += c[z * nz + j] + c[j * nz + z];
    }
    pair_sum[m] = accu;
    const int k = __builtin_popcount(m);
    if (accu < least[k - 1]) least[k - 1] = accu;
  }
  std::vector<float> best(static_cast<size_t>(nz), 255.0f);
  for (int k = 1; k <= nz; ++k) {
    const float d = static_cast<float>(least[k - 1]) / static_cast<float>(k * k);
    if (d < best[k - 1]) best[k - 1] = d;
  }
  return best;
}
}  // namespace

extern "C" int spx_flatten_nrt_tall_nodes(const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_nrt_slots* slots, int64_t tall_cap,
                                          int32_t stride_cap, int64_t* n_tall_out, int32_t* zone_stride_out, int32_t* node_idx, uint8_t* flags,
                                          int32_t* max_numa, uint8_t* node_present, uint8_t* n_zones, uint8_t* zone_id, uint8_t* zone_present,
                                          int64_t* zone_avail, int32_t* zone_cost, float* min_avg_dist) {
  if (!nodes || !nrt || !slots || !n_tall_out || !zone_stride_out || nrt->n_nodes != nodes->n_nodes) return SPX_ERR_ARG;
  const bool count_only = !node_idx && !flags && !max_numa && !node_present && !n_zones && !zone_id && !zone_present && !zone_avail && !zone_cost && !min_avg_dist;
  if (!count_only && (!node_idx || !flags || !max_numa || !node_present || !n_zones || !zone_id || !zone_present || !zone_cost || !min_avg_dist ||
                      (!zone_avail && slots->n_res) || tall_cap < 0 || stride_cap < 0))
    return SPX_ERR_ARG;
  const int R = slots->n_res;
  if (R < 0 || R > RM) return SPX_ERR_ARG;  // (tall nodes in a wide snapshot stay refused)
  int64_t n_tall = 0;
  int32_t zs = 0;
  for (int64_t i = 0; i < nrt->n_nodes; ++i) {
    bool id64 = false;
    const int total = count_zones(nrt, i, &id64);
    if (total <= Z) continue;
    if (id64 || total > SPX_NRT_TALL_MAX_ZONES) return SPX_ERR_ARG;
    ++n_tall;
    zs = total > zs ? total : zs;
  }
  *n_tall_out = n_tall;
  *zone_stride_out = zs;
  if (count_only) return SPX_OK;
  if (n_tall > tall_cap || zs > stride_cap || n_tall > INT32_MAX) return SPX_ERR_ARG;
  const size_t T = static_cast<size_t>(n_tall), S = static_cast<size_t>(zs);
  std::memset(zone_id, 0, T * S);
  std::memset(zone_present, 0, T * S);
  if (R) std::memset(zone_avail, 0, T * S * static_cast<size_t>(R) * sizeof(int64_t));
  for (size_t q = 0; q < T * S * S; ++q) zone_cost[q] = 255;
  for (size_t q = 0; q < T * S; ++q) min_avg_dist[q] = 255.0f;
  // the distance minima are kept per (zone count, cost matrix): the machines of one model share a key and cost one enumeration
  std::map<std::vector<int32_t>, size_t> key_of;
  std::vector<const std::vector<int32_t>*> keys;
  std::vector<int64_t> key_at(T, -1);
  int64_t k = 0;
  for (int64_t i = 0; i < nrt->n_nodes; ++i) {
    bool id64 = false;
    if (count_zones(nrt, i, &id64) <= Z) continue;
    node_idx[k] = static_cast<int32_t>(i);
    // the node's own record: the dense row's flags (with HAS_NRT as the snapshot has it), max_numa and key set, from the dense walk
    {
      uint8_t f = 0, nzd = 0, np = 0, zid[Z] = {0}, zp[Z] = {0};
      int32_t mx = 0, cost[Z * Z];
      float mavg[Z];
      int64_t av[Z * RM] = {0};
      const int rc = flatten_nrt_node<uint8_t>(nodes, nrt, slots, i, 0, &f, &mx, &nzd, zid, zp, av, cost, mavg, &np);
      if (rc != SPX_OK) return rc;
      flags[k] = static_cast<uint8_t>(f | SPX_NRT_F_HAS_NRT);
      max_numa[k] = mx;
      node_present[k] = np;
    }
    int nz = 0;
    int32_t zsrc[SPX_NRT_TALL_MAX_ZONES];
    for (int32_t z = nrt->zone_ptr[i]; z < nrt->zone_ptr[i + 1]; ++z) {
      if (!nrt->zone_is_node[z]) continue;
      const int id = nrt->zone_numa_id[z];
      if (id < 0 || id > 64) continue;
      zsrc[nz] = z;
      zone_id[k * zs + nz] = static_cast<uint8_t>(id);
      uint8_t present = 0;
      for (int32_t e = nrt->zres_ptr[z]; e < nrt->zres_ptr[z + 1]; ++e) {
        const int s = slot_of(slots, nrt->zres_res[e]);
        if (s < 0) return SPX_ERR_ARG;
        int64_t avail = nrt->zres_avail[e];
        if (nrt->assumed_ptr)
          for (int32_t a = nrt->assumed_ptr[i]; a < nrt->assumed_ptr[i + 1]; ++a)
            for (int32_t q = nrt->arl_ptr[a]; q < nrt->arl_ptr[a + 1]; ++q)
              if (nrt->arl_res[q] == nrt->zres_res[e]) avail = avail < nrt->arl_qty[q] ? 0 : avail - nrt->arl_qty[q];
        present |= static_cast<uint8_t>(1u << s);
        zone_avail[(k * zs + nz) * R + s] = avail;
      }
      zone_present[k * zs + nz] = present;
      ++nz;
    }
    n_zones[k] = static_cast<uint8_t>(nz);
    // distance matrix by list position, 255 where Costs has no entry; duplicate ids as in the dense flattener: with unique ids the
    // last entry for an id wins, else every zone with that id takes the entry
    int32_t* row = zone_cost + static_cast<size_t>(k) * S * S;
    if (nrt->zcost_ptr) {
      int8_t pos_of[64];
      std::memset(pos_of, -1, sizeof pos_of);
      bool unique = true;
      for (int b = 0; b < nz; ++b) {
        const int id = zone_id[k * zs + b];
        unique &= pos_of[id] < 0;
        pos_of[id] = static_cast<int8_t>(b);
      }
      if (unique) {
        for (int a = 0; a < nz; ++a)
          for (int32_t e = nrt->zcost_ptr[zsrc[a]]; e < nrt->zcost_ptr[zsrc[a] + 1]; ++e) {
            const int32_t id = nrt->zcost_numa_id[e];
            if (id >= 0 && id < 64 && pos_of[id] >= 0) row[a * zs + pos_of[id]] = static_cast<int32_t>(nrt->zcost_value[e]);
          }
      } else {
        for (int a = 0; a < nz; ++a)
          for (int b = 0; b < nz; ++b) {
            const int want = zone_id[k * zs + b];
            for (int32_t e = nrt->zcost_ptr[zsrc[a]]; e < nrt->zcost_ptr[zsrc[a] + 1]; ++e)
              if (nrt->zcost_numa_id[e] == want) row[a * zs + b] = static_cast<int32_t>(nrt->zcost_value[e]);
          }
      }
    }
    if (nz <= SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA) {
      std::vector<int32_t> key;
      key.reserve(static_cast<size_t>(nz) * nz + 1);
      key.push_back(nz);
      for (int a = 0; a < nz; ++a)
        for (int b = 0; b < nz; ++b) key.push_back(row[a * zs + b]);
      const auto at = key_of.emplace(std::move(key), keys.size());
      if (at.second) keys.push_back(&at.first->first);
      key_at[static_cast<size_t>(k)] = static_cast<int64_t>(at.first->second);
    }
    ++k;
  }
  // the distinct keys on the host threads (a snapshot of 5 000 tall nodes with a matrix each is 5 000 enumerations, a few seconds of one
  // thread), then every node takes its key's row
  std::vector<std::vector<float>> minima(keys.size());
  spx_host::parallel_rows(static_cast<int64_t>(keys.size()), [&](int64_t k0, int64_t k1) {
    for (int64_t q = k0; q < k1; ++q) minima[static_cast<size_t>(q)] = tall_min_avg(*keys[static_cast<size_t>(q)]);
  }, 1);
  for (size_t q = 0; q < T; ++q)
    if (key_at[q] >= 0) std::copy(minima[static_cast<size_t>(key_at[q])].begin(), minima[static_cast<size_t>(key_at[q])].end(), min_avg_dist + q * S);
  return SPX_OK;
}

extern "C" int spx_flatten_nrt_pods(const spx_pod_objects* pods, const spx_resource_classes* rc, const spx_nrt_slots* slots,
                                    uint8_t* qos, uint8_t* non_native, uint8_t* n_ctr, uint8_t* ctr_kind, uint8_t* ctr_present,
                                    int64_t* ctr_req, uint8_t* pod_present, int64_t* pod_req) {
  if (!pods || !slots || !qos || !non_native || !n_ctr || !ctr_kind || !ctr_present || !ctr_req || !pod_present || !pod_req)
    return SPX_ERR_ARG;
  const int R = slots->n_res;
  const int64_t P = pods->n_pods;
  std::atomic<int> err{SPX_OK};
  spx_host::parallel_rows(P, [&](int64_t row0, int64_t row1) {
  std::vector<KV> init_res, res;
  for (int64_t i = row0; i < row1; ++i) {
    // the row's cells are cleared by the thread that fills them, row by row (one serial memset of the 16 MB request column cost
    // more than the whole parallel fill)
    std::memset(ctr_kind + i * CM, 0, CM);
    std::memset(ctr_present + i * CM, 0, CM);
    std::memset(ctr_req + i * CM * R, 0, static_cast<size_t>(CM) * R * sizeof(int64_t));
    std::memset(pod_req + i * R, 0, static_cast<size_t>(R) * sizeof(int64_t));
    const int32_t c0 = pods->ctr_ptr[i], c1 = pods->ctr_ptr[i + 1];
    // more containers than the dense columns hold: a long row (its containers go to spx_flatten_nrt_long_pods' table)
    const bool is_long = c1 - c0 > CM;
    qos[i] = static_cast<uint8_t>(spx_host::nrt_pod_qos(pods, i));
    bool nn = false;
    n_ctr[i] = static_cast<uint8_t>(is_long ? SPX_NRT_CTRS_LONG : c1 - c0);
    for (int32_t c = c0; c < c1; ++c) {
      const int64_t slot_base = (i * CM + (c - c0));
      if (!is_long) ctr_kind[slot_base] = pods->ctr_kind[c];
      uint8_t present = 0;
      for (int32_t k = pods->req_ptr[c]; k < pods->req_ptr[c + 1]; ++k) {
        const int s = slot_of(slots, pods->req_res[k]);
        if (s < 0) {
          err = SPX_ERR_ARG;
          return;
        }
        present |= static_cast<uint8_t>(1u << s);
        if (!is_long) ctr_req[slot_base * R + s] = pods->req_qty[k];
        if (!rc_has(rc, pods->req_res[k], SPX_RC_NATIVE)) nn = true;
      }
      if (!is_long) ctr_present[slot_base] = present;
    }
    non_native[i] = nn ? 1 : 0;
    pod_effective_request(pods, i, init_res, res);
    uint8_t pp = 0;
    for (const KV& e : res) {
      const int s = slot_of(slots, e.res);
      if (s < 0) {
        err = SPX_ERR_ARG;
        return;
      }
      pp |= static_cast<uint8_t>(1u << s);
      pod_req[i * R + s] = e.qty;
    }
    pod_present[i] = pp;
  }
  }, 4096);
  return err.load();
}

extern "C" int spx_flatten_nrt_long_pods(const spx_pod_objects* pods, const spx_resource_classes* rc, const spx_nrt_slots* slots, int64_t long_cap,
                                         int64_t ctr_cap, int64_t* n_long_out, int64_t* n_ctr_out, int32_t* pod_row, int32_t* ctr_ptr,
                                         uint8_t* ctr_kind, uint8_t* ctr_present, int64_t* ctr_req) {
  (void)rc;  // (the dense table carries the pod-level columns; the containers' own need no resource classes)
  if (!pods || !slots || !n_long_out || !n_ctr_out) return SPX_ERR_ARG;
  const bool count_only = !pod_row && !ctr_ptr && !ctr_kind && !ctr_present && !ctr_req;
  if (!count_only && (!pod_row || !ctr_ptr || !ctr_kind || !ctr_present || !ctr_req || long_cap < 0 || ctr_cap < 0)) return SPX_ERR_ARG;
  const int R = slots->n_res;
  int64_t n_long = 0, n_ctr = 0;
  for (int64_t i = 0; i < pods->n_pods; ++i) {
    const int64_t n = pods->ctr_ptr[i + 1] - pods->ctr_ptr[i];
    if (n > CM) ++n_long, n_ctr += n;
  }
  *n_long_out = n_long;
  *n_ctr_out = n_ctr;
  if (count_only) return SPX_OK;
  if (n_long > long_cap || n_ctr > ctr_cap || n_ctr > INT32_MAX) return SPX_ERR_ARG;
  int64_t k = 0, at = 0;
  ctr_ptr[0] = 0;
  for (int64_t i = 0; i < pods->n_pods; ++i) {
    const int32_t c0 = pods->ctr_ptr[i], c1 = pods->ctr_ptr[i + 1];
    if (c1 - c0 <= CM) continue;
    pod_row[k] = static_cast<int32_t>(i);
    for (int32_t c = c0; c < c1; ++c, ++at) {
      ctr_kind[at] = pods->ctr_kind[c];
      std::memset(ctr_req + at * R, 0, static_cast<size_t>(R) * sizeof(int64_t));
      uint8_t present = 0;
      for (int32_t q = pods->req_ptr[c]; q < pods->req_ptr[c + 1]; ++q) {
        const int s = slot_of(slots, pods->req_res[q]);
        if (s < 0) return SPX_ERR_ARG;
        present |= static_cast<uint8_t>(1u << s);
        ctr_req[at * R + s] = pods->req_qty[q];
      }
      ctr_present[at] = present;
    }
    ctr_ptr[++k] = static_cast<int32_t>(at);
  }
  return SPX_OK;
}

// Wide pod table: every list in ascending slot order.  Pass 1 takes each container's and each pod's presence mask (uint32: up to 32
// slots) on the host threads, the list offsets follow from their popcounts, pass 2 fills the lists.
extern "C" int spx_flatten_nrt_pods_wide(const spx_pod_objects* pods, const spx_resource_classes* rc, const spx_nrt_slots* slots, int64_t req_cap,
                                         int64_t ent_cap, int64_t* n_req_out, int64_t* n_ent_out, uint8_t* qos, uint8_t* non_native,
                                         int32_t* req_ptr, uint8_t* req_slot, int64_t* req_qty, int32_t* ctr_ptr, uint8_t* ctr_kind,
                                         int32_t* ent_ptr, uint8_t* ent_slot, int64_t* ent_qty) {
  if (!pods || !slots || !n_req_out || !n_ent_out || slots->n_res < 0 || slots->n_res > SPX_NRT_MAX_RES_WIDE) return SPX_ERR_ARG;
  const bool count_only = !qos && !non_native && !req_ptr && !req_slot && !req_qty && !ctr_ptr && !ctr_kind && !ent_ptr && !ent_slot && !ent_qty;
  if (!count_only && (!qos || !non_native || !req_ptr || !req_slot || !req_qty || !ctr_ptr || !ctr_kind || !ent_ptr || !ent_slot || !ent_qty))
    return SPX_ERR_ARG;
  // (a pod table may be a view into a larger one: its container offsets need not start at 0; the outputs are rebased)
  const int64_t P = pods->n_pods, cb = pods->ctr_ptr[0], C = pods->ctr_ptr[P] - cb;
  std::vector<uint32_t> cmask(static_cast<size_t>(C)), pmask(static_cast<size_t>(P));
  std::atomic<int> err{SPX_OK};
  spx_host::parallel_rows(P, [&](int64_t row0, int64_t row1) {
    std::vector<KV> init_res, res;
    for (int64_t i = row0; i < row1; ++i) {
      bool nn = false;
      for (int32_t c = pods->ctr_ptr[i]; c < pods->ctr_ptr[i + 1]; ++c) {
        uint32_t m = 0;
        for (int32_t k = pods->req_ptr[c]; k < pods->req_ptr[c + 1]; ++k) {
          const int s = slot_of(slots, pods->req_res[k]);
          if (s < 0) {
            err = SPX_ERR_ARG;
            return;
          }
          m |= 1u << s;
          if (!rc_has(rc, pods->req_res[k], SPX_RC_NATIVE)) nn = true;
        }
        cmask[static_cast<size_t>(c - cb)] = m;
      }
      pod_effective_request(pods, i, init_res, res);
      uint32_t m = 0;
      for (const KV& e : res) {
        const int s = slot_of(slots, e.res);
        if (s < 0) {
          err = SPX_ERR_ARG;
          return;
        }
        m |= 1u << s;
      }
      pmask[static_cast<size_t>(i)] = m;
      if (!count_only) {
        qos[i] = static_cast<uint8_t>(spx_host::nrt_pod_qos(pods, i));
        non_native[i] = nn ? 1 : 0;
      }
    }
  }, 4096);
  if (err.load() != SPX_OK) return err.load();
  int64_t n_req = 0, n_ent = 0;
  for (int64_t i = 0; i < P; ++i) n_req += __builtin_popcount(pmask[static_cast<size_t>(i)]);
  for (int64_t c = 0; c < C; ++c) n_ent += __builtin_popcount(cmask[static_cast<size_t>(c)]);
  *n_req_out = n_req;
  *n_ent_out = n_ent;
  if (count_only) return SPX_OK;
  if (n_req > req_cap || n_ent > ent_cap || n_req > INT32_MAX || n_ent > INT32_MAX) return SPX_ERR_ARG;
  req_ptr[0] = 0;
  for (int64_t i = 0; i < P; ++i) {
    req_ptr[i + 1] = req_ptr[i] + __builtin_popcount(pmask[static_cast<size_t>(i)]);
    ctr_ptr[i] = static_cast<int32_t>(pods->ctr_ptr[i] - cb);
  }
  ctr_ptr[P] = static_cast<int32_t>(C);
  ent_ptr[0] = 0;
  for (int64_t c = 0; c < C; ++c) ent_ptr[c + 1] = ent_ptr[c] + __builtin_popcount(cmask[static_cast<size_t>(c)]);
  spx_host::parallel_rows(P, [&](int64_t row0, int64_t row1) {
    std::vector<KV> init_res, res;
    int64_t qty[SPX_NRT_MAX_RES_WIDE];
    for (int64_t i = row0; i < row1; ++i) {
      for (int32_t c = pods->ctr_ptr[i]; c < pods->ctr_ptr[i + 1]; ++c) {
        ctr_kind[c - cb] = pods->ctr_kind[c];
        for (int32_t k = pods->req_ptr[c]; k < pods->req_ptr[c + 1]; ++k) qty[slot_of(slots, pods->req_res[k])] = pods->req_qty[k];  // (the last entry of a name wins, as in the dense table)
        int32_t at = ent_ptr[c - cb];
        for (uint32_t m = cmask[static_cast<size_t>(c - cb)]; m; m &= m - 1) {
          const int s = __builtin_ctz(m);
          ent_slot[at] = static_cast<uint8_t>(s);
          ent_qty[at++] = qty[s];
        }
      }
      pod_effective_request(pods, i, init_res, res);
      for (const KV& e : res) qty[slot_of(slots, e.res)] = e.qty;
      int32_t at = req_ptr[i];
      for (uint32_t m = pmask[static_cast<size_t>(i)]; m; m &= m - 1) {
        const int s = __builtin_ctz(m);
        req_slot[at] = static_cast<uint8_t>(s);
        req_qty[at++] = qty[s];
      }
    }
  }, 4096);
  return SPX_OK;
}
