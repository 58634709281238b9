// flatten_preempt_nrt.cc — object tables -> the NRT side table of the preemption tables (spx_preempt_nrt_soa): what
// NodeResourceTopologyMatch's Filter reads when it runs inside PreemptionToleration's SelectVictimsOnNode.  Host side, once per snapshot.
//
// The eviction simulation (preemption.go:39-157) is additive: what a set of removed pods gives back is the sum of what each gives, per
// (NUMA id, resource), and it lands on the first ResourceInfo of that name of every zone whose name parses to the id.  So a pod's
// releases are formed once here, by the rule spx_nrt_post_eviction applies (nrt_release.hpp), and mapped to the node's zone list; the
// device keeps their running sums per cell.  What does not fit that form is refused: a zone the simulation would touch but the Filter
// does not list, and a resource listed twice in a zone (the simulation updates the first entry, the Filter reads the last).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/spx.h"
#include "nrt_release.hpp"

namespace {

constexpr int Z = SPX_NRT_MAX_ZONES;
constexpr int64_t kSumLimit = int64_t{1} << 62;
constexpr int64_t kBadArgument = INT64_MIN;

enum Kind { kOk = 0, kNode = 1, kAssigned = 2, kRow = 3, kTable = 4 };  // what *bad_out of the check names

// The first node, assigned pod or pod row the device cannot take (*bad), kTable for a table that is no table, or kOk.
Kind table_bad(const spx_preempt_nrt_soa* t, int64_t* bad) {
  *bad = -1;
  if (!t || t->n_nodes <= 0 || t->n_assigned < 0 || !t->slots || !t->node_flags || !t->n_zones || !t->zone_id || !t->zone_present || !t->node_present ||
      !t->zone_avail || !t->zone_headroom || !t->rel_ptr || !t->pods)
    return kTable;
  const spx_nrt_slots* s = t->slots;
  const spx_nrt_pods_soa* p = t->pods;
  const int R = s->n_res;
  if (R < 0 || R > SPX_NRT_MAX_RES || (R > 0 && (!s->slot_res || !s->slot_flags))) return kTable;
  if (t->n_assigned > 0 && !t->pod_contributes) return kTable;
  if (t->rel_ptr[0] != 0) return kTable;
  const int64_t n_rel = t->rel_ptr[t->n_assigned];
  if (n_rel < 0 || (n_rel > 0 && (!t->rel_zone || !t->rel_slot || !t->rel_qty))) return kTable;
  if (p->n_pods <= 0 || p->n_res != R || !p->qos || !p->non_native || !p->n_ctr || !p->ctr_kind || !p->ctr_present || !p->ctr_req || !p->pod_present || !p->pod_req)
    return kTable;
  for (int64_t n = 0; n < t->n_nodes; ++n) {
    *bad = n;
    if (t->n_zones[n] > Z) return kNode;
    for (int z = 0; z < t->n_zones[n]; ++z) {
      if (t->zone_id[n * Z + z] > 63) return kNode;
      if (R < 8 && (t->zone_present[n * Z + z] >> R)) return kNode;
      for (int r = 0; r < R; ++r)
        if (t->zone_headroom[(n * Z + z) * R + r] < 0) return kNode;  // available > allocatable
    }
  }
  for (int64_t j = 0; j < t->n_assigned; ++j) {
    *bad = j;
    if (t->rel_ptr[j + 1] < t->rel_ptr[j]) return kAssigned;
    for (int32_t k = t->rel_ptr[j]; k < t->rel_ptr[j + 1]; ++k)
      if (t->rel_qty[k] < 0 || t->rel_qty[k] >= kSumLimit || t->rel_zone[k] >= Z || t->rel_slot[k] >= R) return kAssigned;
  }
  for (int64_t i = 0; i < p->n_pods; ++i) {
    *bad = i;
    if (p->n_ctr[i] > SPX_NRT_MAX_CTRS) return kRow;  // a long row
  }
  *bad = -1;
  return kOk;
}

}  // namespace

extern "C" int spx_flatten_preempt_nrt_check(const spx_preempt_nrt_soa* t, int32_t* kind_out, int64_t* bad_out) {
  if (!kind_out || !bad_out) return SPX_ERR_ARG;
  *kind_out = table_bad(t, bad_out);
  return *kind_out == kOk ? SPX_OK : SPX_ERR_ARG;
}

extern "C" int spx_flatten_preempt_nrt(const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_resource_classes* rc, const spx_nrt_slots* slots,
                                       const spx_preempt_objects* o, const int32_t* ctr_numa, const uint8_t* placement_present,
                                       const int32_t* placement_containers, int64_t n_pods, const int32_t* pod_src, int64_t rel_cap, int64_t* n_rel_out, int64_t* bad_out,
                                       uint8_t* node_flags, uint8_t* n_zones, uint8_t* zone_id, uint8_t* zone_present, uint8_t* node_present, int64_t* zone_avail,
                                       int64_t* zone_headroom, uint8_t* pod_contributes, int32_t* rel_ptr, uint8_t* rel_zone, uint8_t* rel_slot, int64_t* rel_qty) {
  if (bad_out) *bad_out = kBadArgument;
  if (n_rel_out) *n_rel_out = 0;
  if (!nodes || !nrt || !slots || !o || !placement_present || !placement_containers || !n_rel_out || !bad_out || !node_flags || !n_zones || !zone_id ||
      !zone_present || !node_present || !zone_avail || !zone_headroom || !rel_ptr || n_pods < 0 || rel_cap < 0)
    return SPX_ERR_ARG;
  const int64_t N = nodes->n_nodes;
  const int R = slots->n_res;
  if (N <= 0 || nrt->n_nodes != N || !nrt->zres_allocatable || R < 0 || R > SPX_NRT_MAX_RES) return SPX_ERR_ARG;
  if (n_pods > 0 && (!o->assigned || !o->assigned_node || !ctr_numa || !pod_src || !pod_contributes)) return SPX_ERR_ARG;
  if (rel_cap > 0 && (!rel_zone || !rel_slot || !rel_qty)) return SPX_ERR_ARG;

  // the Filter's view of the nodes: spx_flatten_nrt_nodes' columns (assumed pods already subtracted from `available`)
  {
    std::vector<int32_t> max_numa(N), cost(static_cast<size_t>(N) * Z * Z);
    std::vector<float> dist(static_cast<size_t>(N) * Z);
    if (spx_flatten_nrt_nodes(nodes, nrt, slots, node_flags, max_numa.data(), n_zones, zone_id, zone_present, zone_avail, cost.data(), dist.data(), node_present) != SPX_OK) {
      // more than 8 zones, or a zone resource outside the slot table: find the node
      for (int64_t n = 0; n < N; ++n) {
        uint8_t f, nz, id[Z], zp[Z], np;
        int32_t mx, c[Z * Z];
        float d[Z];
        std::vector<int64_t> av(static_cast<size_t>(Z) * (R ? R : 1));
        const int64_t idx = n;
        if (spx_flatten_nrt_node_rows(nodes, nrt, slots, &idx, 1, &f, &mx, &nz, id, zp, av.data(), c, d, &np) != SPX_OK) {
          *bad_out = n;
          return SPX_ERR_ARG;
        }
      }
      return SPX_ERR_ARG;
    }
    // a node with more than 8 zones (spx_flatten_nrt_nodes marks it, its zones travel in a side table the refits do not read): refused
    // by name before any walk over its zones — this table keeps its 8 zones per node
    for (int64_t n = 0; n < N; ++n)
      if (n_zones[n] == SPX_NRT_ZONES_TALL) {
        *bad_out = n;
        return SPX_ERR_ARG;
      }
  }
  std::memset(zone_headroom, 0, static_cast<size_t>(N) * Z * (R ? R : 1) * sizeof(int64_t));
  auto slot_of = [&](int32_t res) {
    for (int s = 0; s < R; ++s)
      if (slots->slot_res[s] == res) return s;
    return -1;
  };
  for (int64_t n = 0; n < N; ++n) {
    if (placement_present[n] && placement_containers[n] != 0) node_flags[n] |= SPX_PNRT_F_PLACEMENT;
    if (!nrt->has_nrt[n]) continue;
    int pos = 0;
    for (int32_t z = nrt->zone_ptr[n]; z < nrt->zone_ptr[n + 1]; ++z) {
      const int32_t id = nrt->zone_numa_id[z];
      const bool listed = nrt->zone_is_node[z] && id >= 0 && id <= 63;
      if (id >= 0 && !listed) {  // the simulation would add to a zone the Filter never reads
        *bad_out = n;
        return SPX_ERR_ARG;
      }
      if (!listed) continue;
      for (int32_t k = nrt->zres_ptr[z]; k < nrt->zres_ptr[z + 1]; ++k) {
        for (int32_t k2 = nrt->zres_ptr[z]; k2 < k; ++k2)
          if (nrt->zres_res[k2] == nrt->zres_res[k]) {
            *bad_out = n;
            return SPX_ERR_ARG;
          }
        const int s = slot_of(nrt->zres_res[k]);  // (>= 0: spx_flatten_nrt_nodes took the node)
        const int64_t room = nrt->zres_allocatable[k] - zone_avail[(n * Z + pos) * R + s];
        if (room < 0) {  // available > allocatable
          *bad_out = n;
          return SPX_ERR_ARG;
        }
        zone_headroom[(n * Z + pos) * R + s] = room;
      }
      ++pos;
    }
  }

  // the pods, in the node table's order
  int64_t n_rel = 0;
  std::vector<uint64_t> total(static_cast<size_t>(N) * (R ? R : 1), 0);  // per node and slot: every release of its pods
  rel_ptr[0] = 0;
  for (int64_t j = 0; j < n_pods; ++j) {
    const int64_t v = pod_src[j];
    if (v < 0 || v >= o->n_assigned) return SPX_ERR_ARG;
    const int64_t n = o->assigned_node[v];
    if (n < 0 || n >= N) return SPX_ERR_ARG;
    pod_contributes[j] = 0;
    const bool sim = nrt->has_nrt[n] && (node_flags[n] & SPX_PNRT_F_PLACEMENT);  // without either no simulation ever reads the pod
    if (sim) {
      const int32_t e0 = nrt->zres_ptr[nrt->zone_ptr[n]], e1 = nrt->zres_ptr[nrt->zone_ptr[n + 1]];
      auto reported = [&](int32_t res) {  // cache.ResourceNamesFromNRT
        for (int32_t e = e0; e < e1; ++e)
          if (nrt->zres_res[e] == res) return true;
        return false;
      };
      int64_t bad = 0;
      int64_t entry_at[Z * SPX_NRT_MAX_RES];  // where the pod's entry for a (zone position, slot) sits, -1 = none yet
      std::fill(entry_at, entry_at + Z * SPX_NRT_MAX_RES, int64_t{-1});
      const bool any = spx_host::nrt_pod_releases(rc, o->assigned, v, spx_host::nrt_pod_qos(o->assigned, v), ctr_numa, reported, [&](int32_t numa, int32_t res, int64_t q) {
        if (q < 0) bad = -1 - v;
        if (q <= 0 || bad) return;  // a zero release changes nothing where available <= allocatable
        const int s = slot_of(res);
        if (s < 0) return;  // no zone reports it
        for (int z = 0; z < n_zones[n]; ++z) {
          if (zone_id[n * Z + z] != numa || !((zone_present[n * Z + z] >> s) & 1u)) continue;
          uint64_t& sum = total[static_cast<size_t>(n) * R + s];
          sum += static_cast<uint64_t>(q);
          if (q >= kSumLimit || sum >= static_cast<uint64_t>(kSumLimit)) {
            bad = n + 1;
            return;
          }
          int64_t& at = entry_at[z * SPX_NRT_MAX_RES + s];  // one entry per (zone position, slot) of the pod
          if (at >= 0) {
            if (at < rel_cap) rel_qty[at] += q;
            continue;
          }
          at = n_rel;
          if (n_rel < rel_cap) rel_zone[n_rel] = static_cast<uint8_t>(z), rel_slot[n_rel] = static_cast<uint8_t>(s), rel_qty[n_rel] = q;
          ++n_rel;
        }
      });
      if (bad) {
        *bad_out = bad < 0 ? bad : bad - 1;
        return SPX_ERR_ARG;
      }
      pod_contributes[j] = any;
    }
    if (n_rel > INT32_MAX) return SPX_ERR_ARG;
    rel_ptr[j + 1] = static_cast<int32_t>(n_rel);
  }
  *n_rel_out = n_rel;
  if (n_rel > rel_cap) return SPX_ERR_ARG;  // (*bad_out stays INT64_MIN: the count says what to allocate)
  *bad_out = 0;
  return SPX_OK;
}
