// flatten_cosched.cc — object tables -> SoA columns for Coscheduling's PreFilter gate (pkg/coscheduling/core/core.go), the limits of
// the device's int64 sums, and Coscheduling.Less.  Host-side product code (once per snapshot).
//
// What is hoisted out of the per-(group, node) path, and where the reference does it per call:
//   node  : getNodeResource's left-over with NO pod removed (core.go:446-464): allocatable - requested per resource, AllowedPodNumber -
//           len(pods); requested and the pod count are the sums over the assigned pods listed for the node            -> left_base
//   group : info.Snapshot() + RemovePod of the group's own pods (core.go:434-444): what those pods requested, +1 pod each, per node that
//           hosts any                                                                                               -> the step list
//           MinResources.DeepCopy() with pods = MinMember (core.go:295-297)                                           -> req, req_mask
// With those, CheckClusterResource (core.go:406-426) is: every named slot r has a present node i with
// sum over present j <= i of (left_base[r][j] + step_g[r][j]) >= req_r (include/spx.h).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/spx.h"

namespace {

bool groups_ok(const spx_cosched_objects* o) {
  if (!o || o->n_groups < 0 || o->n_nodes < 0 || o->n_pods < 0) return false;
  if (o->n_groups && (!o->g_exists || !o->g_min_member || !o->g_has_min_resources || !o->g_res_ptr)) return false;
  for (int32_t g = 0; g < o->n_groups; ++g)
    if (o->g_res_ptr[g] < 0 || o->g_res_ptr[g + 1] < o->g_res_ptr[g]) return false;
  const int32_t total = o->n_groups ? o->g_res_ptr[o->n_groups] : 0;
  if (total && (!o->g_res_id || !o->g_res_qty)) return false;
  for (int32_t i = 0; i < total; ++i)
    if (o->g_res_id[i] < 0) return false;
  return true;
}

bool assigned_ok(const spx_cosched_objects* o) {
  if (o->n_nodes == 0) return true;
  if (!o->node_present || !o->a_ptr) return false;
  for (int64_t n = 0; n < o->n_nodes; ++n)
    if (o->a_ptr[n] < 0 || o->a_ptr[n + 1] < o->a_ptr[n]) return false;
  const int32_t total = o->a_ptr[o->n_nodes];
  if (total == 0) return true;
  if (!o->a_group || !o->a_req_ptr) return false;
  for (int32_t i = 0; i < total; ++i) {
    if (o->a_group[i] < -1 || o->a_group[i] >= o->n_groups) return false;
    if (o->a_req_ptr[i] < 0 || o->a_req_ptr[i + 1] < o->a_req_ptr[i]) return false;
  }
  if (o->a_req_ptr[total] && (!o->a_req_res || !o->a_req_qty)) return false;
  return true;
}

// the group reaches CheckClusterResource at all (core.go:246-249, :279-281)
inline bool gated_by_resources(const spx_cosched_objects* o, int32_t g) { return o->g_exists[g] && o->g_has_min_resources[g]; }

inline int slot_of(int32_t n_slots, const int32_t* slot_res, int32_t res) {
  for (int32_t s = 0; s < n_slots; ++s)
    if (slot_res[s] == res) return s;
  return -1;
}

// allocatable of node n for a resource id; *listed = false when the node does not carry it (a scalar outside ScalarResources)
int64_t node_alloc(const spx_node_objects* nodes, int64_t n, int32_t res, bool* listed) {
  *listed = true;
  switch (res) {
    case SPX_RES_CPU: return nodes->alloc_cpu_milli[n];
    case SPX_RES_MEMORY: return nodes->alloc_mem[n];
    case SPX_RES_EPHEMERAL: return nodes->alloc_eph[n];
    case SPX_RES_PODS: return nodes->alloc_pods[n];
    default: break;
  }
  if (nodes->scalar_ptr)
    for (int32_t j = nodes->scalar_ptr[n]; j < nodes->scalar_ptr[n + 1]; ++j)
      if (nodes->scalar_res[j] == res) return nodes->scalar_qty[j];
  *listed = false;
  return 0;
}

bool nodes_ok(const spx_node_objects* nodes, const spx_cosched_objects* o) {
  if (!nodes || nodes->n_nodes != o->n_nodes) return false;
  if (o->n_nodes && (!nodes->alloc_cpu_milli || !nodes->alloc_mem || !nodes->alloc_eph || !nodes->alloc_pods)) return false;
  return true;
}

inline uint64_t mag(int64_t v) { return v < 0 ? uint64_t{0} - static_cast<uint64_t>(v) : static_cast<uint64_t>(v); }

}  // namespace

extern "C" int spx_flatten_cosched_slots(const spx_cosched_objects* o, int32_t* n_slots_out, int32_t* slot_res) {
  if (!groups_ok(o) || !n_slots_out || !slot_res) return SPX_ERR_ARG;
  std::vector<int32_t> ids{SPX_RES_PODS};
  for (int32_t g = 0; g < o->n_groups; ++g) {
    if (!gated_by_resources(o, g)) continue;
    for (int32_t i = o->g_res_ptr[g]; i < o->g_res_ptr[g + 1]; ++i) ids.push_back(o->g_res_id[i]);
  }
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  *n_slots_out = static_cast<int32_t>(std::min<size_t>(ids.size(), INT32_MAX));
  if (ids.size() > SPX_COSCHED_MAX_SLOTS) return SPX_ERR_ARG;
  std::copy(ids.begin(), ids.end(), slot_res);
  return SPX_OK;
}

extern "C" int spx_flatten_cosched_nodes(const spx_node_objects* nodes, const spx_cosched_objects* o, int32_t n_slots, const int32_t* slot_res,
                                         int64_t* left_base, uint8_t* node_present) {
  if (!groups_ok(o) || !assigned_ok(o) || !nodes_ok(nodes, o) || n_slots < 1 || n_slots > SPX_COSCHED_MAX_SLOTS || !slot_res || !left_base || !node_present)
    return SPX_ERR_ARG;
  const int64_t N = o->n_nodes;
  for (int64_t n = 0; n < N; ++n) {
    node_present[n] = o->node_present[n] ? 1 : 0;
    int64_t requested[SPX_COSCHED_MAX_SLOTS] = {0};
    for (int32_t i = o->a_ptr[n]; i < o->a_ptr[n + 1]; ++i) {
      for (int32_t j = o->a_req_ptr[i]; j < o->a_req_ptr[i + 1]; ++j) {
        const int s = slot_of(n_slots, slot_res, o->a_req_res[j]);
        if (s >= 0 && slot_res[s] != SPX_RES_PODS) requested[s] += o->a_req_qty[j];
      }
    }
    for (int32_t s = 0; s < n_slots; ++s) {
      bool listed;
      const int64_t alloc = node_alloc(nodes, n, slot_res[s], &listed);
      int64_t left = 0;
      if (node_present[n] && listed) left = slot_res[s] == SPX_RES_PODS ? alloc - (o->a_ptr[n + 1] - o->a_ptr[n]) : alloc - requested[s];
      left_base[static_cast<size_t>(s) * static_cast<size_t>(N) + static_cast<size_t>(n)] = left;
    }
  }
  return SPX_OK;
}

extern "C" int spx_flatten_cosched_groups(const spx_node_objects* nodes, const spx_cosched_objects* o, int32_t n_slots, const int32_t* slot_res,
                                          int64_t step_cap, int64_t* n_steps_out, int64_t* req, uint32_t* req_mask, int32_t* step_ptr, int32_t* step_node,
                                          int64_t* step_add) {
  if (!groups_ok(o) || !assigned_ok(o) || !nodes_ok(nodes, o) || n_slots < 1 || n_slots > SPX_COSCHED_MAX_SLOTS || !slot_res || !n_steps_out) return SPX_ERR_ARG;
  const bool count_only = !step_node && !step_add;
  if (!count_only && (!req || !req_mask || !step_ptr || (step_cap > 0 && (!step_node || !step_add)))) return SPX_ERR_ARG;
  const int64_t N = o->n_nodes;
  const int32_t G = o->n_groups;
  const int pods_slot = slot_of(n_slots, slot_res, SPX_RES_PODS);
  if (pods_slot < 0) return SPX_ERR_ARG;
  // the steps of every group that reaches the resource check: (group, node) -> add-back per slot; nodes ascend as they are walked
  struct Step {
    int32_t node;
    int64_t add[SPX_COSCHED_MAX_SLOTS];
  };
  std::vector<std::vector<Step>> steps(static_cast<size_t>(G));
  for (int64_t n = 0; n < N; ++n) {
    if (!o->node_present[n]) continue;
    for (int32_t i = o->a_ptr[n]; i < o->a_ptr[n + 1]; ++i) {
      const int32_t g = o->a_group[i];
      if (g < 0 || !gated_by_resources(o, g)) continue;
      std::vector<Step>& sg = steps[static_cast<size_t>(g)];
      if (sg.empty() || sg.back().node != n) {
        Step st{};
        st.node = static_cast<int32_t>(n);
        sg.push_back(st);
      }
      Step& st = sg.back();
      st.add[pods_slot] += 1;
      for (int32_t j = o->a_req_ptr[i]; j < o->a_req_ptr[i + 1]; ++j) {
        const int s = slot_of(n_slots, slot_res, o->a_req_res[j]);
        if (s < 0 || s == pods_slot) continue;
        bool listed;
        (void)node_alloc(nodes, n, slot_res[s], &listed);
        if (listed) st.add[s] += o->a_req_qty[j];
      }
    }
  }
  int64_t total = 0;
  for (const auto& sg : steps) total += static_cast<int64_t>(sg.size());
  *n_steps_out = total;
  if (count_only) return SPX_OK;
  if (total > step_cap || total > INT32_MAX) return SPX_ERR_ARG;
  int32_t at = 0;
  for (int32_t g = 0; g < G; ++g) {
    step_ptr[g] = at;
    int64_t* rq = req + static_cast<size_t>(g) * static_cast<size_t>(n_slots);
    std::fill(rq, rq + n_slots, int64_t{0});
    req_mask[g] = 0;
    if (gated_by_resources(o, g)) {
      for (int32_t i = o->g_res_ptr[g]; i < o->g_res_ptr[g + 1]; ++i) {
        const int s = slot_of(n_slots, slot_res, o->g_res_id[i]);
        if (s < 0) return SPX_ERR_ARG;  // the slot list was built from other groups
        if (s == pods_slot) continue;   // overwritten by MinMember below
        rq[s] = o->g_res_qty[i];        // a name listed twice: the last entry stands, as in a map
        req_mask[g] |= 1u << s;
      }
      rq[pods_slot] = o->g_min_member[g];
      req_mask[g] |= 1u << pods_slot;
    }
    for (const Step& st : steps[static_cast<size_t>(g)]) {
      step_node[at] = st.node;
      std::copy(st.add, st.add + n_slots, step_add + static_cast<size_t>(at) * static_cast<size_t>(n_slots));
      ++at;
    }
  }
  step_ptr[G] = at;
  return SPX_OK;
}

extern "C" int spx_cosched_check(const spx_cosched_soa* t, int32_t* bad_slot) {
  if (bad_slot) *bad_slot = -1;
  if (!t || t->n_slots < 1 || t->n_slots > SPX_COSCHED_MAX_SLOTS || t->n_nodes < 0 || t->n_groups < 0) return SPX_ERR_ARG;
  if ((t->n_nodes && !t->left_base) || (t->n_groups && (!t->req || !t->req_mask || !t->step_ptr))) return SPX_ERR_ARG;
  const uint64_t limit = uint64_t{1} << 62;
  const int64_t n_steps = t->n_groups ? t->step_ptr[t->n_groups] : 0;
  if (n_steps && !t->step_add) return SPX_ERR_ARG;
  for (int32_t s = 0; s < t->n_slots; ++s) {
    uint64_t sum = 0;  // saturates at the limit: every term is below 2^63, the sum so far below 2^62
    bool over = false;
    for (int64_t n = 0; n < t->n_nodes && !over; ++n) {
      const uint64_t m = mag(t->left_base[static_cast<size_t>(s) * static_cast<size_t>(t->n_nodes) + static_cast<size_t>(n)]);
      over = m >= limit || (sum += m) >= limit;
    }
    for (int64_t k = 0; k < n_steps && !over; ++k) {
      const uint64_t m = mag(t->step_add[static_cast<size_t>(k) * static_cast<size_t>(t->n_slots) + static_cast<size_t>(s)]);
      over = m >= limit || (sum += m) >= limit;
    }
    for (int32_t g = 0; g < t->n_groups && !over; ++g)
      if ((t->req_mask[g] >> s) & 1u) over = mag(t->req[static_cast<size_t>(g) * static_cast<size_t>(t->n_slots) + static_cast<size_t>(s)]) >= limit;
    if (over) {
      if (bad_slot) *bad_slot = s;
      return SPX_ERR_ARG;
    }
  }
  return SPX_OK;
}

extern "C" int spx_cosched_less(const spx_cosched_objects* o, const int32_t* priority, const int64_t* initial_attempt_ns, const int64_t* key_ptr,
                                const uint8_t* key_bytes, int64_t n_pairs, const int64_t* a, const int64_t* b, uint8_t* less_out) {
  if (!o || o->n_pods < 0 || o->n_groups < 0 || n_pairs < 0) return SPX_ERR_ARG;
  if (n_pairs == 0) return SPX_OK;
  if (!priority || !initial_attempt_ns || !key_ptr || !a || !b || !less_out || !o->pod_group) return SPX_ERR_ARG;
  if (o->n_groups && (!o->g_exists || !o->g_created_ns || !o->g_has_last_failed || !o->g_last_failed_ns)) return SPX_ERR_ARG;
  // GetCreationTimestamp (core.go:368-384)
  auto created = [&](int64_t p) {
    const int32_t g = o->pod_group[p];
    if (g < 0) return initial_attempt_ns[p];
    if (o->g_has_last_failed[g]) return o->g_last_failed_ns[g];
    if (!o->g_exists[g]) return initial_attempt_ns[p];
    return o->g_created_ns[g];
  };
  for (int64_t i = 0; i < n_pairs; ++i) {
    const int64_t x = a[i], y = b[i];
    if (x < 0 || x >= o->n_pods || y < 0 || y >= o->n_pods) return SPX_ERR_ARG;
    if (o->pod_group[x] < -1 || o->pod_group[x] >= o->n_groups || o->pod_group[y] < -1 || o->pod_group[y] >= o->n_groups) return SPX_ERR_ARG;
    if (priority[x] != priority[y]) {
      less_out[i] = priority[x] > priority[y];
      continue;
    }
    const int64_t tx = created(x), ty = created(y);
    if (tx != ty) {
      less_out[i] = tx < ty;
      continue;
    }
    const int64_t lx = key_ptr[x + 1] - key_ptr[x], ly = key_ptr[y + 1] - key_ptr[y];
    if (lx < 0 || ly < 0 || ((lx || ly) && !key_bytes)) return SPX_ERR_ARG;
    const int64_t m = std::min(lx, ly);
    const int c = m ? std::memcmp(key_bytes + key_ptr[x], key_bytes + key_ptr[y], static_cast<size_t>(m)) : 0;  // Go compares strings bytewise
    less_out[i] = c < 0 || (c == 0 && lx < ly);
  }
  return SPX_OK;
}
