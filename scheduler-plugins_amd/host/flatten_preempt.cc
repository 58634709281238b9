// flatten_preempt.cc — object tables -> spx_preempt_nodes_soa for the preemption dry run (host side, once per snapshot), and
// PodEligibleToPreemptOthers.
//
// What SelectVictimsOnNode (pkg/capacityscheduling/capacity_scheduling.go:486-677) does per (preemptor, node) and is the same for
// every preemptor is done here once per node:
//   the walk order, least important first (:537-539) and the most-important-first order of the reprieve (:625-627).  MoreImportantPod:
//     priority higher, else start time earlier.  sort.Slice is unstable; ties are broken by the order of the assigned-pod objects
//   computePodResourceRequest of every assigned and nominated pod (:865-882), formed as flatten_capacity.cc forms it
//   NodeInfo.Requested as the sum of what its pods charge
//   the PDBs that match a node's pods, renumbered per node in the order of the PDB list (filterPodsWithPDBViolation walks that list, :900)
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/spx.h"

namespace {

constexpr int S = SPX_QUOTA_SLOTS;
constexpr uint64_t kSumLimit = uint64_t{1} << 62;

struct Vec {
  int64_t v[S] = {0};
  uint8_t present = 0;
};

int slot_of(const spx_quota_objects* q, const spx_resource_classes* rc, int32_t res) {
  if (res == SPX_RES_CPU) return 0;
  if (res == SPX_RES_MEMORY) return 1;
  if (res == SPX_RES_EPHEMERAL) return 2;
  if (res == SPX_RES_PODS) return 3;
  if (!rc || res < 0 || res >= rc->n_res || !(rc->flags[res] & SPX_RC_SCALAR)) return -1;
  for (int s = 0; s < q->n_scalar_slots; ++s)
    if (q->scalar_res[s] == res) return 4 + s;
  return -2;
}

// framework.Resource.Add / SetMaxResource over one resource list; false: a scalar without a slot, or a negative quantity
bool apply(Vec& r, const spx_quota_objects* q, const spx_resource_classes* rc, const int32_t* res, const int64_t* qty, int32_t lo, int32_t hi, bool max_mode) {
  for (int32_t i = lo; i < hi; ++i) {
    const int s = slot_of(q, rc, res[i]);
    if (s == -2 || qty[i] < 0) return false;
    if (s < 0 || (max_mode && s == 3)) continue;
    if (max_mode) r.v[s] = qty[i] > r.v[s] ? qty[i] : r.v[s];
    else if ((r.v[s] += qty[i]) < 0 || static_cast<uint64_t>(r.v[s]) >= kSumLimit) return false;
    if (s >= 4) r.present |= static_cast<uint8_t>(1u << s);
  }
  return true;
}

bool pod_request(const spx_pod_objects* p, const spx_quota_objects* q, const spx_resource_classes* rc, int64_t pod, Vec& out) {
  out = Vec{};
  for (int32_t c = p->ctr_ptr[pod]; c < p->ctr_ptr[pod + 1]; ++c)
    if (p->ctr_kind[c] == SPX_CTR_APP && !apply(out, q, rc, p->req_res, p->req_qty, p->req_ptr[c], p->req_ptr[c + 1], false)) return false;
  for (int32_t c = p->ctr_ptr[pod]; c < p->ctr_ptr[pod + 1]; ++c)
    if (p->ctr_kind[c] != SPX_CTR_APP && !apply(out, q, rc, p->req_res, p->req_qty, p->req_ptr[c], p->req_ptr[c + 1], true)) return false;
  if (p->ovh_ptr && !apply(out, q, rc, p->ovh_res, p->ovh_qty, p->ovh_ptr[pod], p->ovh_ptr[pod + 1], false)) return false;
  return true;
}

}  // namespace

extern "C" int spx_flatten_preempt_nodes(const spx_node_objects* nodes, const spx_resource_classes* rc, const spx_quota_objects* q, const spx_preempt_objects* o,
                                         int64_t* n_pods_out, int64_t* n_nom_out, int64_t* n_pdb_out, int64_t* bad_out, uint8_t* present, int64_t* allocatable,
                                         int64_t* requested, int32_t* pod_ptr, int32_t* pod_src, int32_t* pod_priority, int64_t* pod_start, int32_t* pod_ns,
                                         int64_t* pod_fit_req, int64_t* pod_quota_req, uint8_t* pod_quota_req_present, uint8_t* pod_flags, uint32_t* pod_pdb_mask,
                                         int32_t* pod_hi_order, int32_t* nom_ptr, int32_t* nom_priority, int64_t* nom_fit_req, int64_t* nom_pending_row, int32_t* pdb_ptr,
                                         int32_t* pdb_allowed) {
  if (!nodes || !q || !o || !n_pods_out || !n_nom_out || !n_pdb_out || !bad_out) return SPX_ERR_ARG;
  const void* outs[] = {present,  allocatable,  requested,    pod_ptr,      pod_src,      pod_priority, pod_start,   pod_ns,          pod_fit_req, pod_quota_req, pod_quota_req_present,
                        pod_flags, pod_pdb_mask, pod_hi_order, nom_ptr,      nom_priority, nom_fit_req,  nom_pending_row, pdb_ptr,    pdb_allowed};
  size_t given = 0;
  for (const void* p : outs) given += p != nullptr;
  if (given != 0 && given != sizeof outs / sizeof *outs) return SPX_ERR_ARG;
  const bool fill = given != 0;
  const int64_t N = nodes->n_nodes, A = o->n_assigned, M = o->n_nominated;
  if (N <= 0 || A < 0 || M < 0 || o->n_pdbs < 0 || q->n_scalar_slots < 0 || q->n_scalar_slots > S - 4) return SPX_ERR_ARG;
  if (A > 0 && (!o->assigned || !o->assigned_node || !o->assigned_start_ns || !o->assigned_in_quota_set || !o->assigned_terminating || !o->assigned_pdb_ptr)) return SPX_ERR_ARG;
  if (M > 0 && (!o->nominated || !o->nominated_node || !o->nominated_pending_row)) return SPX_ERR_ARG;
  *bad_out = -1;
  auto on_node = [&](int64_t n) { return n >= 0 && n < N && (!o->node_present || o->node_present[n]); };
  std::vector<std::vector<int32_t>> pods_of(static_cast<size_t>(N)), noms_of(static_cast<size_t>(N));
  for (int64_t i = 0; i < A; ++i)
    if (on_node(o->assigned_node[i])) pods_of[o->assigned_node[i]].push_back(static_cast<int32_t>(i));
  for (int64_t i = 0; i < M; ++i)
    if (on_node(o->nominated_node[i])) noms_of[o->nominated_node[i]].push_back(static_cast<int32_t>(i));
  uint64_t total[S] = {0};
  auto account = [&](const int64_t* v) {  // the device's int64 sums: every slot's values stay below 2^62 in all
    for (int s = 0; s < S; ++s)
      if (v[s] < 0 || (total[s] += static_cast<uint64_t>(v[s])) >= kSumLimit) return false;
    return true;
  };
  int64_t at_pod = 0, at_nom = 0, at_pdb = 0;
  for (int64_t n = 0; n < N; ++n) {
    std::vector<int32_t>& list = pods_of[n];
    const int64_t L = static_cast<int64_t>(list.size());
    auto refuse = [&](int64_t what) {
      *bad_out = what;
      return SPX_ERR_ARG;
    };
    if (L > SPX_PREEMPT_MAX_NODE_PODS) return refuse(n);
    const spx_pod_objects* ap = o->assigned;
    // least important first; equal (priority, start time): the order of the objects (`list` ascends)
    std::stable_sort(list.begin(), list.end(), [&](int32_t x, int32_t y) {
      if (ap->priority[x] != ap->priority[y]) return ap->priority[x] < ap->priority[y];
      return o->assigned_start_ns[x] > o->assigned_start_ns[y];
    });
    std::vector<int32_t> hi(static_cast<size_t>(L));
    for (int64_t k = 0; k < L; ++k) hi[k] = static_cast<int32_t>(k);
    std::stable_sort(hi.begin(), hi.end(), [&](int32_t x, int32_t y) {
      if (ap->priority[list[x]] != ap->priority[list[y]]) return ap->priority[list[x]] > ap->priority[list[y]];
      return o->assigned_start_ns[list[x]] < o->assigned_start_ns[list[y]];
    });
    // the PDBs that match a pod of this node, ascending = the order of the PDB list
    std::vector<int32_t> local;
    for (int32_t i : list)
      for (int32_t k = o->assigned_pdb_ptr[i]; k < o->assigned_pdb_ptr[i + 1]; ++k) {
        if (o->assigned_pdb[k] < 0 || o->assigned_pdb[k] >= o->n_pdbs) return refuse(n);
        local.push_back(o->assigned_pdb[k]);
      }
    std::sort(local.begin(), local.end());
    local.erase(std::unique(local.begin(), local.end()), local.end());
    if (local.size() > SPX_PREEMPT_MAX_NODE_PDBS) return refuse(n);
    Vec alloc, req_sum;
    alloc.v[0] = nodes->alloc_cpu_milli[n], alloc.v[1] = nodes->alloc_mem[n], alloc.v[2] = nodes->alloc_eph[n], alloc.v[3] = nodes->alloc_pods[n];
    if (nodes->scalar_ptr)
      for (int32_t k = nodes->scalar_ptr[n]; k < nodes->scalar_ptr[n + 1]; ++k) {
        const int s = slot_of(q, rc, nodes->scalar_res[k]);
        if (s >= 4) alloc.v[s] = nodes->scalar_qty[k];  // a scalar without a quota slot: no pod of the tables can request it
      }
    if (!account(alloc.v)) return refuse(n);
    if (fill) {
      present[n] = on_node(n);
      pod_ptr[n] = static_cast<int32_t>(at_pod), nom_ptr[n] = static_cast<int32_t>(at_nom), pdb_ptr[n] = static_cast<int32_t>(at_pdb);
      std::memcpy(allocatable + n * S, alloc.v, sizeof alloc.v);
    }
    for (int64_t k = 0; k < L; ++k) {
      const int32_t i = list[k];
      Vec r;
      if (!pod_request(ap, q, rc, i, r)) return refuse(-1 - i);
      Vec f = r;
      f.v[3] = 1;
      if (!account(r.v) || !account(f.v)) return refuse(n);
      for (int s = 0; s < S; ++s) req_sum.v[s] += f.v[s];
      if (!fill) continue;
      const int64_t j = at_pod + k;
      uint32_t mask = 0;
      for (int32_t m = o->assigned_pdb_ptr[i]; m < o->assigned_pdb_ptr[i + 1]; ++m)
        mask |= 1u << (std::lower_bound(local.begin(), local.end(), o->assigned_pdb[m]) - local.begin());
      pod_src[j] = i, pod_priority[j] = ap->priority[i], pod_start[j] = o->assigned_start_ns[i], pod_ns[j] = ap->ns[i];
      std::memcpy(pod_fit_req + j * S, f.v, sizeof f.v);
      std::memcpy(pod_quota_req + j * S, r.v, sizeof r.v);
      pod_quota_req_present[j] = r.present;
      pod_flags[j] = static_cast<uint8_t>((o->assigned_in_quota_set[i] ? SPX_PREEMPT_POD_IN_QUOTA_SET : 0) | (o->assigned_terminating[i] ? SPX_PREEMPT_POD_TERMINATING : 0));
      pod_pdb_mask[j] = mask;
      pod_hi_order[j] = hi[k];
    }
    if (!account(req_sum.v)) return refuse(n);
    if (fill) std::memcpy(requested + n * S, req_sum.v, sizeof req_sum.v);
    for (size_t k = 0; k < noms_of[n].size(); ++k) {
      const int32_t i = noms_of[n][k];
      Vec r;
      if (!pod_request(o->nominated, q, rc, i, r)) return refuse(n);
      r.v[3] = 1;
      if (!account(r.v)) return refuse(n);
      if (!fill) continue;
      nom_priority[at_nom + k] = o->nominated->priority[i];
      nom_pending_row[at_nom + k] = o->nominated_pending_row[i];
      std::memcpy(nom_fit_req + (at_nom + k) * S, r.v, sizeof r.v);
    }
    if (fill)
      for (size_t k = 0; k < local.size(); ++k) pdb_allowed[at_pdb + k] = o->pdb_allowed[local[k]];
    at_pod += L, at_nom += static_cast<int64_t>(noms_of[n].size()), at_pdb += static_cast<int64_t>(local.size());
  }
  if (fill) pod_ptr[N] = static_cast<int32_t>(at_pod), nom_ptr[N] = static_cast<int32_t>(at_nom), pdb_ptr[N] = static_cast<int32_t>(at_pdb);
  *n_pods_out = at_pod, *n_nom_out = at_nom, *n_pdb_out = at_pdb;
  return SPX_OK;
}

// The nominated records of spx_flatten_preempt_nodes' table again, with what CapacityScheduling's sequential loop reads of them beyond
// the node charge: the namespace and computePodResourceRequest.  Same order: node by node, the objects' order within a node.
extern "C" int spx_flatten_preempt_nominated_quota(const spx_node_objects* nodes, const spx_resource_classes* rc, const spx_quota_objects* q, const spx_preempt_objects* o,
                                                   int64_t n_nom, int32_t* nom_src, int32_t* ns, int64_t* quota_req, uint8_t* quota_req_present) {
  if (!nodes || !q || !o || n_nom < 0 || nodes->n_nodes <= 0 || o->n_nominated < 0 || q->n_scalar_slots < 0 || q->n_scalar_slots > S - 4) return SPX_ERR_ARG;
  if (o->n_nominated > 0 && (!o->nominated || !o->nominated_node)) return SPX_ERR_ARG;
  if (n_nom > 0 && (!ns || !quota_req || !quota_req_present)) return SPX_ERR_ARG;
  const int64_t N = nodes->n_nodes, M = o->n_nominated;
  auto on_node = [&](int64_t n) { return n >= 0 && n < N && (!o->node_present || o->node_present[n]); };
  std::vector<int32_t> at(static_cast<size_t>(N) + 1, 0);  // records per node, then where each node's records start
  for (int64_t i = 0; i < M; ++i)
    if (on_node(o->nominated_node[i])) ++at[o->nominated_node[i] + 1];
  for (int64_t n = 0; n < N; ++n) at[n + 1] += at[n];
  if (at[N] != n_nom) return SPX_ERR_ARG;
  for (int64_t i = 0; i < M; ++i) {
    if (!on_node(o->nominated_node[i])) continue;
    const int64_t j = at[o->nominated_node[i]]++;
    Vec r;
    if (!pod_request(o->nominated, q, rc, i, r)) return SPX_ERR_ARG;
    if (nom_src) nom_src[j] = static_cast<int32_t>(i);
    ns[j] = o->nominated->ns[i];
    std::memcpy(quota_req + j * S, r.v, sizeof r.v);
    quota_req_present[j] = r.present;
  }
  return SPX_OK;
}

// PodEligibleToPreemptOthers, capacity_scheduling.go:409-484
extern "C" int spx_preempt_eligible(const spx_preempt_nodes_soa* t, const spx_quota_objects* q, const uint8_t* over_min, int64_t n, const int32_t* ns,
                                    const int32_t* priority, const uint8_t* preempt_never, const int64_t* nominated_node, const uint8_t* nominated_unresolvable,
                                    const uint8_t* more_than_min, uint8_t* eligible_out) {
  if (!t || !q || n < 0 || !t->present || !t->pod_ptr || (n > 0 && (!ns || !priority || !preempt_never || !nominated_node || !nominated_unresolvable || !more_than_min || !eligible_out)))
    return SPX_ERR_ARG;
  if (q->n_namespaces > 0 && (!q->has_quota || !over_min)) return SPX_ERR_ARG;
  auto with_eq = [&](int32_t k) { return k >= 0 && k < q->n_namespaces && q->has_quota[k]; };
  for (int64_t i = 0; i < n; ++i) {
    eligible_out[i] = 0;
    if (preempt_never[i]) continue;  // :412-415
    eligible_out[i] = 1;
    const int64_t node = nominated_node[i];
    if (node < 0 || nominated_unresolvable[i]) continue;  // :425, :428-430
    if (node >= t->n_nodes) return SPX_ERR_ARG;
    if (!t->present[node]) continue;  // nodeInfo == nil, :439-441
    const bool pre_eq = with_eq(ns[i]);
    for (int32_t j = t->pod_ptr[node]; j < t->pod_ptr[node + 1] && eligible_out[i]; ++j) {
      if (!(t->pod_flags[j] & SPX_PREEMPT_POD_TERMINATING)) continue;
      const int32_t pns = t->pod_ns[j];
      if (pre_eq) {
        if (!with_eq(pns)) continue;
        if (pns == ns[i] ? t->pod_priority[j] < priority[i] : (!more_than_min[i] && over_min[pns])) eligible_out[i] = 0;  // :454-467
      } else if (!with_eq(pns) && t->pod_priority[j] < priority[i]) {
        eligible_out[i] = 0;  // :476-479
      }
    }
  }
  return SPX_OK;
}
