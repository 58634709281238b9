// nrt_release.hpp — what one evicted pod gives back to its node's NUMA zones (preemption.go:56-110, resourcerequests/exclusive.go:78-102):
// the one copy of the per-pod rule that spx_nrt_post_eviction (nrt_preemption.cc) and spx_flatten_preempt_nrt (flatten_preempt_nrt.cc)
// share, and the pod's QoS class as the Filter and the simulation read it (also flatten_nrt.cc's).
//
// Only app containers count; a pod that is neither Guaranteed nor requests a non-native resource (any container, init ones included)
// gives nothing; a container gives to the NUMA node the placement info pins it to (none / unknown: skipped); per request only what was
// exclusively assigned: extended resources the NRT reports, whole cpus and memory / hugepages of Guaranteed pods.
#pragma once

#include <cstdint>

#include "../../include/spx.h"

namespace spx_host {

inline bool nrt_native(const spx_resource_classes* rc, int32_t res) {
  if (res == SPX_RES_CPU || res == SPX_RES_MEMORY || res == SPX_RES_EPHEMERAL || res == SPX_RES_PODS || res == SPX_RES_STORAGE) return true;
  return rc != nullptr && res >= 0 && res < rc->n_res && (rc->flags[res] & SPX_RC_NATIVE) != 0;
}
inline bool nrt_hugepage(const spx_resource_classes* rc, int32_t res) {
  return rc != nullptr && res >= SPX_RES_FIRST_DYNAMIC && res < rc->n_res && (rc->flags[res] & SPX_RC_HUGEPAGE) != 0;
}

// v1qos.ComputePodQOS restated for the fields the hot path reads (cpu, memory; zero quantities ignored)
inline int nrt_pod_qos(const spx_pod_objects* p, int64_t pod) {
  int64_t req[2] = {0, 0}, lim[2] = {0, 0};
  bool has_req[2] = {false, false}, has_lim[2] = {false, false};
  bool guaranteed = true;
  for (int32_t c = p->ctr_ptr[pod]; c < p->ctr_ptr[pod + 1]; ++c) {
    for (int32_t i = p->req_ptr[c]; i < p->req_ptr[c + 1]; ++i) {
      const int32_t r = p->req_res[i];
      if ((r == SPX_RES_CPU || r == SPX_RES_MEMORY) && p->req_qty[i] > 0) {
        req[r] += p->req_qty[i];
        has_req[r] = true;
      }
    }
    bool found[2] = {false, false};
    for (int32_t i = p->lim_ptr[c]; i < p->lim_ptr[c + 1]; ++i) {
      const int32_t r = p->lim_res[i];
      if ((r == SPX_RES_CPU || r == SPX_RES_MEMORY) && p->lim_qty[i] > 0) {
        lim[r] += p->lim_qty[i];
        has_lim[r] = found[r] = true;
      }
    }
    if (!(found[0] && found[1])) guaranteed = false;
  }
  if (!has_req[0] && !has_req[1] && !has_lim[0] && !has_lim[1]) return SPX_QOS_BESTEFFORT;
  if (guaranteed)
    for (int r = 0; r < 2; ++r)
      if (has_req[r] && (!has_lim[r] || lim[r] != req[r])) guaranteed = false;
  if (guaranteed && (int(has_req[0]) + int(has_req[1])) == (int(has_lim[0]) + int(has_lim[1]))) return SPX_QOS_GUARANTEED;
  return SPX_QOS_BURSTABLE;
}

// give(numa, res, qty) for every exclusive request of pod v's placed app containers, in container and request order; reported(res):
// cache.ResourceNamesFromNRT of the node.  ctr_numa: per container of `pods` in CSR order.  Returns whether give was called at all:
// the pod then contributes to the simulation, whether or not the node has that zone or resource.
template <class Reported, class Give>
bool nrt_pod_releases(const spx_resource_classes* rc, const spx_pod_objects* pods, int64_t v, int qos, const int32_t* ctr_numa, Reported reported, Give give) {
  bool non_native = false;  // resourcerequests.IncludeNonNative: any container, init ones included
  for (int32_t c = pods->ctr_ptr[v]; c < pods->ctr_ptr[v + 1] && !non_native; ++c)
    for (int32_t i = pods->req_ptr[c]; i < pods->req_ptr[c + 1]; ++i)
      if (!nrt_native(rc, pods->req_res[i])) {
        non_native = true;
        break;
      }
  if (qos != SPX_QOS_GUARANTEED && !non_native) return false;
  bool any = false;
  for (int32_t c = pods->ctr_ptr[v]; c < pods->ctr_ptr[v + 1]; ++c) {
    if (pods->ctr_kind[c] != SPX_CTR_APP || ctr_numa[c] < 0) continue;
    for (int32_t i = pods->req_ptr[c]; i < pods->req_ptr[c + 1]; ++i) {
      const int32_t res = pods->req_res[i];
      const int64_t q = pods->req_qty[i];
      bool exclusive;
      if (!nrt_native(rc, res)) exclusive = reported(res);
      else if (qos != SPX_QOS_GUARANTEED) exclusive = false;
      else if (res == SPX_RES_CPU) exclusive = q > 0 && q % 1000 == 0;
      else exclusive = (res == SPX_RES_MEMORY || nrt_hugepage(rc, res)) && q > 0;
      if (!exclusive) continue;
      give(ctr_numa[c], res, q);
      any = true;
    }
  }
  return any;
}

}  // namespace spx_host
