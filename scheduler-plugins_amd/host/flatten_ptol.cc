// flatten_ptol.cc — PriorityClass objects + the assigned pods' class names and PodScheduled conditions -> spx_preempt_toleration_soa
// for PreemptionToleration's dry run (host side, once per snapshot), and its PodEligibleToPreemptOthers.
//
// ExemptedFromPreemption (pkg/preemptiontoleration/preemption_toleration.go:129-181) asks, per (victim candidate, preemptor):
//   :136      PriorityClassName empty                          -> not exempted          flags 0
//   :139-142  the class is not in the lister                   -> error                 SPX_PTOL_POD_CLASS_MISSING
//   :148-150  the preemptor is PreemptNever                    -> exempted              SPX_PTOL_POD_HAS_CLASS (the device knows the preemptor)
//   :153-162  the policy does not parse                        -> not exempted          min_preemptable = INT32_MIN: no priority is below it
//   :164      preemptorPriority >= MinimumPreemptablePriority  -> not exempted          min_preemptable
//   :168      TolerationSeconds < 0                            -> exempted              exempt_until_ns = INT64_MAX
//   :173-176  no PodScheduled=True condition                   -> exempted              exempt_until_ns = INT64_MAX
//   :177-180  scheduledAt.Add(TolerationSeconds * time.Second).After(now)               exempt_until_ns = that instant
// time.Duration(TolerationSeconds) * time.Second is an int64 product and wraps; Time.Add does not, so the sum is formed wide and clamped.
#include <cstdint>
#include <cstring>

#include "../../include/spx.h"

namespace {

// strconv.ParseInt(s, 10, bits): one optional '+' or '-', then decimal digits only (underscores belong to base 0), and a value inside
// the bit size's range; everything else is an error (the clamped value Go returns with a range error is never used by the caller)
bool parse_int(const char* s, int bits, int64_t* out) {
  if (!s || !*s) return false;
  const bool neg = *s == '-';
  if (*s == '+' || *s == '-') ++s;
  if (!*s) return false;
  const uint64_t limit = (uint64_t{1} << (bits - 1)) - (neg ? 0 : 1);  // |min| or max of the bit size
  uint64_t v = 0;
  for (; *s; ++s) {
    if (*s < '0' || *s > '9') return false;
    const uint64_t d = static_cast<uint64_t>(*s - '0');
    if (v > (limit - d) / 10) return false;  // v * 10 + d > limit
    v = v * 10 + d;
  }
  *out = neg ? static_cast<int64_t>(~v + 1) : static_cast<int64_t>(v);
  return true;
}

struct Policy {
  bool ok;
  int32_t min_preemptable;
  int64_t toleration_seconds;
};

// parsePreemptionTolerationPolicy, preemption_toleration_policy.go:55-83
Policy parse_policy(const spx_priority_classes* c, int32_t k) {
  Policy p{true, 0, 0};
  const char* mp = c->minimum_preemptable_priority ? c->minimum_preemptable_priority[k] : nullptr;
  const char* ts = c->toleration_seconds ? c->toleration_seconds[k] : nullptr;
  int64_t v = 0;
  if (!mp) p.min_preemptable = static_cast<int32_t>(static_cast<uint32_t>(c->value[k]) + 1u);  // pc.Value + 1 in int32
  else if (parse_int(mp, 32, &v)) p.min_preemptable = static_cast<int32_t>(v);
  else p.ok = false;
  if (ts && !parse_int(ts, 64, &p.toleration_seconds)) p.ok = false;
  return p;
}

}  // namespace

extern "C" int spx_flatten_preempt_toleration(const spx_priority_classes* classes, int64_t n_assigned, const int32_t* pod_class, const uint8_t* pod_scheduled,
                                              const int64_t* pod_scheduled_at_ns, int64_t n_pods, const int32_t* pod_src, int32_t* min_preemptable,
                                              int64_t* exempt_until_ns, uint8_t* flags) {
  if (!classes || classes->n_classes < 0 || n_assigned < 0 || n_pods < 0) return SPX_ERR_ARG;
  if (classes->n_classes > 0 && (!classes->present || !classes->value)) return SPX_ERR_ARG;
  if (n_pods > 0 && (!pod_class || !pod_scheduled || !pod_scheduled_at_ns || !pod_src || !min_preemptable || !exempt_until_ns || !flags)) return SPX_ERR_ARG;
  for (int64_t j = 0; j < n_pods; ++j) {
    const int64_t i = pod_src[j];
    if (i < 0 || i >= n_assigned) return SPX_ERR_ARG;
    const int32_t k = pod_class[i];
    if (k < -1 || k >= classes->n_classes) return SPX_ERR_ARG;
    min_preemptable[j] = 0, exempt_until_ns[j] = 0, flags[j] = 0;
    if (k < 0) continue;
    if (!classes->present[k]) {
      flags[j] = SPX_PTOL_POD_CLASS_MISSING;
      continue;
    }
    flags[j] = SPX_PTOL_POD_HAS_CLASS;
    const Policy p = parse_policy(classes, k);
    if (!p.ok) {
      min_preemptable[j] = INT32_MIN;
      continue;
    }
    min_preemptable[j] = p.min_preemptable;
    if (p.toleration_seconds < 0 || !pod_scheduled[i]) {
      exempt_until_ns[j] = INT64_MAX;
      continue;
    }
    const int64_t d = static_cast<int64_t>(static_cast<uint64_t>(p.toleration_seconds) * uint64_t{1000000000});  // the Duration, wrapped
    const __int128 until = static_cast<__int128>(pod_scheduled_at_ns[i]) + d;
    exempt_until_ns[j] = until > INT64_MAX ? INT64_MAX : until < INT64_MIN ? INT64_MIN : static_cast<int64_t>(until);
  }
  return SPX_OK;
}

// PodEligibleToPreemptOthers, preemption_toleration.go:339-364
extern "C" int spx_preempt_toleration_eligible(const spx_preempt_nodes_soa* t, int64_t n, const int32_t* priority, const uint8_t* preempt_never,
                                               const int64_t* nominated_node, const uint8_t* nominated_unresolvable, uint8_t* eligible_out) {
  if (!t || n < 0 || !t->present || !t->pod_ptr || (n > 0 && (!priority || !preempt_never || !nominated_node || !nominated_unresolvable || !eligible_out)))
    return SPX_ERR_ARG;
  for (int64_t i = 0; i < n; ++i) {
    eligible_out[i] = 0;
    if (preempt_never[i]) continue;  // :341-344
    eligible_out[i] = 1;
    const int64_t node = nominated_node[i];
    if (node < 0 || nominated_unresolvable[i]) continue;  // :347, :350-352
    if (node >= t->n_nodes) return SPX_ERR_ARG;
    if (!t->present[node]) continue;  // nodeInfo == nil, :354
    for (int32_t j = t->pod_ptr[node]; j < t->pod_ptr[node + 1]; ++j)
      if ((t->pod_flags[j] & SPX_PREEMPT_POD_TERMINATING) && t->pod_priority[j] < priority[i]) eligible_out[i] = 0;  // :356-360
  }
  return SPX_OK;
}
