// lroc_form.hpp — which form of LowRiskOverCommitment's sweep a sequential commit of a batch may run (spx_commit.hip).  Plain host
// code: tests reach it through spx_internal_lroc_commit_form.
#pragma once

#include <stdint.h>

namespace spx_host {

constexpr int kLrocCommitI64 = 0, kLrocCommitF32 = 1, kLrocCommitF64 = 2;  // (spx::kLrocForm* of spx_internal.h)

// A commit adds a bound pod's four numbers to its node's four sums, so after ANY sequence of commits of the batch a sum stays at or
// below (largest node value of the column) + (sum of the batch's pod column).  Per column c of {req cpu, req mem, lim cpu, lim mem}:
// node_max[c] and pod_sum[c], both >= 0 (a sum that does not fit int64 is passed as INT64_MAX).  alloc_max: the largest allocatable
// value the sweep reads.  limits_cover_requests: no node sum and no pod has a limit below its request — commits preserve it (pod
// limits are raised to the requests).
//   every bound and alloc_max below 2^47, limits_cover_requests  -> float32 form (values and differences are sums of two float32)
//   below 2^52                                                   -> float64 form (sums and differences exact)
//   otherwise                                                    -> int64 form
int lroc_commit_form(const int64_t node_max[4], const int64_t pod_sum[4], int64_t alloc_max, bool limits_cover_requests);

}  // namespace spx_host
