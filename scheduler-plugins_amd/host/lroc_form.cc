// lroc_form.cc — see lroc_form.hpp.
#include "lroc_form.hpp"

#include <limits>

#include "../../include/spx.h"

namespace spx_host {

int lroc_commit_form(const int64_t node_max[4], const int64_t pod_sum[4], int64_t alloc_max, bool limits_cover_requests) {
  uint64_t most = alloc_max < 0 ? std::numeric_limits<uint64_t>::max() : static_cast<uint64_t>(alloc_max);
  for (int c = 0; c < 4; ++c) {
    if (node_max[c] < 0 || pod_sum[c] < 0) return kLrocCommitI64;  // outside what a v1.Pod produces: the reference's own arithmetic
    const uint64_t b = static_cast<uint64_t>(node_max[c]) + static_cast<uint64_t>(pod_sum[c]);  // < 2^64: both below 2^63
    if (b > most) most = b;
  }
  if ((most >> 47) == 0 && limits_cover_requests) return kLrocCommitF32;
  if ((most >> 52) == 0) return kLrocCommitF64;
  return kLrocCommitI64;
}

}  // namespace spx_host

// test hook (not in spx.h): the selection above, reachable without a device
extern "C" int spx_internal_lroc_commit_form(const int64_t* node_max, const int64_t* pod_sum, int64_t alloc_max, int32_t limits_cover_requests) {
  if (!node_max || !pod_sum) return SPX_ERR_ARG;
  return spx_host::lroc_commit_form(node_max, pod_sum, alloc_max, limits_cover_requests != 0);
}
