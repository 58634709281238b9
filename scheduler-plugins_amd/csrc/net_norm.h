// net_norm.h — NetworkOverhead's NormalizeScore (networkoverhead.go:389-418), once for every kernel that runs it: the sweeps of
// net_device.h / kernels_network.hip / kernels_network_wide.hip and the cooperative sequential commit (kernels_commit_coop.hip).
//
// The reference computes int64(100.0 * float64(s - min) / float64(max - min)).  For 0 <= d <= r < 2^31 that equals the integer
// quotient (100 * d) / r: a non-integer 100*d/r lies at least 1/r > 2^-31 from the next integer, the float64 quotient (one rounding: 100 * d is exact)
// is within a relative 2^-53 of it (tests/test_exactness_arguments.py).  The claim is about the quotient, not about the width of the product:
// 100 * d needs up to 38 bits, and fits 32 only while r < 2^31 / 100.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace spx {

namespace {

// NormalizeScore operation for operation: 100.0 * float64(s - min) / float64(max - min), truncated; min == max: float64(s - min);
// min == max == 0: untouched.  Returned as the score byte.  A scored node has min <= s <= max, so norm lies in [0, 100]; the
// differences wrap and norm is fenced for the cells outside that (nodes another Filter plugin rejected, a row without a feasible
// node): their byte is never stored as a score.
__device__ __forceinline__ int norm_cost_f64(int64_t cost, int64_t mn, int64_t mx) {
  int64_t s = cost;
  if (!(mn == 0 && mx == 0)) {
    const int64_t d = static_cast<int64_t>(static_cast<uint64_t>(cost) - static_cast<uint64_t>(mn));
    const int64_t r = static_cast<int64_t>(static_cast<uint64_t>(mx) - static_cast<uint64_t>(mn));
    double norm = r != 0 ? 100.0 * static_cast<double>(d) / static_cast<double>(r) : static_cast<double>(d);
    norm = norm < -1000.0 ? -1000.0 : (norm > 1000.0 ? 1000.0 : norm);
    s = 100 - static_cast<int64_t>(norm);
  }
  return s < 0 ? 0 : (s > 255 ? 255 : static_cast<int>(s));
}

// the largest range whose product 100 * d (d <= range) fits int32: 100 * 21 474 836 = 2 147 483 600 < 2^31
constexpr int kNormNarrowRange = 21474836;

// NormalizeScore of the 32-bit sweeps (costs below 2^31), returned as the score byte.  While the range is small enough for a
// 32-bit product the quotient is one integer division; above that (costs in microseconds or bytes/s) it is the reference's own
// float64 sequence.  The branch depends on the cell only through d's position in [0, range], which holds for every scored cell:
// it is uniform over a row's scored cells.
__device__ __forceinline__ int norm_cost(int cost, int mn, int mx) {
  const unsigned d = static_cast<unsigned>(cost) - static_cast<unsigned>(mn), range = static_cast<unsigned>(mx) - static_cast<unsigned>(mn);
  if (range - 1u < static_cast<unsigned>(kNormNarrowRange) && d <= range) return 100 - static_cast<int>((100u * d) / range);
  return norm_cost_f64(cost, mn, mx);
}

}  // namespace

}  // namespace spx
