// peaks_cell.h — Peaks' arithmetic of ONE (pod, node) cell before NormalizeScore: the one copy that the table sweeps
// (kernels_peaks.hip) and the sequential commit loop's single-row sweep (kernels_commit_scorers.hip) compute a raw score with.
//
// Everything is in the anonymous namespace: each translation unit gets its own copy (as nrt_ref_device.h).
//
// Reference: peaks.go:103-144, :186-196.
#pragma once

#include <hip/hip_runtime.h>

#include "spx_internal.h"

namespace spx {
namespace {

// a / b correctly rounded from y = RN(1/b): q = RN(a*y) is within an ulp of the quotient, the residual a - b*q is exact in
// one fma, and RN(q + r*y) is RN(a/b) (Markstein's theorem; the exception, a divisor whose significand is all ones, cannot
// occur for the integer-valued divisors used here).  Three full-rate instructions instead of the ~14 of the IEEE division
// sequence; tests/test_exactness_arguments.py replays it against true division in exact rational arithmetic.
__device__ __forceinline__ double div_rn(double a, double b, double y) {
  const double q = a * y;
  const double r = fma(-b, q, a);
  return fma(r, y, q);
}

struct NodeP {
  double cap;       // float64(node.Status.Capacity.Cpu().MilliValue())   peaks.go:132
  double rcap;      // RN(1 / cap), for div_rn
  double util_m;    // (util / 100) * cap                                  :133
  double k1, k2;    // power model                                          :190-196
  double e_now;     // exp(K2 * util)                                       :187
  bool valid;       // metrics present and a CPU AVG/Latest metric found   :108-131
};

__device__ __forceinline__ NodeP load_node(const PeaksArgs& a, int64_t n) {
  NodeP nd;
  const bool in = n < a.n_nodes;
  nd.valid = in && a.valid[n] != 0;
  nd.cap = in ? static_cast<double>(a.cap_cpu_milli[n]) : 0.0;
  const double util = in ? a.cpu_util[n] : 0.0;
  nd.rcap = 1.0 / nd.cap;
  nd.util_m = (util / 100) * nd.cap;
  nd.k1 = in ? a.k1[n] : 0.0;
  nd.k2 = in ? a.k2[n] : 0.0;
  nd.e_now = exp(nd.k2 * util);
  return nd;
}

// Peaks.Score for one node given float64(curPodCPUUsage), as an integer-valued float64: int64(x) truncates toward zero and
// |x| < 2^63 here, so trunc(x) is that int64 exactly (a float64 at or above 2^53 is an integer already).  Staying in float64
// saves the two multi-instruction conversions per cell; differences of two such values taken in float64 are the correctly
// rounded exact difference, i.e. the very float64(score - minCost) the reference forms (peaks.go:158).
__device__ __forceinline__ double raw_score(const NodeP& nd, double pod_cpu) {
  double predicted = 0.0;
  if (nd.cap != 0) predicted = div_rn(100 * (nd.util_m + pod_cpu), nd.cap, nd.rcap);  // :135-138
  const double jump = nd.k1 * (exp(nd.k2 * predicted) - nd.e_now);     // :186-188
  const double v = trunc(jump * 1e15);                                 // :143
  return (nd.valid && !(predicted > 100)) ? v : 0.0;                   // :108-112, :128-131, :139-140
}

}  // namespace
}  // namespace spx
