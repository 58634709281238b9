// lroc_cell.h — LowRiskOverCommitment's arithmetic of ONE (pod, node) cell: the one copy that the table sweeps (kernels_lroc.hip:
// k_lroc, k_lroc_fast) and the sequential commit loop's single-row sweep (kernels_commit_scorers.hip) evaluate a cell with.  What
// is theirs is the grid, where the node's and the pod's numbers come from and how the bytes are stored.
//
// Everything is in the anonymous namespace: each translation unit gets its own copy (as nrt_ref_device.h).
//
// Reference: lowriskovercommitment.go:158-255, resourcestats.go:163-225.  The float32 form's derivation and its error budget:
// kernels_lroc.hip's header and DESIGN.md 3.8.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spx {
namespace {

typedef float F32x2 __attribute__((ext_vector_type(2)));

// totalRisk of one resource (lowriskovercommitment.go:205-208, :250-253) given (1-w)*riskLoad
__device__ __forceinline__ double total_risk(double w, double kl, double node_req, double node_lim, double cap, double pod_req, double pod_lim) {
  const double limit = node_lim + pod_lim;                        // resourcestats.go:204-205
  const double request = fmin(node_req + pod_req, cap);           // :202-203, :208-209
  const double over = limit - cap;
  const double risk_limit = over > 0.0 ? over / (limit - request) : 0.0;
  const double total = w * risk_limit + kl;
  return fmax(fmin(total, 1.0), 0.0);
}
__device__ __forceinline__ double total_risk(double w, double kl, int64_t node_req, int64_t node_lim, int64_t cap, int64_t pod_req, int64_t pod_lim) {
  const int64_t limit = node_lim + pod_lim;
  int64_t request = node_req + pod_req;
  if (request > cap) request = cap;
  const double risk_limit = limit > cap ? static_cast<double>(limit - cap) / static_cast<double>(limit - request) : 0.0;
  const double total = w * risk_limit + kl;
  return fmax(fmin(total, 1.0), 0.0);
}

__device__ __forceinline__ uint32_t score_byte(bool has, double risk_c, double risk_m) {
  const double rank = 1 - fmax(risk_c, risk_m);                   // :165
  const int v = static_cast<int>(round(rank * 100.0));            // :136-137
  return has ? static_cast<uint32_t>(v < 0 ? 0 : (v > 100 ? 100 : v)) : 0u;
}

// The float32 form of a cell (cpu in .x, memory in .y).  Per node: A = limits - capacity as the sum of two float32 (Ah, Al),
// D = limits - requests held at >= 2^-30, kl = (1 - w) * riskLoad; per pod: its limit as two float32 (plh, pll) and limit - request
// (df); w2 = the two RiskLimitWeights.  Returns the bits of 2^23 + (100 * (1 - max risk) + 1/2 + band) in units of 2^-16: byte 2 is the
// score, and the low 16 bits below 2 * kLrocBandUnits mean "within the band of a rounding boundary k + 1/2" (lroc_cell_near).
constexpr float kLrocMagic = 8388608.0f;   // 2^23: a sum in [2^23, 2^24) is a whole number, and the mantissa bits are that number - 2^23
constexpr float kLrocScale = 6553600.0f;   // 100 * 2^16
constexpr float kLrocBandUnits = 8.0f;     // the band around k + 1/2 in units of 2^-16: 1.22e-4 (float32 error of the score < 8.7e-5)
__device__ __forceinline__ uint32_t lroc_cell_f32(F32x2 Ah, F32x2 Al, F32x2 D, F32x2 kl, F32x2 plh, F32x2 pll, F32x2 df, F32x2 w2) {
  // riskLimit = over / max(D + d, over) for over > 0, else 0  ==  clamp(over / (D + d), 0, 1): over exact, then float32
  // (high parts, low parts, then both: the high sum is exact whenever it cancels, the low sum always — within 3 ulp of A + limit)
  const F32x2 ov = (Ah + plh) + (Al + pll);
  const F32x2 dd = D + df;
  const float rr = __builtin_amdgcn_rcpf(dd.x * dd.y);  // one reciprocal for both quotients
  const F32x2 x = ov * __builtin_shufflevector(dd, dd, 1, 0);
  F32x2 qq, r2;
  r2.x = rr;  // (.y is not read: op_sel_hi takes the low half for both products)
  // (inline: the compiler has no packed clamp pattern; s_nop: the wait state a transcendental's consumer needs, which the
  // hazard pass cannot add inside an asm statement)
  asm("s_nop 0\n\tv_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0] clamp" : "=v"(qq) : "v"(x), "v"(r2));  // both quotients, clamped to [0, 1] (NaN cannot occur: rr and x are finite or x is an infinity)
  const F32x2 t2 = __builtin_elementwise_fma(w2, qq, kl);
  const float t_c = t2.x, t_m = t2.y;
  const float m = __builtin_amdgcn_fmed3f(__builtin_fmaxf(t_c, t_m), 0.0f, 1.0f);  // totalRisk's clamp (:252), after the max
  // 100 * (1 - max risk) in units of 2^-16, + 1/2 + the band, rounded to a whole number by the sum with 2^23 (the fma rounds once):
  // the mantissa then reads  score << 16 | fraction,  and a fraction below 2 * kLrocBandUnits means "within the band of k + 1/2"
  const float k = __builtin_fmaf(m, -kLrocScale, kLrocMagic + kLrocScale + 32768.0f + kLrocBandUnits);
  return __float_as_uint(k);
}
__device__ __forceinline__ bool lroc_cell_near(uint32_t kb) { return (kb & (0xffffu & ~(2u * static_cast<uint32_t>(kLrocBandUnits) - 1u))) == 0u; }

}  // namespace
}  // namespace spx
