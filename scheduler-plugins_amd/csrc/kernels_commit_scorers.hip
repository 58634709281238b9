// kernels_commit_scorers.hip — LowRiskOverCommitment and Peaks inside the sequential commit loop (spx_commit.hip, per-pod route).
//
// The loop evaluates ONE pod row per step on the current device tables; the table sweeps of kernels_lroc.hip / kernels_peaks.hip put
// one wave on a row (a wave owns 256-512 nodes x 64 pods).  Here a whole workgroup walks the row, loops striding by the block size,
// and the row index comes from the device counter the replayed graph advances (SPX_RESOLVE_ROWS) — as k_alloc_masked, k_net_cls and
// k_best were treated.  The cell arithmetic is the sweeps' own (lroc_cell.h, peaks_cell.h): same bytes.
//
//   k_commit_lroc_apply  after the argmax of a pod: the bound pod's requests and limits join its node's four sums
//                        (GetNodeRequestsAndLimits over nodeInfo.GetPods(), resourcestats.go:163-225: the scheduler cache has assumed
//                        the pod) and the node's 14 columns of the per-node table are rewritten with k_lroc_prepare's expressions —
//                        riskLimit moves through the sums, riskLoad through NodeRequestMinusPod (lowriskovercommitment.go:210-246);
//   k_commit_lroc_row    the pod's LowRiskOverCommitment row in the float32 (in-band cells recomputed in float64 in place), the
//                        float64 or the int64 form;
//   k_commit_peaks_row   the pod's Peaks row: min / max of the raw scores over the nodes the pod's CURRENT status rows pass (one LDS
//                        reduction), then NormalizeScore's byte (peaks.go:150-166), 0 for infeasible cells as the table sweep writes them.
#include <hip/hip_runtime.h>

#include <climits>

#include "lroc_cell.h"
#include "lroc_math.h"
#include "peaks_cell.h"
#include "spx_internal.h"

namespace spx {
namespace {

constexpr int kWave = 64;
constexpr int kRowBlock = 1024;       // threads of a single-row launch: 16 waves
constexpr int kRowWaves = kRowBlock / kWave;
constexpr int kNpl = 4;               // consecutive nodes per thread and step: one dword of scores (row_stride is a multiple of 16)
constexpr double kNoOver = -1e30;     // as kernels_lroc.hip: "limit - capacity" of a node that must not contribute a riskLimit
constexpr double kInf = __builtin_huge_val();

// ------------------------------------------------------------------------------------------------ LowRiskOverCommitment: commit
// Lane 0 owns cpu, lane 1 memory: each adds its resource's two numbers to the sums and rewrites its resource's columns of the
// node's table (k_lroc_prepare's expressions, split by resource) — one Beta fit per lane, no other node touched.
__global__ __launch_bounds__(kWave) void k_commit_lroc_apply(CommitLrocApplyArgs a) {
  const int64_t pod = a.row_counter ? *a.row_counter : a.pod;
  const int t = threadIdx.x;
  if (t > 1) return;
  const int32_t node = a.best_node[pod];
  if (node < 0) return;  // the pod binds nowhere: nothing changes
  const LrocArgs& l = a.l;
  const int64_t n = node, s = l.row_stride;
  double* tab = l.node_tab + n;
  const uint8_t f = l.flags[n];
  const bool has = (f & SPX_LV_HAS_METRICS) != 0;
  lroc::NodeResource r;
  if (t == 0) {
    r.requested = a.node_req_cpu[n] + l.pod_req_cpu[pod];
    r.limits = a.node_lim_cpu[n] + l.pod_lim_cpu[pod];  // the pod's limits are already raised to its requests (the flattener)
    a.node_req_cpu[n] = r.requested, a.node_lim_cpu[n] = r.limits;
    r.metric_valid = has && (f & SPX_LV_CPU_VALID) != 0;
    r.capacity = l.alloc_cpu_milli[n];
    r.capacity_stat = static_cast<double>(r.capacity);  // resourcestats.go:60-61
    r.avg = l.cpu_avg[n];
    r.stdev = l.cpu_std[n];
    // a node without metrics scores MinNodeScore (lowriskovercommitment.go:130-134): flagged by NaN in slot 0
    const double kl = has ? (1 - l.w_cpu) * lroc::risk_load(r, l.sqrt_window) : __builtin_nan("");
    tab[0 * s] = kl;
    tab[2 * s] = static_cast<double>(r.requested);
    tab[3 * s] = static_cast<double>(r.limits);
    tab[4 * s] = static_cast<double>(r.capacity);
    tab[8 * s] = has ? static_cast<double>(r.limits - r.capacity) : kNoOver;
    tab[9 * s] = has ? static_cast<double>(r.limits - r.requested) : 0.0;
    tab[12 * s] = has ? static_cast<double>(static_cast<float>(kl)) : 1.0;  // no metrics: total risk 1 -> score 0
  } else {
    r.requested = a.node_req_mem[n] + l.pod_req_mem[pod];
    r.limits = a.node_lim_mem[n] + l.pod_lim_mem[pod];
    a.node_req_mem[n] = r.requested, a.node_lim_mem[n] = r.limits;
    r.metric_valid = has && (f & SPX_LV_MEM_VALID) != 0;
    r.capacity = l.alloc_mem[n];
    r.capacity_stat = static_cast<double>(r.capacity);  // :63-65
    r.capacity_stat *= lroc::kMega;
    r.avg = l.mem_avg[n];
    r.stdev = l.mem_std[n];
    const double kl = has ? (1 - l.w_mem) * lroc::risk_load(r, l.sqrt_window) : 0.0;
    tab[1 * s] = kl;
    tab[5 * s] = static_cast<double>(r.requested);
    tab[6 * s] = static_cast<double>(r.limits);
    tab[7 * s] = static_cast<double>(r.capacity);
    tab[10 * s] = has ? static_cast<double>(r.limits - r.capacity) : kNoOver;
    tab[11 * s] = has ? static_cast<double>(r.limits - r.requested) : 0.0;
    tab[13 * s] = has ? static_cast<double>(static_cast<float>(kl)) : 0.0;
  }
}

// ------------------------------------------------------------------------------------------------ LowRiskOverCommitment: one row
// exact float64 score of one cell from the node table (k_lroc<true>'s cell, and the float32 form's fallback)
__device__ __forceinline__ uint32_t cell_f64(const LrocArgs& a, int64_t n, double prc, double prm, double plc, double plm) {
  const double* tab = a.node_tab + n;
  const int64_t s = a.row_stride;
  const double k0 = tab[0];
  const bool has = k0 == k0;
  const double rc = total_risk(a.w_cpu, has ? k0 : 0.0, tab[2 * s], tab[3 * s], tab[4 * s], prc, plc);
  const double rm = total_risk(a.w_mem, tab[s], tab[5 * s], tab[6 * s], tab[7 * s], prm, plm);
  return score_byte(has, rc, rm);
}

template <int FORM>
__global__ __launch_bounds__(kRowBlock) void k_commit_lroc_row(LrocArgs a, const int64_t* row_ptr) {
  const int64_t pod = row_ptr ? *row_ptr : a.row_begin;
  const int64_t s = a.row_stride;
  const int64_t prc = a.pod_req_cpu[pod], prm = a.pod_req_mem[pod], plc = a.pod_lim_cpu[pod], plm = a.pod_lim_mem[pod];
  const bool none = prc == 0 && prm == 0 && plc == 0 && plm == 0;  // best-effort pods score MinNodeScore (:124-128); uniform
  const double dprc = static_cast<double>(prc), dprm = static_cast<double>(prm), dplc = static_cast<double>(plc), dplm = static_cast<double>(plm);
  F32x2 plh{0.0f, 0.0f}, pll{0.0f, 0.0f}, df{0.0f, 0.0f};
  if constexpr (FORM == kLrocFormF32) {
    const float* rec = a.pod_f32 + pod * 8;
    plh = F32x2{rec[0], rec[1]}, pll = F32x2{rec[2], rec[3]}, df = F32x2{rec[4], rec[5]};
  }
  const F32x2 w2{static_cast<float>(a.w_cpu), static_cast<float>(a.w_mem)};
  unsigned redone = 0;
  uint8_t* out = a.out_score + pod * s;
  for (int64_t node0 = static_cast<int64_t>(threadIdx.x) * kNpl; node0 < s; node0 += static_cast<int64_t>(kRowBlock) * kNpl) {
    uint32_t word = 0;
    if (!none) {
#pragma unroll
      for (int j = 0; j < kNpl; ++j) {
        const int64_t n = node0 + j;  // < row_stride: the table is padded
        uint32_t b;
        if constexpr (FORM == kLrocFormF32) {
          const double* tab = a.node_tab + n;
          const double ac = tab[8 * s], am = tab[10 * s];
          const F32x2 Ah{static_cast<float>(ac), static_cast<float>(am)};
          const F32x2 Al{static_cast<float>(ac - static_cast<double>(Ah.x)), static_cast<float>(am - static_cast<double>(Ah.y))};
          const F32x2 D{__builtin_fmaxf(static_cast<float>(tab[9 * s]), 0x1p-30f), __builtin_fmaxf(static_cast<float>(tab[11 * s]), 0x1p-30f)};
          const F32x2 kl{static_cast<float>(tab[12 * s]), static_cast<float>(tab[13 * s])};
          const uint32_t kb = lroc_cell_f32(Ah, Al, D, kl, plh, pll, df, w2);
          b = (kb >> 16) & 0xffu;
          if (lroc_cell_near(kb)) {  // within the band of a rounding boundary: this cell in float64, here
            b = cell_f64(a, n, dprc, dprm, dplc, dplm);
            ++redone;
          }
        } else if constexpr (FORM == kLrocFormF64) {
          b = cell_f64(a, n, dprc, dprm, dplc, dplm);
        } else {
          const double* tab = a.node_tab + n;
          const double k0 = tab[0];
          const bool has = k0 == k0;
          const bool in = n < a.n_nodes;
          const int64_t req_c = in ? a.node_req_cpu[n] : 0, lim_c = in ? a.node_lim_cpu[n] : 0, cap_c = in ? a.alloc_cpu_milli[n] : 0;
          const int64_t req_m = in ? a.node_req_mem[n] : 0, lim_m = in ? a.node_lim_mem[n] : 0, cap_m = in ? a.alloc_mem[n] : 0;
          const double rc = total_risk(a.w_cpu, has ? k0 : 0.0, req_c, lim_c, cap_c, prc, plc);
          const double rm = total_risk(a.w_mem, tab[s], req_m, lim_m, cap_m, prm, plm);
          b = score_byte(has, rc, rm);
        }
        word |= b << (8 * j);
      }
    }
    *reinterpret_cast<uint32_t*>(out + node0) = word;
  }
  if constexpr (FORM == kLrocFormF32) {
    if (redone && a.stats) atomicAdd(a.stats + (SPX_PLUGIN_LROC * kStatSlots + (threadIdx.x & (kStatSlots - 1))) * kStatStride, static_cast<unsigned long long>(redone));
  }
}

// ------------------------------------------------------------------------------------------------ Peaks: one row
__device__ __forceinline__ double shfl_xor_f64(double v, int m) {
  const int lo = __shfl_xor(__double2loint(v), m);
  const int hi = __shfl_xor(__double2hiint(v), m);
  return __hiloint2double(hi, lo);
}

// bit j set = node0 + j does not count for `pod`: past n_nodes, or some Filter status table in play says non-zero
__device__ __forceinline__ uint32_t infeasible4(const PeaksArgs& a, int64_t pod, int64_t node0, bool active) {
  uint32_t bad = 0;
#pragma unroll
  for (int t = 0; t < 3; ++t)
    if (a.other_status[t] != nullptr && active) bad |= *reinterpret_cast<const uint32_t*>(a.other_status[t] + pod * a.row_stride + node0);
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < kNpl; ++j) m |= ((!active || node0 + j >= a.n_nodes || ((bad >> (8 * j)) & 0xffu) != 0) ? 1u : 0u) << j;
  return m;
}

__global__ __launch_bounds__(kRowBlock) void k_commit_peaks_row(PeaksArgs a, const int64_t* row_ptr) {
  __shared__ double red[2][kRowWaves];
  const int64_t pod = row_ptr ? *row_ptr : a.row_begin;
  const int64_t s = a.row_stride;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const double pod_cpu = static_cast<double>(a.pod_cpu_milli[pod]);
  constexpr int64_t kStep = static_cast<int64_t>(kRowBlock) * kNpl;
  // first pass: min and max of the raw scores over the feasible nodes (every thread stays in both loops: uniform bounds)
  double mn = kInf, mx = -kInf;
  for (int64_t base = 0; base < s; base += kStep) {
    const int64_t node0 = base + static_cast<int64_t>(threadIdx.x) * kNpl;
    const bool active = node0 < s;
    const uint32_t bad = infeasible4(a, pod, node0, active);
#pragma unroll
    for (int j = 0; j < kNpl; ++j) {
      if ((bad >> j) & 1u) continue;
      const double raw = raw_score(load_node(a, node0 + j), pod_cpu);
      mn = fmin(mn, raw);
      mx = fmax(mx, raw);
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    mn = fmin(mn, shfl_xor_f64(mn, m));
    mx = fmax(mx, shfl_xor_f64(mx, m));
  }
  if (lane == 0) red[0][wave] = mn, red[1][wave] = mx;
  __syncthreads();
  mn = red[0][0], mx = red[1][0];
#pragma unroll
  for (int w = 1; w < kRowWaves; ++w) {
    mn = fmin(mn, red[0][w]);
    mx = fmax(mx, red[1][w]);
  }
  // second pass: NormalizeScore (k_peaks<true>'s expressions); the raw scores are integers below 2^63
  const bool any = mn <= mx;  // at least one feasible node
  const long long mni = any ? static_cast<long long>(mn) : 0, mxi = any ? static_cast<long long>(mx) : 0;
  const bool zero = !any || (mni == 0 && mxi == 0);  // peaks.go:152-154: all raw scores are 0 and stay 0
  const double mnd = static_cast<double>(mni);       // exact: it came from an integer-valued float64
  const double span = static_cast<double>(mxi - mni);  // float64(maxCost - minCost)
  const bool flat = mxi == mni;
  const double rspan = 1.0 / span;
  uint8_t* out = a.out_score + pod * s;
  for (int64_t base = 0; base < s; base += kStep) {
    const int64_t node0 = base + static_cast<int64_t>(threadIdx.x) * kNpl;
    if (node0 >= s) continue;
    uint32_t word = 0;
    if (!zero) {
      const uint32_t bad = infeasible4(a, pod, node0, true);
#pragma unroll
      for (int j = 0; j < kNpl; ++j) {
        if ((bad >> j) & 1u) continue;
        const double raw = raw_score(load_node(a, node0 + j), pod_cpu);
        const double diff = raw - mnd;                      // float64(score - minCost), see raw_score
        const double norm = flat ? diff : div_rn(100.0 * diff, span, rspan);  // :158, :161
        const int sc = 100 - static_cast<int>(norm);         // :159, :162 (|norm| <= 100 for a feasible node)
        word |= static_cast<uint32_t>(sc < 0 ? 0 : (sc > 100 ? 100 : sc)) << (8 * j);
      }
    }
    *reinterpret_cast<uint32_t*>(out + node0) = word;
  }
}

}  // namespace

void launch_commit_lroc_apply(const CommitLrocApplyArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_commit_lroc_apply, dim3(1), dim3(kWave), 0, s, a); }

void launch_commit_lroc_row(const LrocArgs& a, const int64_t* row_ptr, int form, hipStream_t s) {
  if (form == kLrocFormF32)
    hipLaunchKernelGGL((k_commit_lroc_row<kLrocFormF32>), dim3(1), dim3(kRowBlock), 0, s, a, row_ptr);
  else if (form == kLrocFormF64)
    hipLaunchKernelGGL((k_commit_lroc_row<kLrocFormF64>), dim3(1), dim3(kRowBlock), 0, s, a, row_ptr);
  else
    hipLaunchKernelGGL((k_commit_lroc_row<kLrocFormI64>), dim3(1), dim3(kRowBlock), 0, s, a, row_ptr);
}

void launch_commit_peaks_row(const PeaksArgs& a, const int64_t* row_ptr, hipStream_t s) {
  hipLaunchKernelGGL(k_commit_peaks_row, dim3(1), dim3(kRowBlock), 0, s, a, row_ptr);
}

}  // namespace spx
