// kernels_network_wide.hip — NetworkOverhead for snapshots whose costs need 64 bits: the reference's own int64 accumulation
// (networkoverhead.go:576-638) and its float64 NormalizeScore (:389-418), in the shape of kernels_network.hip's table sweep.
//
// The engine takes this unit when the device holds int64 cost matrices (spx_upload_net_topo_wide, or the narrow ones widened
// because (largest cost entry) x (most pairs of a workload key) reaches 2^31).  What differs from k_net_cls:
//   - the class word in LDS is 64 bits: cost in bits 0-62, the Filter verdict in bit 63 (4 ints per class instead of 3);
//   - the row minimum and maximum are 64-bit wave reductions;
//   - phase 3b normalises with 100.0 * float64(s - min) / float64(max - min), truncated — once per class and per host node, so
//     the float64 divide stays off the per-cell path.  Integer division differs from it once the differences pass 2^53;
//   - Allocatable's normalisation is never fused in (its own launch runs).
// Phase 4 is k_net_cls's: one (status << 8 | score) word per class from LDS, host nodes patched exactly, 16-byte stores.
// The per-node form (no class table, class tables too large for LDS, raw rows, SPX_OPT_REFERENCE_KERNELS) is k_net<int64_t>.
#include <cstdlib>

#include "net_device.h"

namespace spx {

namespace {

using Acc = AccT<int64_t>;
constexpr int64_t kFailBit = std::numeric_limits<int64_t>::min();  // bit 63 of a class word

__global__ __launch_bounds__(kNetRowThreads) void k_net_cls_wide(NetArgs g) {
  SPX_RESOLVE_ROWS(g);
  extern __shared__ __align__(16) int lds[];
  const int C = g.n_classes;
  int64_t* cls_word = reinterpret_cast<int64_t*>(lds);            // cost | (Filter fails) << 63
  int* cls_hosts = lds + 2 * C;                                   // distinct host nodes of the class
  uint32_t* cls_fin = reinterpret_cast<uint32_t*>(lds + 3 * C);   // status << 8 | normalised score
  unsigned* host_bits = reinterpret_cast<unsigned*>(lds + 4 * C);
  const int lane = threadIdx.x, nthr = blockDim.x;
  const int64_t pod = g.row_begin + blockIdx.x;
  if (pod >= g.row_end) return;
  const int key = g.pod_key[pod];
  const int flag = g.key_flag[key];
  const int lo = g.pair_ptr[key], hi = g.pair_end ? g.pair_end[key] : g.pair_ptr[key + 1];  // pair_end: lists that grow (commit loop)
  const int64_t n_words = (g.n_nodes + 31) / 32;
  const uint8_t* other0 = g.other_status[0] ? g.other_status[0] + pod * g.row_stride : nullptr;
  const uint8_t* other1 = g.other_status[1] ? g.other_status[1] + pod * g.row_stride : nullptr;
  uint8_t* out_st = g.out_status + pod * g.row_stride;
  uint8_t* out_sc = g.out_score + pod * g.row_stride;

  constexpr int kG = 16;
  const int64_t groups = g.row_stride / kG;  // rows are padded to a multiple of 16 bytes
  uint16_t* scored = reinterpret_cast<uint16_t*>(host_bits + n_words);  // [groups]
  auto load16 = [](const void* p) { return *reinterpret_cast<const uint4*>(p); };
  auto byte_of = [](const uint32_t (&w)[4], int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xffu; };
  auto half_of = [](const uint32_t (&w)[8], int j) { return (w[j >> 1] >> (16 * (j & 1))) & 0xffffu; };

  if (flag != 0) {  // scoreEqually / PreFilter error, as in k_net: status 0 / 0xff everywhere, score 0
    const uint32_t st = flag == 2 ? 0xffffffffu : 0u;
    for (int64_t q = lane; q < groups; q += nthr) {
      const int64_t n0 = q * kG;
      *reinterpret_cast<uint4*>(out_st + n0) = uint4{st, st, st, st};
      *reinterpret_cast<uint4*>(out_sc + n0) = uint4{0u, 0u, 0u, 0u};
    }
    return;
  }

  // ---- the pair list into LDS when it is short enough (single-row launches only, behind the "scored" bits: as k_net_cls)
  constexpr int kStage = kNetStagePairs;
  const int scored_words = static_cast<int>((g.row_stride / 16 + 1) / 2);
  long long* sp_max = reinterpret_cast<long long*>(lds + ((4 * C + static_cast<int>(n_words) + scored_words + 1) & ~1));
  int* sp_host = reinterpret_cast<int*>(sp_max + kStage);
  int* sp_region = sp_host + kStage;
  int* sp_zone = sp_region + kStage;
  const bool staged = nthr == kNetRowThreads && hi - lo <= kStage;
  const StagedPairs sp{sp_host, sp_region, sp_zone, sp_max, hi - lo};
  if (staged) {
    for (int i = lane; i < hi - lo; i += nthr) {
      const int host = g.pair_node[lo + i];
      sp_host[i] = host, sp_region[i] = g.region[host], sp_zone[i] = g.zone[host], sp_max[i] = g.pair_max[lo + i];
    }
    __syncthreads();
  }
  auto direct = [&](int64_t node) { return staged ? direct_eval_staged<int64_t>(g, node, sp) : direct_eval<int64_t>(g, node, lo, hi); };
  // ---- phase 1 + 2
  for (int c = lane; c < C; c += nthr) {
    Acc a{0, 0, 0};
    const int region = g.cls_region[c], zone = g.cls_zone[c];
    if (staged) {
      for (int i = 0; i < sp.n; ++i) add_pair(a, g, region, zone, sp_region[i], sp_zone[i], sp_max[i]);
    } else {
      for (int i = lo; i < hi; ++i) {
        const int host = g.pair_node[i];  // wave-uniform
        add_pair(a, g, region, zone, g.region[host], g.zone[host], g.pair_max[i]);
      }
    }
    cls_word[c] = a.cost | (a.vio > a.sat ? kFailBit : 0);  // (the engine keeps a node's accumulated cost below 2^63)
    cls_hosts[c] = 0;
  }
  for (int64_t w = lane; w < n_words; w += nthr) host_bits[w] = 0u;
  __syncthreads();
  for (int i = lo + lane; i < hi; i += nthr) {
    const int host = g.pair_node[i];
    const unsigned bit = 1u << (host & 31);
    if (!(atomicOr(&host_bits[host >> 5], bit) & bit)) atomicAdd(&cls_hosts[g.node_class16[host]], 1);
  }
  __syncthreads();

  auto others16 = [&](int64_t n0, uint32_t (&oth)[4]) {  // non-zero byte: another Filter plugin rejected the node
    uint4 o4 = uint4{0, 0, 0, 0};
    if (other0) o4 = load16(other0 + n0);
    if (other1) {
      const uint4 v = load16(other1 + n0);
      o4.x |= v.x, o4.y |= v.y, o4.z |= v.z, o4.w |= v.w;
    }
    oth[0] = o4.x, oth[1] = o4.y, oth[2] = o4.z, oth[3] = o4.w;
  };
  auto classes16 = [&](int64_t n0, uint32_t (&cw)[8]) {
    const uint4 c0 = load16(g.node_class16 + n0), c1 = load16(g.node_class16 + n0 + 8);
    cw[0] = c0.x, cw[1] = c0.y, cw[2] = c0.z, cw[3] = c0.w, cw[4] = c1.x, cw[5] = c1.y, cw[6] = c1.z, cw[7] = c1.w;
  };
  auto hosts16 = [&](int64_t n0) -> uint32_t { return (host_bits[n0 >> 5] >> (n0 & 31)) & 0xffffu; };  // n0 is a multiple of 16

  // ---- phase 3: the row's minimum and maximum over the nodes that pass every Filter plugin
  int64_t mn = std::numeric_limits<int64_t>::max(), mx = std::numeric_limits<int64_t>::min();
  const bool walk = other0 || other1;
  if (!walk) {  // this plugin's verdict alone: classes that keep a non-host node, and the hosts exactly
    for (int c = lane; c < C; c += nthr) {
      const int64_t w = cls_word[c];
      if (w >= 0 && g.cls_size[c] - cls_hosts[c] > 0) {
        mn = w < mn ? w : mn;
        mx = w > mx ? w : mx;
      }
    }
    for (int i = lo + lane; i < hi; i += nthr) {
      const Acc a = direct(g.pair_node[i]);
      if (!(a.vio > a.sat)) {
        mn = a.cost < mn ? a.cost : mn;
        mx = a.cost > mx ? a.cost : mx;
      }
    }
  } else {  // 16 nodes per lane over the other plugins' status bytes; each group's "scored" bits stay in LDS for phase 4
    for (int64_t q = lane; q < groups; q += nthr) {
      const int64_t n0 = q * kG;
      uint32_t ok = 0;
      if (n0 < g.n_nodes) {
        uint32_t oth[4], cw[8];
        others16(n0, oth);
        classes16(n0, cw);
        const uint32_t hb = hosts16(n0);
        uint32_t open = 0;  // passed the other plugins, inside the table
#pragma unroll
        for (int j = 0; j < kG; ++j) open |= (n0 + j < g.n_nodes && byte_of(oth, j) == 0u) ? 1u << j : 0u;
#pragma unroll
        for (int j = 0; j < kG; ++j) {
          const int64_t w = cls_word[half_of(cw, j)];
          if (((open & ~hb) >> j) & 1u && w >= 0) {
            mn = w < mn ? w : mn;
            mx = w > mx ? w : mx;
            ok |= 1u << j;
          }
        }
        for (uint32_t hs = open & hb; hs != 0; hs &= hs - 1) {  // hosts of the pod's pairs (rare): exact
          const int j = __builtin_ctz(hs);
          const Acc a = direct(n0 + j);
          if (!(a.vio > a.sat)) {
            mn = a.cost < mn ? a.cost : mn;
            mx = a.cost > mx ? a.cost : mx;
            ok |= 1u << j;
          }
        }
      }
      scored[q] = static_cast<uint16_t>(ok);
    }
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  if (nthr > 64) {
    __shared__ int64_t s_mn[kNetRowThreads / 64], s_mx[kNetRowThreads / 64];
    if ((lane & 63) == 0) s_mn[lane >> 6] = mn, s_mx[lane >> 6] = mx;
    __syncthreads();
    mn = std::numeric_limits<int64_t>::max(), mx = std::numeric_limits<int64_t>::min();
    for (int w = 0; w < (nthr >> 6); ++w) {
      mn = s_mn[w] < mn ? s_mn[w] : mn;
      mx = s_mx[w] > mx ? s_mx[w] : mx;
    }
  }

  // ---- phase 3b: NormalizeScore per class in float64
  for (int c = lane; c < C; c += nthr) {
    const int64_t w = cls_word[c];
    const int score = w >= 0 ? norm_cost_f64(w, mn, mx) : 0;
    cls_fin[c] = static_cast<uint32_t>(score) | (w < 0 ? static_cast<uint32_t>(SPX_NET_ST_UNSCHEDULABLE) << 8 : 0u);
  }
  __syncthreads();

  // ---- phase 4
  for (int64_t q = lane; q < groups; q += nthr) {
    const int64_t n0 = q * kG;
    uint32_t st_w[4] = {0, 0, 0, 0}, sc_w[4] = {0, 0, 0, 0};
    if (n0 < g.n_nodes) {
      const uint32_t ok = walk ? scored[q] : 0xffffu;  // (written by this thread) rejected elsewhere: not scored
      uint32_t cw[8];
      classes16(n0, cw);
      const uint32_t hb = hosts16(n0);
#pragma unroll
      for (int j = 0; j < kG; ++j) {
        uint32_t fin = cls_fin[half_of(cw, j)];
        if (n0 + j >= g.n_nodes) fin = 0;
        st_w[j >> 2] |= (fin >> 8) << (8 * (j & 3));
        if ((ok >> j) & 1u) sc_w[j >> 2] |= (fin & 0xffu) << (8 * (j & 3));
      }
      for (uint32_t hs = hb; hs != 0; hs &= hs - 1) {  // a host of one of the pod's pairs: exact
        const int j = __builtin_ctz(hs);
        if (n0 + j >= g.n_nodes) continue;
        const Acc a = direct(n0 + j);
        const bool pass = !(a.vio > a.sat);
        const int score = pass ? norm_cost_f64(a.cost, mn, mx) : 0;
        const uint32_t sh = 8 * (j & 3), keep = ~(0xffu << sh);
        st_w[j >> 2] = (st_w[j >> 2] & keep) | ((pass ? 0u : static_cast<uint32_t>(SPX_NET_ST_UNSCHEDULABLE)) << sh);
        sc_w[j >> 2] = (sc_w[j >> 2] & keep) | ((((ok >> j) & 1u) ? static_cast<uint32_t>(score) : 0u) << sh);
      }
    }
    *reinterpret_cast<uint4*>(out_st + n0) = uint4{st_w[0], st_w[1], st_w[2], st_w[3]};
    *reinterpret_cast<uint4*>(out_sc + n0) = uint4{sc_w[0], sc_w[1], sc_w[2], sc_w[3]};
  }
}

}  // namespace

size_t net_wide_lds_bytes(int n_classes, int64_t n_nodes) {
  // class words (8 bytes), host counts, finished byte pairs; host bitmap; the 16 "scored" bits per group of 16 nodes of the padded row
  return static_cast<size_t>(4 * n_classes) * sizeof(int) + static_cast<size_t>((n_nodes + 31) / 32) * sizeof(unsigned) +
         static_cast<size_t>((n_nodes + 4096) / 16 + 2) * sizeof(uint16_t) + 16;  // (as net_lds_bytes)
}

void launch_net_wide(const NetArgs& g, hipStream_t s) {
  if (g.row_end <= g.row_begin) return;
  const unsigned blocks = static_cast<unsigned>(g.row_end - g.row_begin);
  NetArgs h = g;
  h.alloc_rel = nullptr, h.out_alloc = nullptr;
  // the narrow footprint fitted the budget when the node table was uploaded; a class count whose wide footprint does not takes
  // the per-node form without the class table
  if (h.n_classes > 0 && net_wide_lds_bytes(h.n_classes, h.n_nodes) > kNetLdsBudget) h.n_classes = 0;
  size_t lds = h.n_classes > 0 ? net_wide_lds_bytes(h.n_classes, h.n_nodes) : 16;
  const bool generic_only = (h.opts & kOptNetGeneric) != 0;  // SPX_OPT_REFERENCE_KERNELS
  if (!generic_only && !h.out_raw && h.n_classes > 0 && h.n_classes <= 65535 && h.node_class16 && h.row_stride % 16 == 0) {
    if (blocks == 1) lds = ((lds + 7) & ~static_cast<size_t>(7)) + kNetStagePairs * (sizeof(long long) + 3 * sizeof(int));  // the staged pair list
    hipLaunchKernelGGL(k_net_cls_wide, dim3(blocks), dim3(blocks == 1 ? kNetRowThreads : 64), lds, s, h);
    return;
  }
  hipLaunchKernelGGL(k_net<int64_t>, dim3(blocks), dim3(64), lds, s, h);
}

}  // namespace spx
