// spx_uploads.hip — tables into HBM: spx_upload_* (SoA columns), spx_update_* (snapshot deltas) and the derived host-built streams of the
// NRT sweeps (host/nrt_streams.cc).  A full node table and a delta of its rows take one road: the helpers of the first namespace below.
// The one-call loaders (object tables -> SoA -> these functions): spx_loads.hip.  Engine state and what crosses the units:
// spx_engine.h.  The first namespace below opens with the helpers only the uploads call: the exactness scans, the transposed and
// the cost-matrix uploads, the copy tasks of the pod classes.
#include "spx_engine.h"

#include <algorithm>
#include <array>
#include <cstring>
#include <mutex>
#include <utility>

#include "../host/parallel.hpp"

namespace {

using spx_host::kNrtWeightLimit;
using spx_host::nrt_biased_rcp;
using spx_host::nrt_exact_f32;
using spx_host::nrt_fast_qty;
using spx_host::nrt_value_of;
using spx_host::nrt_build_classes;
using spx_host::nrt_build_items;
using spx_host::nrt_build_rank_stream;

// every value in [0, 2^52): sums and differences of two such values are exact in float64
bool all_below_2p52(const int64_t* v, size_t n) {
  uint64_t acc = 0;
  for (size_t i = 0; i < n; ++i) acc |= static_cast<uint64_t>(v[i]);
  return (acc >> 52) == 0;
}
// every value in [0, 2^47): such a value, and the difference of two, is the sum of two float32 exactly (k_lroc_fast)
bool all_below_2p47(const int64_t* v, size_t n) {
  uint64_t acc = 0;
  for (size_t i = 0; i < n; ++i) acc |= static_cast<uint64_t>(v[i]);
  return (acc >> 47) == 0;
}
bool none_below(const int64_t* hi, const int64_t* lo, size_t n) {
  bool ok = true;
  for (size_t i = 0; i < n; ++i) ok = ok && hi[i] >= lo[i];
  return ok;
}

// the cost matrices of either width onto the device (one pair of buffers: an upload of one width replaces the other), their int64
// host copy and the largest entry
template <typename T>
int upload_net_costs(spx_engine* e, int32_t n_regions, int32_t n_zones, const T* region_cost, const T* zone_cost) {
  if (n_regions < 0 || n_zones < 0) return fail(e, SPX_ERR_ARG, "negative topology size");
  const size_t rr = static_cast<size_t>(n_regions) * n_regions, zz = static_cast<size_t>(n_zones) * n_zones;
  int rc;
  if ((rc = upload(e, e->d_net_rcost, region_cost ? static_cast<const void*>(region_cost) : static_cast<const void*>(&rc), rr * sizeof(T)))) return rc;
  if ((rc = upload(e, e->d_net_zcost, zone_cost ? static_cast<const void*>(zone_cost) : static_cast<const void*>(&rc), zz * sizeof(T)))) return rc;
  e->net_n_regions = n_regions;
  e->net_n_zones = n_zones;
  e->net_wide_dev = sizeof(T) == 8;
  e->h_net_rcost.assign(region_cost ? region_cost : nullptr, region_cost ? region_cost + rr : nullptr);
  e->h_net_zcost.assign(zone_cost ? zone_cost : nullptr, zone_cost ? zone_cost + zz : nullptr);
  e->h_net_rcost.resize(rr, -1), e->h_net_zcost.resize(zz, -1);  // (a NULL column: net_prepare widens to "no entry", full size)
  e->net_max_cost = SPX_NET_MAX_COST;
  for (const int64_t c : e->h_net_rcost) e->net_max_cost = std::max(e->net_max_cost, c);
  for (const int64_t c : e->h_net_zcost) e->net_max_cost = std::max(e->net_max_cost, c);
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->net_topo = true;
  return SPX_OK;
}

// host [N][inner] -> device [inner][N] so that lane = node reads coalesce
template <typename T>
int upload_transposed(spx_engine* e, DevBuf& b, const T* src, int64_t n, int64_t inner) {
  if (!src) return fail(e, SPX_ERR_ARG, "NULL column in table");
  std::vector<T> tmp(static_cast<size_t>(n) * static_cast<size_t>(inner));
  spx_host::parallel_rows(n, [&](int64_t row0, int64_t row1) {
    for (int64_t i = row0; i < row1; ++i)
      for (int64_t k = 0; k < inner; ++k) tmp[static_cast<size_t>(k) * n + i] = src[static_cast<size_t>(i) * inner + k];
  }, 2048);
  int rc = upload(e, b, tmp.data(), tmp.size() * sizeof(T));
  if (rc) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));  // tmp dies at scope exit
  return SPX_OK;
}

// The (row, representative) pairs of a pod batch's equivalence classes as launch_rows_expand reads them: sorted by representative (then row), and
// behind them the copy tasks — (first pair, count <= kRowsExpandFan) per run of pairs with one representative — so that a workgroup reads a
// representative's row once for up to eight copies.  Returns the task count; `dups` = [pairs | tasks].
int64_t expand_tasks(std::vector<int32_t>& dups, int64_t n_rows) {
  const size_t n = dups.size() / 2;
  // counting sort by representative (the pairs arrive in ascending order of the copied row, and stay so inside a representative's run)
  std::vector<int32_t> at(static_cast<size_t>(n_rows) + 1, 0), sorted(2 * n);
  for (size_t i = 0; i < n; ++i) ++at[static_cast<size_t>(dups[2 * i + 1]) + 1];
  for (int64_t r = 0; r < n_rows; ++r) at[static_cast<size_t>(r) + 1] += at[static_cast<size_t>(r)];
  for (size_t i = 0; i < n; ++i) {
    const size_t k = static_cast<size_t>(at[static_cast<size_t>(dups[2 * i + 1])]++);
    sorted[2 * k] = dups[2 * i], sorted[2 * k + 1] = dups[2 * i + 1];
  }
  dups.swap(sorted);
  int64_t tasks = 0;
  for (size_t i = 0; i < n;) {
    size_t j = i;
    while (j < n && j - i < static_cast<size_t>(spx::kRowsExpandFan) && dups[2 * j + 1] == dups[2 * i + 1]) ++j;
    dups.push_back(static_cast<int32_t>(i)), dups.push_back(static_cast<int32_t>(j - i));
    ++tasks;
    i = j;
  }
  return tasks;
}

// one pinned blob for a delta's columns: [idx int32 n] then each column, 16-byte aligned; uploaded with one DMA
struct DeltaBlob {
  spx_engine* e;
  size_t bytes = 0;
  std::vector<std::pair<const void*, size_t>> parts;  // (source, bytes)
  std::vector<size_t> offset;
  size_t add(const void* src, size_t n) {
    const size_t at = bytes;
    parts.emplace_back(src, n);
    offset.push_back(at);
    bytes = (bytes + n + 15) & ~static_cast<size_t>(15);
    return at;
  }
  int ship() {
    if (int rc = ensure_pinned(e, e->h_stage, e->h_stage_bytes, bytes, 65536)) return rc;
    for (size_t k = 0; k < parts.size(); ++k) {
      char* dst = static_cast<char*>(e->h_stage) + offset[k];
      const char* src = static_cast<const char*>(parts[k].first);
      const int64_t blocks = static_cast<int64_t>((parts[k].second + 65535) / 65536);  // (a full node table: megabytes per column)
      const size_t len = parts[k].second;
      spx_host::parallel_rows(blocks, [&](int64_t b0, int64_t b1) {
        const size_t at = static_cast<size_t>(b0) * 65536, end = std::min(len, static_cast<size_t>(b1) * 65536);
        if (end > at) std::memcpy(dst + at, src + at, end - at);
      }, 16);
    }
    return upload(e, e->d_delta, e->h_stage, bytes);
  }
  const char* dev(size_t at) const { return static_cast<const char*>(e->d_delta.p) + at; }
};

// an index listed twice would be scattered twice in no particular order — and the columns that travel with the rows (the float64
// images, the host copies, a presence column) could end up describing different rows of the delta: refused
int refuse_duplicates(spx_engine* e, const int32_t* idx, int64_t n, const char* msg) {
  std::vector<int32_t> sorted(idx, idx + n);
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(e, SPX_ERR_ARG, msg);
  return SPX_OK;
}

int delta_indices(spx_engine* e, const int64_t* idx, int64_t n_rows, std::vector<int32_t>& out) {
  if (n_rows < 0 || (n_rows && !idx)) return fail(e, SPX_ERR_ARG, "delta: NULL index column");
  out.resize(static_cast<size_t>(n_rows));
  for (int64_t i = 0; i < n_rows; ++i) {
    if (idx[i] < 0 || idx[i] >= e->n_nodes) return fail(e, SPX_ERR_ARG, "delta: node index out of range");
    out[static_cast<size_t>(i)] = static_cast<int32_t>(idx[i]);
  }
  return refuse_duplicates(e, out.data(), n_rows, "delta: a node index is listed twice");
}

// the trimaran node table's columns, in the order they are shipped
struct TriCol {
  DevBuf* dst;
  const void* src;
  int bytes;  // per node
};
std::array<TriCol, 11> trimaran_cols(spx_engine* e, const spx_trimaran_nodes_soa* t) {
  return {{{&e->d_cap_cpu, t->cap_cpu_milli, 8}, {&e->d_tlp_util, t->tlp_cpu_util, 8}, {&e->d_tlp_missing, t->tlp_missing_milli, 8}, {&e->d_tlp_valid, t->tlp_valid, 1},
           {&e->d_lv_acpu, t->lv_alloc_cpu_milli, 8}, {&e->d_lv_amem, t->lv_alloc_mem, 8}, {&e->d_lv_cavg, t->lv_cpu_avg, 8}, {&e->d_lv_cstd, t->lv_cpu_std, 8},
           {&e->d_lv_mavg, t->lv_mem_avg, 8}, {&e->d_lv_mstd, t->lv_mem_std, 8}, {&e->d_lv_flags, t->lv_flags, 1}}};
}
// the exactness of LVRB's allocatable columns, an aggregate over all nodes: a full table establishes it (replace), a delta's rows
// may only take it away
void trimaran_alloc_exactness(spx_engine* e, const spx_trimaran_nodes_soa* t, bool replace) {
  const size_t n = static_cast<size_t>(t->n_nodes);
  e->lv_alloc_exact = (replace || e->lv_alloc_exact) && all_below_2p52(t->lv_alloc_cpu_milli, n) && all_below_2p52(t->lv_alloc_mem, n);
  e->lv_alloc_f32 = (replace || e->lv_alloc_f32) && all_below_2p47(t->lv_alloc_cpu_milli, n) && all_below_2p47(t->lv_alloc_mem, n);
}

// What rows [row0, row1) of an NRT node table say about the float64 formulation's preconditions.  A full upload scans the table in
// chunks and merges; a delta scans its rows and merges into what the engine holds.
struct NrtRowScan {
  bool ok = true;     // NUMA ids are list positions, every present capacity is in the formulation's range (nrt_fast_qty)
  bool ln_ok = true;  // every zone cost lies within [0, 255]: LeastNUMANodes' tables can be built (findSuitableCombination's 256 sentinel)
  uint32_t big = 0;   // slots with a capacity (Value() form) that float32 does not hold exactly
  spx_engine::NrtQty qty;
  void merge(const NrtRowScan& o) { ok = ok && o.ok, ln_ok = ln_ok && o.ln_ok, big |= o.big, qty.merge(o.qty); }
};
NrtRowScan nrt_scan_rows(const spx_nrt_nodes_soa* t, int cpu_slot, int64_t row0, int64_t row1) {
  constexpr int64_t Zm = SPX_NRT_MAX_ZONES;
  const int64_t R = t->n_res;
  NrtRowScan s;
  for (int64_t i = row0; i < row1; ++i) {
    const int nz = t->n_zones[i];
    for (int z = 0; z < nz && z < Zm; ++z) {
      if (t->zone_id[i * Zm + z] != z) s.ok = false;  // "lowest NUMA id" must be "lowest list position"
      for (int64_t r = 0; r < R; ++r) {
        if (!((t->zone_present[i * Zm + z] >> r) & 1u)) continue;
        const int64_t cap = t->zone_avail[(i * Zm + z) * R + r];
        if (!nrt_fast_qty(cap)) s.ok = false;
        if (!nrt_exact_f32(static_cast<double>(nrt_value_of(r == cpu_slot, cap)))) s.big |= 1u << r;
        if (cap >= 0) s.qty.add(static_cast<int>(r), nrt_value_of(r == cpu_slot, cap));
      }
      for (int zb = 0; zb < nz && zb < Zm; ++zb) {
        const int64_t c = t->zone_cost[(i * Zm + z) * Zm + zb];
        if (c < 0 || c > 255) s.ln_ok = false;
      }
    }
  }
  return s;
}

// Rows of an NRT node table to the device: row i of `t` describes node ix[i] (`whole`: every node, in order — a full upload).  The
// rows as they are join `b` (which may hold parts of the caller's already) and leave with one DMA; the device turns them into the
// node-major columns (k_scatter_rows) and the float64 formulation's derived columns (k_nrt_derive_rows).  The caller waits for the stream.
int ship_nrt_rows(spx_engine* e, const spx_nrt_nodes_soa* t, const std::vector<int32_t>& ix, bool whole, DeltaBlob& b) {
  constexpr size_t Zm = SPX_NRT_MAX_ZONES;
  const int64_t n = t->n_nodes, N = e->n_nodes;
  const size_t m = static_cast<size_t>(n), R = static_cast<size_t>(t->n_res);
  const size_t o_idx = b.add(ix.data(), m * 4);
  const size_t o_flags = b.add(t->flags, m), o_max = b.add(t->max_numa, m * 4), o_nz = b.add(t->n_zones, m), o_np = b.add(t->node_present, m);
  const size_t o_zid = b.add(t->zone_id, m * Zm), o_zp = b.add(t->zone_present, m * Zm);
  const size_t o_av = b.add(t->zone_avail, m * Zm * R * 8), o_cost = b.add(t->zone_cost, m * Zm * Zm * 4);
  const size_t o_min = b.add(t->min_avg_dist, m * Zm * 4);
  if (int rc = b.ship()) return rc;
  const int32_t* d_idx = reinterpret_cast<const int32_t*>(b.dev(o_idx));
  hipStream_t s = e->stream;
  // the one-wide columns of a whole table are the staged columns as they are: copied (scattered with the identity index, the four
  // took stage 4 of spx_load_nrt from 2.61 to 2.80 ms at 20 000 nodes, outside its run-to-run spread)
  const struct { DevBuf& dst; size_t at; int bytes; } narrow[] = {{e->d_nrt_flags, o_flags, 1}, {e->d_nrt_max_numa, o_max, 4}, {e->d_nrt_nz, o_nz, 1}, {e->d_nrt_np, o_np, 1}};
  for (const auto& c : narrow) {
    if (whole) SPX_HIP(e, hipMemcpyAsync(c.dst.p, b.dev(c.at), m * static_cast<size_t>(c.bytes), hipMemcpyDeviceToDevice, s));
    else spx::launch_scatter_rows(c.dst.p, N, 1, d_idx, b.dev(c.at), n, c.bytes, s);
  }
  spx::launch_scatter_rows(e->d_nrt_zid.p, N, static_cast<int>(Zm), d_idx, b.dev(o_zid), n, 1, s);
  spx::launch_scatter_rows(e->d_nrt_zp.p, N, static_cast<int>(Zm), d_idx, b.dev(o_zp), n, 1, s);
  if (R) spx::launch_scatter_rows(e->d_nrt_avail.p, N, static_cast<int>(Zm * R), d_idx, b.dev(o_av), n, 8, s);
  spx::launch_scatter_rows(e->d_nrt_cost.p, N, static_cast<int>(Zm * Zm), d_idx, b.dev(o_cost), n, 4, s);
  spx::launch_scatter_rows(e->d_nrt_minavg.p, N, static_cast<int>(Zm), d_idx, b.dev(o_min), n, 4, s);
  spx::NrtDeltaArgs da{};
  da.n_rows = n, da.n_nodes = N, da.n_res = t->n_res, da.cpu_slot = e->nrt_cpu_slot;
  da.idx = d_idx, da.n_zones = reinterpret_cast<const uint8_t*>(b.dev(o_nz)), da.zone_present = reinterpret_cast<const uint8_t*>(b.dev(o_zp));
  da.zone_avail = reinterpret_cast<const int64_t*>(b.dev(o_av));
  da.f_av = static_cast<double*>(e->d_nrt_fav.p), da.f_rc = static_cast<double*>(e->d_nrt_frc.p), da.f_rcv = static_cast<double*>(e->d_nrt_frcv.p);
  da.f_cpu = static_cast<double*>(e->d_nrt_fcpu.p), da.f_braw = static_cast<double*>(e->d_nrt_fbraw.p), da.f_rep = static_cast<uint8_t*>(e->d_nrt_frep.p);
  spx::launch_nrt_derive_rows(da, s);
  SPX_HIP(e, hipGetLastError());
  return SPX_OK;
}

// Rows of a SySched node table to the device: row i of `t` describes node ix[i] (`whole`: every node, in order — a full upload).  The
// word columns and the three per-node columns leave in one blob and are scattered (or, whole, copied) into place; the stale CSR is
// rebuilt on the host from the engine's copy with the listed nodes' lists replaced, and uploaded whole (the lists are short and
// rare).  Everything is validated before the first byte moves.  The caller waits for the stream.
int ship_sysched_rows(spx_engine* e, const spx_sysched_nodes_soa* t, const std::vector<int32_t>& ix, bool whole) {
  const int64_t n = t->n_nodes, N = e->n_nodes;
  const int32_t W = t->n_words;
  if (!t->host_bits || !t->present || !t->n_resident || !t->resident_missing || !t->stale_ptr) return fail(e, SPX_ERR_ARG, "NULL column in table");
  if (t->stale_ptr[0] < 0 || (t->stale_ptr[n] > t->stale_ptr[0] && (!t->stale_bit || !t->stale_count))) return fail(e, SPX_ERR_ARG, "SySched: bad stale list");
  for (int64_t i = 0; i < n; ++i) {
    if (t->stale_ptr[i + 1] < t->stale_ptr[i]) return fail(e, SPX_ERR_ARG, "SySched: stale_ptr is not monotone");
    int64_t stale_sum = 0;
    for (int32_t j = t->stale_ptr[i]; j < t->stale_ptr[i + 1]; ++j) {
      if (t->stale_bit[j] < 0 || t->stale_bit[j] >= W * 64 || t->stale_count[j] < 0) return fail(e, SPX_ERR_ARG, "SySched: stale entry out of range");
      stale_sum += t->stale_count[j];
    }
    // the largest score any pod can get on this node: every name outside H, k times — 100 x that is formed in 32 bits
    const int64_t k = t->n_resident[i], a = t->resident_missing[i];
    if (k < 0 || a < 0 || a + (k + 1) * static_cast<int64_t>(W) * 64 >= SPX_SYSCHED_MAX_SCORE || stale_sum > a + (k + 1) * static_cast<int64_t>(W) * 64)
      return fail(e, SPX_ERR_ARG, "SySched: a node's largest possible score reaches SPX_SYSCHED_MAX_SCORE");
  }
  // the stale CSR with the listed nodes' lists replaced
  std::vector<int32_t> sptr(static_cast<size_t>(N) + 1, 0), sbit, scnt;
  if (whole) {
    const int32_t base = t->stale_ptr[0];
    for (int64_t i = 0; i <= N; ++i) sptr[static_cast<size_t>(i)] = t->stale_ptr[i] - base;
    sbit.assign(t->stale_bit + base, t->stale_bit + t->stale_ptr[N]);
    scnt.assign(t->stale_count + base, t->stale_count + t->stale_ptr[N]);
  } else {
    std::vector<int64_t> row_of(static_cast<size_t>(N), -1);
    for (int64_t i = 0; i < n; ++i) row_of[static_cast<size_t>(ix[static_cast<size_t>(i)])] = i;
    for (int64_t node = 0; node < N; ++node) {
      const int64_t r = row_of[static_cast<size_t>(node)];
      const int32_t* b = r >= 0 ? t->stale_bit : e->h_sy_sbit.data();
      const int32_t* c = r >= 0 ? t->stale_count : e->h_sy_scnt.data();
      const int32_t j0 = r >= 0 ? t->stale_ptr[r] : e->h_sy_sptr[static_cast<size_t>(node)], j1 = r >= 0 ? t->stale_ptr[r + 1] : e->h_sy_sptr[static_cast<size_t>(node) + 1];
      for (int32_t j = j0; j < j1; ++j) sbit.push_back(b[j]), scnt.push_back(c[j]);
      sptr[static_cast<size_t>(node) + 1] = static_cast<int32_t>(sbit.size());
    }
  }
  int rc;
  const size_t m = static_cast<size_t>(n);
  DeltaBlob b{e};
  const size_t o_idx = b.add(ix.data(), m * 4);
  const size_t o_bits = b.add(t->host_bits, m * static_cast<size_t>(W) * 8), o_pres = b.add(t->present, m), o_k = b.add(t->n_resident, m * 4),
               o_a = b.add(t->resident_missing, m * 4);
  if ((rc = b.ship())) return rc;
  const int32_t* d_idx = reinterpret_cast<const int32_t*>(b.dev(o_idx));
  hipStream_t s = e->stream;
  if (whole) {  // the staged columns are the device columns as they are
    SPX_HIP(e, hipMemcpyAsync(e->d_sy_host.p, b.dev(o_bits), m * static_cast<size_t>(W) * 8, hipMemcpyDeviceToDevice, s));
    SPX_HIP(e, hipMemcpyAsync(e->d_sy_present.p, b.dev(o_pres), m, hipMemcpyDeviceToDevice, s));
    SPX_HIP(e, hipMemcpyAsync(e->d_sy_k.p, b.dev(o_k), m * 4, hipMemcpyDeviceToDevice, s));
    SPX_HIP(e, hipMemcpyAsync(e->d_sy_a.p, b.dev(o_a), m * 4, hipMemcpyDeviceToDevice, s));
  } else {
    for (int32_t w = 0; w < W; ++w)  // word w of the rows [W][n] -> word column w of the table [W][N]
      spx::launch_scatter_rows(static_cast<uint64_t*>(e->d_sy_host.p) + static_cast<size_t>(w) * N, N, 1, d_idx, b.dev(o_bits + static_cast<size_t>(w) * m * 8), n, 8, s);
    spx::launch_scatter_rows(e->d_sy_present.p, N, 1, d_idx, b.dev(o_pres), n, 1, s);
    spx::launch_scatter_rows(e->d_sy_k.p, N, 1, d_idx, b.dev(o_k), n, 4, s);
    spx::launch_scatter_rows(e->d_sy_a.p, N, 1, d_idx, b.dev(o_a), n, 4, s);
    SPX_HIP(e, hipGetLastError());
  }
  if ((rc = upload(e, e->d_sy_sptr, sptr.data(), sptr.size() * 4)) || (rc = upload(e, e->d_sy_sbit, sbit.data(), sbit.size() * 4)) ||
      (rc = upload(e, e->d_sy_scnt, scnt.data(), scnt.size() * 4)))
    return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));  // sptr / sbit / scnt are about to move
  e->h_sy_sptr = std::move(sptr), e->h_sy_sbit = std::move(sbit), e->h_sy_scnt = std::move(scnt);
  return SPX_OK;
}

// The float64 formulation's view of an NRT slot table: the cpu slot, whether the weights are in its range, and per slot subset the sum
// of the weights with its biased reciprocal ([2^n_res][2]; zeros when they are not in range).
struct NrtSlotWeights {
  int32_t cpu_slot = -1;
  bool fast = true;
  std::vector<double> wtab;
};
NrtSlotWeights nrt_slot_weights(const spx_nrt_slots* t) {
  NrtSlotWeights w;
  int64_t wtotal = 0;
  for (int i = 0; i < t->n_res; ++i) {
    if (t->slot_flags[i] & SPX_NRT_SLOT_CPU) w.cpu_slot = i;
    // the Least/MostAllocated Score accumulates integer zone totals (v_mad_u32_u24: weights below 2^24) whose high bit marks a
    // zero zone score: 100 * sum(weights) must stay below 2^31 — with room, sum(weights) < 2^20 (upstream weights are 1..100)
    if (t->slot_weight[i] < 0 || t->slot_weight[i] >= kNrtWeightLimit) w.fast = false;
    else wtotal += t->slot_weight[i];
  }
  if (wtotal >= kNrtWeightLimit) w.fast = false;
  w.wtab.assign(static_cast<size_t>(2) << t->n_res, 0.0);
  if (w.fast)
    for (unsigned m = 0; m < (1u << t->n_res); ++m) {
      int64_t sum = 0;
      for (int i = 0; i < t->n_res; ++i)
        if ((m >> i) & 1u) sum += t->slot_weight[i];
      w.wtab[2 * m] = static_cast<double>(sum);
      w.wtab[2 * m + 1] = nrt_biased_rcp(static_cast<double>(sum));
    }
  return w;
}

// Pod classes to the device: `uniq` the representative rows, `dups` the (row, representative) pairs, which leave as [pairs | copy
// tasks] (expand_tasks).  The three counters are set once both columns are on their way and the vectors may go out of scope.
int ship_classes(spx_engine* e, DevBuf& d_uniq, DevBuf& d_dups, const std::vector<int32_t>& uniq, std::vector<int32_t>& dups, int64_t n_rows, int64_t& n_uniq,
                 int64_t& n_dups, int64_t& n_tasks) {
  const int64_t pairs = static_cast<int64_t>(dups.size() / 2), tasks = expand_tasks(dups, n_rows);
  int rc;
  if ((rc = upload(e, d_uniq, uniq.data(), uniq.size() * sizeof(int32_t)))) return rc;
  if ((rc = upload(e, d_dups, dups.data(), dups.size() * sizeof(int32_t)))) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  n_uniq = static_cast<int64_t>(uniq.size()), n_dups = pairs, n_tasks = tasks;
  return SPX_OK;
}
}  // namespace

extern "C" {

int spx_upload_alloc_nodes(spx_engine* e, const spx_alloc_nodes_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  int rc = set_nodes(e, t->n_nodes);
  if (rc) return rc;
  if (t->n_res <= 0) return fail(e, SPX_ERR_ARG, "n_res must be positive");
  rc = upload(e, e->d_alloc, t->alloc, static_cast<size_t>(t->n_res) * static_cast<size_t>(t->n_nodes) * sizeof(int64_t));
  if (rc) return rc;
  e->alloc_n_res = t->n_res;
  e->alloc_ready = false;
  SPX_HIP(e, hipStreamSynchronize(e->stream));  // host columns are only borrowed for the call
  return SPX_OK;
}

int spx_upload_trimaran_nodes(spx_engine* e, const spx_trimaran_nodes_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  int rc = set_nodes(e, t->n_nodes);
  if (rc) return rc;
  const size_t n = static_cast<size_t>(t->n_nodes);
  e->tlp_amb_built = e->lv_amb_built = false;  // (before the first column changes: a failed upload must not leave tables that describe the old ones)
  for (const TriCol& c : trimaran_cols(e, t))
    if ((rc = upload(e, *c.dst, c.src, n * static_cast<size_t>(c.bytes)))) return rc;
  trimaran_alloc_exactness(e, t, true);
  e->lroc_tab_ready = false;
  e->tri_nodes = true;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}


int spx_update_trimaran_nodes(spx_engine* e, const int64_t* idx, const spx_trimaran_nodes_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (!e->tri_nodes) return fail(e, SPX_ERR_STATE, "trimaran node delta: upload the full table first");
  const int64_t n = t->n_nodes;
  if (n == 0) return SPX_OK;
  const std::array<TriCol, 11> cols = trimaran_cols(e, t);
  for (const TriCol& c : cols)
    if (!c.src) return fail(e, SPX_ERR_ARG, "NULL column in table");
  std::vector<int32_t> ix;
  int rc = delta_indices(e, idx, n, ix);
  if (rc) return rc;
  e->tlp_amb_built = e->lv_amb_built = false;  // rows of the columns k_tlp_amb_build / k_lvrb_amb_build read are about to change
  const size_t m = static_cast<size_t>(n);
  DeltaBlob b{e};
  const size_t o_idx = b.add(ix.data(), m * 4);
  size_t at[11];
  for (size_t k = 0; k < cols.size(); ++k) at[k] = b.add(cols[k].src, m * static_cast<size_t>(cols[k].bytes));
  if ((rc = b.ship())) return rc;
  for (size_t k = 0; k < cols.size(); ++k)
    spx::launch_scatter_rows(cols[k].dst->p, e->n_nodes, 1, reinterpret_cast<const int32_t*>(b.dev(o_idx)), b.dev(at[k]), n, cols[k].bytes, e->stream);
  SPX_HIP(e, hipGetLastError());
  trimaran_alloc_exactness(e, t, false);
  e->lroc_tab_ready = false;
  e->evaluated = 0;  // every table computed from the old rows is stale
  e->best_valid = false;
  SPX_HIP(e, hipStreamSynchronize(e->stream));  // host columns are only borrowed for the call
  return SPX_OK;
}

// AppGroup scheduled lists grow between cycles (networkoverhead.go:654-694 reads them from the pod lister): the new (key, host,
// MaxNetworkCost) pairs — spx_flatten_net_placed — are appended to the workload keys' lists on the device.  The host lays out the
// new CSR (key counts only), the old pairs move inside the device (k_spread_pairs), the new ones are scattered behind them.
int spx_update_net_placed(spx_engine* e, int64_t n, const int32_t* key, const int32_t* node, const int64_t* max_cost) {
  if (!e || n < 0 || (n && (!key || !node || !max_cost))) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (!e->net_pods) return fail(e, SPX_ERR_STATE, "NetworkOverhead delta: upload the pod table first");
  if (n == 0) return SPX_OK;
  const size_t K = static_cast<size_t>(e->net_n_keys);
  std::vector<int32_t> add(K, 0);
  std::vector<uint8_t> flag = e->h_key_flag;
  for (int64_t i = 0; i < n; ++i) {
    if (key[i] < 0 || static_cast<size_t>(key[i]) >= K) return fail(e, SPX_ERR_ARG, "NetworkOverhead delta: key out of range");
    if (max_cost[i] < 0) {  // the group's scheduled list is no longer empty: the key stops scoring equally (networkoverhead.go:215-224)
      if (flag[static_cast<size_t>(key[i])] == 1) flag[static_cast<size_t>(key[i])] = 0;
      continue;
    }
    if (node[i] >= e->n_nodes) return fail(e, SPX_ERR_ARG, "NetworkOverhead delta: node index out of range");
    if (node[i] < 0) flag[static_cast<size_t>(key[i])] = 2;  // host not in the snapshot: PreFilter returns Error (:258, :274)
    else if (flag[static_cast<size_t>(key[i])] == 1) flag[static_cast<size_t>(key[i])] = 0;
    ++add[static_cast<size_t>(key[i])];
  }
  std::vector<int32_t> ptr(K + 1, 0), fill(K);
  for (size_t k = 0; k < K; ++k) {
    const int64_t next = static_cast<int64_t>(ptr[k]) + (e->h_pair_ptr[k + 1] - e->h_pair_ptr[k]) + add[k];
    if (next > INT32_MAX) return fail(e, SPX_ERR_ARG, "NetworkOverhead delta: more than 2^31 pairs");
    ptr[k + 1] = static_cast<int32_t>(next);
    fill[k] = ptr[k] + (e->h_pair_ptr[k + 1] - e->h_pair_ptr[k]);
  }
  std::vector<int32_t> pos, nd;
  std::vector<int64_t> cost;
  pos.reserve(static_cast<size_t>(n)), nd.reserve(static_cast<size_t>(n)), cost.reserve(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i)
    if (max_cost[i] >= 0) pos.push_back(fill[static_cast<size_t>(key[i])]++), nd.push_back(node[i]), cost.push_back(max_cost[i]);
  const size_t m = pos.size(), total = static_cast<size_t>(ptr[K]);
  int rc;
  if ((rc = ensure(e, e->d_net_pair_node2, (total ? total : 1) * 4)) || (rc = ensure(e, e->d_net_pair_max2, (total ? total : 1) * 8))) return rc;
  DeltaBlob b{e};
  const size_t o_ptr = b.add(ptr.data(), (K + 1) * 4), o_flag = b.add(flag.data(), K), o_pos = b.add(pos.data(), m * 4), o_node = b.add(nd.data(), m * 4),
               o_cost = b.add(cost.data(), m * 8);
  if ((rc = b.ship())) return rc;
  spx::launch_spread_pairs(static_cast<int32_t>(K), static_cast<const int32_t*>(e->d_net_pair_ptr.p), reinterpret_cast<const int32_t*>(b.dev(o_ptr)),
                           static_cast<const int32_t*>(e->d_net_pair_node.p), static_cast<const int64_t*>(e->d_net_pair_max.p),
                           static_cast<int32_t*>(e->d_net_pair_node2.p), static_cast<int64_t*>(e->d_net_pair_max2.p), e->stream);
  spx::launch_net_append(static_cast<int64_t>(m), reinterpret_cast<const int32_t*>(b.dev(o_pos)), reinterpret_cast<const int32_t*>(b.dev(o_node)),
                         reinterpret_cast<const int64_t*>(b.dev(o_cost)), static_cast<int32_t*>(e->d_net_pair_node2.p), static_cast<int64_t*>(e->d_net_pair_max2.p),
                         e->stream);
  SPX_HIP(e, hipGetLastError());
  SPX_HIP(e, hipMemcpyAsync(e->d_net_pair_ptr.p, b.dev(o_ptr), (K + 1) * 4, hipMemcpyDeviceToDevice, e->stream));
  SPX_HIP(e, hipMemcpyAsync(e->d_net_key_flag.p, b.dev(o_flag), K, hipMemcpyDeviceToDevice, e->stream));
  std::swap(e->d_net_pair_node, e->d_net_pair_node2);
  std::swap(e->d_net_pair_max, e->d_net_pair_max2);
  e->h_pair_ptr = std::move(ptr);
  e->h_key_flag = std::move(flag);
  e->net_max_pairs = 0;
  for (size_t k = 0; k < K; ++k) e->net_max_pairs = std::max<int64_t>(e->net_max_pairs, e->h_pair_ptr[k + 1] - e->h_pair_ptr[k]);
  e->evaluated &= ~(1u << SPX_PLUGIN_NETOVERHEAD);
  e->best_valid = false;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

// ElasticQuota Used moves with every pod added to or removed from a namespace (capacity_scheduling.go:679-803 -> elasticquota.go
// reserveResource / unreserveResource): the changed namespaces' rows replace the device rows, with the aggregate vector PreFilter
// compares against the aggregate Min (capacity_scheduling.go:260-262).
int spx_update_quota_used(spx_engine* e, int64_t n_rows, const int32_t* ns, const int64_t* used, const uint8_t* used_present, const int64_t* agg_used,
                          const uint8_t* agg_used_present) {
  if (!e || n_rows < 0 || !agg_used || !agg_used_present || (n_rows && (!ns || !used || !used_present))) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (!e->quota) return fail(e, SPX_ERR_STATE, "quota delta: upload the quota table first");
  e->pre_marks_valid = e->pre_valid = false;  // the preemption dry run read the old Used
  constexpr size_t S = SPX_QUOTA_SLOTS;
  for (int64_t i = 0; i < n_rows; ++i)
    if (ns[i] < 0 || ns[i] >= e->q_n_namespaces) return fail(e, SPX_ERR_ARG, "quota delta: namespace index out of range");
  if (int rc = refuse_duplicates(e, ns, n_rows, "quota delta: a namespace is listed twice")) return rc;  // (d_q_used and d_q_usedp from different rows)
  const size_t m = static_cast<size_t>(n_rows);
  int64_t agg[SPX_QUOTA_SLOTS + 1];
  std::memcpy(agg, agg_used, sizeof e->q_agg_used);
  agg[SPX_QUOTA_SLOTS] = *agg_used_present;
  DeltaBlob b{e};
  const size_t o_idx = b.add(ns, m * 4), o_used = b.add(used, m * S * 8), o_p = b.add(used_present, m), o_agg = b.add(agg, sizeof agg);
  int rc;
  if ((rc = b.ship())) return rc;
  spx::launch_scatter_rows_rowmajor(e->d_q_used.p, static_cast<int>(S), reinterpret_cast<const int32_t*>(b.dev(o_idx)), b.dev(o_used), n_rows, 8, e->stream);
  spx::launch_scatter_rows_rowmajor(e->d_q_usedp.p, 1, reinterpret_cast<const int32_t*>(b.dev(o_idx)), b.dev(o_p), n_rows, 1, e->stream);
  SPX_HIP(e, hipGetLastError());
  SPX_HIP(e, hipMemcpyAsync(e->d_q_agg.p, b.dev(o_agg), sizeof agg, hipMemcpyDeviceToDevice, e->stream));
  std::memcpy(e->q_agg_used, agg_used, sizeof e->q_agg_used);
  e->q_agg_used_present = *agg_used_present;
  e->evaluated &= ~(1u << SPX_PLUGIN_CAPACITY);
  e->best_valid = false;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

int spx_update_nrt_nodes(spx_engine* e, const int64_t* idx, const spx_nrt_nodes_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (e->nrt_wide)
    return fail(e, SPX_ERR_STATE, "NRT node delta: the engine holds a wide snapshot (more than 8 resource slots, or SPX_OPT_NRT_WIDE): load it again instead");
  if (!e->nrt_nodes || !e->nrt_slots) return fail(e, SPX_ERR_STATE, "NRT node delta: upload the slot and node tables first");
  if (!e->h_nrt_tall_nodes.empty())
    return fail(e, SPX_ERR_STATE, "NRT node delta: the engine holds nodes with more than 8 NUMA zones (spx_upload_nrt_tall_nodes): load the snapshot again instead");
  if (t->n_res != e->nrt_n_res) return fail(e, SPX_ERR_ARG, "NRT node delta: n_res differs from the slot table");
  const int64_t n = t->n_nodes;
  if (n == 0) return SPX_OK;
  if (!t->flags || !t->max_numa || !t->n_zones || !t->zone_id || !t->zone_present || !t->zone_cost || !t->min_avg_dist || !t->node_present ||
      (!t->zone_avail && t->n_res))
    return fail(e, SPX_ERR_ARG, "NULL column in table");
  for (int64_t i = 0; i < n; ++i)
    if (t->n_zones[i] == SPX_NRT_ZONES_TALL)
      return fail(e, SPX_ERR_STATE, "NRT node delta: row " + std::to_string(i) + " is a node with more than 8 NUMA zones (n_zones = SPX_NRT_ZONES_TALL): load the snapshot again instead");
  std::vector<int32_t> ix;
  int rc = delta_indices(e, idx, n, ix);
  if (rc) return rc;
  constexpr size_t Zm = SPX_NRT_MAX_ZONES;
  // a row that breaks the float64 formulation's preconditions sends the whole table to the reference-arithmetic kernel until the next full upload
  const NrtRowScan scan = nrt_scan_rows(t, e->nrt_cpu_slot, 0, n);
  bool cost_changed = false;  // zone costs or zone counts differ from what LeastNUMANodes' tables were built from
  for (int64_t i = 0; i < n && !cost_changed; ++i) {
    const size_t node = static_cast<size_t>(ix[static_cast<size_t>(i)]);
    cost_changed = std::memcmp(&e->h_nrt_cost[node * Zm * Zm], t->zone_cost + i * Zm * Zm, sizeof(int32_t) * Zm * Zm) != 0 || e->h_nrt_nz[node] != t->n_zones[i];
  }
  DeltaBlob b{e};
  if ((rc = ship_nrt_rows(e, t, ix, false, b))) return rc;
  if (cost_changed)  // (the host copies follow once the rows have shipped: a failed delta leaves them describing the device)
    for (int64_t i = 0; i < n; ++i) {
      const size_t node = static_cast<size_t>(ix[static_cast<size_t>(i)]);
      std::memcpy(&e->h_nrt_cost[node * Zm * Zm], t->zone_cost + i * Zm * Zm, sizeof(int32_t) * Zm * Zm);
      e->h_nrt_nz[node] = t->n_zones[i];
    }
  e->nrt_fast_nodes = e->nrt_fast_nodes && scan.ok;
  e->nrt_big_nodes |= scan.big;
  e->nrt_qty_nodes.merge(scan.qty);
  // (an unchanged row's costs are the host copy's, which an earlier scan vouched for unless nrt_ln_ok is false already — and it stays
  // false until the next full upload: scanning every row of the delta decides as scanning the changed ones would)
  e->nrt_ln_ok = e->nrt_ln_ok && scan.ln_ok;
  e->nrt_pk_tab_built = e->nrt_wsort_built = false;  // zone capacities changed
  if (cost_changed) e->nrt_ln_built = false;  // LeastNUMANodes' per-node tables are rebuilt when that strategy is next evaluated
  // (the window-local node order — perm — is a grouping hint for the sweep, not a correctness input: left as it is)
  e->evaluated = 0;  // NRT's tables, and every table normalised over the feasible nodes its status named (Allocatable, NetworkOverhead, Peaks)
  e->best_valid = false;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

int spx_set_lroc_params(spx_engine* e, const spx_lroc_params* p) {
  if (!e || !p) return SPX_ERR_ARG;
  // defaults.go:176-186 substitutes defaults for bad values before the plugin sees them; the engine takes the result
  if (p->smoothing_window_size <= 0) return fail(e, SPX_ERR_ARG, "LowRiskOverCommitment: SmoothingWindowSize must be positive");
  if (!(p->risk_limit_weight_cpu >= 0 && p->risk_limit_weight_cpu <= 1) || !(p->risk_limit_weight_mem >= 0 && p->risk_limit_weight_mem <= 1))
    return fail(e, SPX_ERR_ARG, "LowRiskOverCommitment: RiskLimitWeights must be in [0,1]");  // validation_pluginargs.go
  e->lroc = *p;
  e->lroc_tab_ready = false;
  return SPX_OK;
}

int spx_upload_lroc_nodes(spx_engine* e, const spx_lroc_nodes_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (!e->tri_nodes) return fail(e, SPX_ERR_STATE, "LowRiskOverCommitment reads the trimaran node table: upload it first");
  int rc = set_nodes(e, t->n_nodes);
  if (rc) return rc;
  const size_t n = static_cast<size_t>(t->n_nodes);
  if ((rc = upload(e, e->d_lroc_nreq_c, t->req_cpu_milli, n * 8))) return rc;
  if ((rc = upload(e, e->d_lroc_nreq_m, t->req_mem, n * 8))) return rc;
  if ((rc = upload(e, e->d_lroc_nlim_c, t->lim_cpu_milli, n * 8))) return rc;
  if ((rc = upload(e, e->d_lroc_nlim_m, t->lim_mem, n * 8))) return rc;
  e->lroc_nodes_exact = all_below_2p52(t->req_cpu_milli, n) && all_below_2p52(t->req_mem, n) && all_below_2p52(t->lim_cpu_milli, n) &&
                        all_below_2p52(t->lim_mem, n);
  e->lroc_nodes_f32 = all_below_2p47(t->req_cpu_milli, n) && all_below_2p47(t->req_mem, n) && all_below_2p47(t->lim_cpu_milli, n) && all_below_2p47(t->lim_mem, n) &&
                      none_below(t->lim_cpu_milli, t->req_cpu_milli, n) && none_below(t->lim_mem, t->req_mem, n);
  const int64_t* ncols[4] = {t->req_cpu_milli, t->req_mem, t->lim_cpu_milli, t->lim_mem};
  for (int c = 0; c < 4; ++c) e->lroc_node_max[c] = n ? *std::max_element(ncols[c], ncols[c] + n) : 0;
  e->lroc_nodes_cover = none_below(t->lim_cpu_milli, t->req_cpu_milli, n) && none_below(t->lim_mem, t->req_mem, n);
  e->lroc_last_form = -1;
  e->lroc_nodes = true;
  e->lroc_tab_ready = false;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

int spx_upload_lroc_pods(spx_engine* e, const spx_lroc_pods_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  int rc = set_pods(e, t->n_pods);
  if (rc) return rc;
  const size_t p = static_cast<size_t>(t->n_pods);
  if ((rc = upload(e, e->d_lroc_preq_c, t->req_cpu_milli, p * 8))) return rc;
  if ((rc = upload(e, e->d_lroc_preq_m, t->req_mem, p * 8))) return rc;
  if ((rc = upload(e, e->d_lroc_plim_c, t->lim_cpu_milli, p * 8))) return rc;
  if ((rc = upload(e, e->d_lroc_plim_m, t->lim_mem, p * 8))) return rc;
  e->lroc_pods_exact = all_below_2p52(t->req_cpu_milli, p) && all_below_2p52(t->req_mem, p) && all_below_2p52(t->lim_cpu_milli, p) &&
                       all_below_2p52(t->lim_mem, p);
  e->lroc_pods_f32 = e->lroc_pods_exact && all_below_2p47(t->req_cpu_milli, p) && all_below_2p47(t->req_mem, p) && all_below_2p47(t->lim_cpu_milli, p) &&
                     all_below_2p47(t->lim_mem, p) && none_below(t->lim_cpu_milli, t->req_cpu_milli, p) && none_below(t->lim_mem, t->req_mem, p);
  if (e->lroc_pods_f32) {
    // the float32 sweep's pod records, 32 bytes each (one scalar load): the limits' high float32 parts (cpu, memory), their low parts (exact below
    // 2^47), limit - request as the float32 it is used as, and a marker for the pod without requests and limits
    std::vector<float> f(8 * p);
    for (size_t i = 0; i < p; ++i) {
      float* r = &f[8 * i];
      const bool none = t->req_cpu_milli[i] == 0 && t->req_mem[i] == 0 && t->lim_cpu_milli[i] == 0 && t->lim_mem[i] == 0;
      const double lc = static_cast<double>(t->lim_cpu_milli[i]), lm = static_cast<double>(t->lim_mem[i]);
      r[0] = static_cast<float>(lc), r[2] = static_cast<float>(lc - static_cast<double>(r[0]));
      r[1] = static_cast<float>(lm), r[3] = static_cast<float>(lm - static_cast<double>(r[1]));
      r[4] = static_cast<float>(static_cast<double>(t->lim_cpu_milli[i] - t->req_cpu_milli[i]));
      r[5] = static_cast<float>(static_cast<double>(t->lim_mem[i] - t->req_mem[i]));
      r[6] = none ? 1.0f : 0.0f, r[7] = 0.0f;
    }
    if ((rc = upload(e, e->d_lroc_podf, f.data(), f.size() * sizeof(float)))) return rc;
    SPX_HIP(e, hipStreamSynchronize(e->stream));  // f goes out of scope
  }
  const int64_t* pcols[4] = {t->req_cpu_milli, t->req_mem, t->lim_cpu_milli, t->lim_mem};
  for (int c = 0; c < 4; ++c) e->h_lroc_pod[c].assign(pcols[c], pcols[c] + p);
  e->lroc_pods_cover = none_below(t->lim_cpu_milli, t->req_cpu_milli, p) && none_below(t->lim_mem, t->req_mem, p);
  e->lroc_last_form = -1;
  e->lroc_pods = true;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

int spx_upload_peaks_nodes(spx_engine* e, const spx_peaks_nodes_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  int rc = set_nodes(e, t->n_nodes);
  if (rc) return rc;
  const size_t n = static_cast<size_t>(t->n_nodes);
  if ((rc = upload(e, e->d_pk_cap, t->cap_cpu_milli, n * 8))) return rc;
  if ((rc = upload(e, e->d_pk_util, t->cpu_util, n * 8))) return rc;
  if ((rc = upload(e, e->d_pk_valid, t->valid, n))) return rc;
  if ((rc = upload(e, e->d_pk_k1, t->k1, n * 8))) return rc;
  if ((rc = upload(e, e->d_pk_k2, t->k2, n * 8))) return rc;
  e->peaks_nodes = true;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

int spx_upload_peaks_pods(spx_engine* e, const spx_peaks_pods_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  int rc = set_pods(e, t->n_pods);
  if (rc) return rc;
  if ((rc = upload(e, e->d_pk_pod, t->cpu_milli, static_cast<size_t>(t->n_pods) * 8))) return rc;
  // Pod classes: the pod's cpu request is all Peaks.Score reads of it (peaks.go:134-138), so rows of equal requests are equal —
  // raw scores always, normalised scores when every pod's node list is the whole snapshot.  First row of each distinct value
  // (flat open-addressing table, rows in order), the others as (row, representative) pairs.
  e->pk_n_uniq = e->pk_n_dups = 0;
  e->pk_negative = false;
  for (int64_t i = 0; i < t->n_pods; ++i)
    if (t->cpu_milli[i] < 0) e->pk_negative = true;
  if (t->n_pods > 1) {
    const size_t p = static_cast<size_t>(t->n_pods);
    size_t cap = 64;
    while (cap < 2 * p) cap <<= 1;
    std::vector<int32_t> tab(cap, -1), uniq, dups;
    uniq.reserve(p), dups.reserve(2 * p);
    for (size_t i = 0; i < p; ++i) {
      const int64_t v = t->cpu_milli[i];
      size_t k = static_cast<size_t>((static_cast<uint64_t>(v) * 0x9e3779b97f4a7c15ull) >> 24) & (cap - 1);
      while (tab[k] >= 0 && t->cpu_milli[tab[k]] != v) k = (k + 1) & (cap - 1);
      if (tab[k] < 0) tab[k] = static_cast<int32_t>(i), uniq.push_back(static_cast<int32_t>(i));
      else dups.push_back(static_cast<int32_t>(i)), dups.push_back(tab[k]);
    }
    if (!dups.empty()) {
      if ((rc = ship_classes(e, e->d_pk_uniq, e->d_pk_dups, uniq, dups, t->n_pods, e->pk_n_uniq, e->pk_n_dups, e->pk_n_tasks))) return rc;
    }
  }
  e->peaks_pods = true;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

int spx_upload_sysched_nodes(spx_engine* e, const spx_sysched_nodes_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (t->n_words < 1 || t->n_words > SPX_SYSCHED_MAX_WORDS) return fail(e, SPX_ERR_ARG, "SySched: n_words must be in [1, SPX_SYSCHED_MAX_WORDS]");
  int rc = set_nodes(e, t->n_nodes);
  if (rc) return rc;
  const size_t n = static_cast<size_t>(t->n_nodes);
  e->sy_nodes = false;
  if ((rc = ensure(e, e->d_sy_host, n * static_cast<size_t>(t->n_words) * 8)) || (rc = ensure(e, e->d_sy_present, n)) || (rc = ensure(e, e->d_sy_k, n * 4)) ||
      (rc = ensure(e, e->d_sy_a, n * 4)))
    return rc;
  std::vector<int32_t> ix(n);
  for (size_t i = 0; i < n; ++i) ix[i] = static_cast<int32_t>(i);
  if ((rc = ship_sysched_rows(e, t, ix, true))) return rc;
  e->sy_node_words = t->n_words;
  e->sy_nodes = true;
  e->evaluated &= ~(1u << SPX_PLUGIN_SYSCHED);
  e->best_valid = false;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

int spx_update_sysched_nodes(spx_engine* e, const int64_t* idx, const spx_sysched_nodes_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (!e->sy_nodes) return fail(e, SPX_ERR_STATE, "SySched node delta: upload the full table first");
  if (t->n_words != e->sy_node_words) return fail(e, SPX_ERR_ARG, "SySched node delta: n_words differs from the table in place");
  const int64_t n = t->n_nodes;
  if (n == 0) return SPX_OK;
  std::vector<int32_t> ix;
  int rc = delta_indices(e, idx, n, ix);
  if (rc) return rc;
  if ((rc = ship_sysched_rows(e, t, ix, false))) return rc;
  e->evaluated = 0;  // every table computed from the old rows is stale
  e->best_valid = false;
  SPX_HIP(e, hipStreamSynchronize(e->stream));  // host columns are only borrowed for the call
  return SPX_OK;
}

int spx_upload_sysched_pods(spx_engine* e, const spx_sysched_pods_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (t->n_words < 1 || t->n_words > SPX_SYSCHED_MAX_WORDS) return fail(e, SPX_ERR_ARG, "SySched: n_words must be in [1, SPX_SYSCHED_MAX_WORDS]");
  if (t->n_sets < 1 || !t->set_bits || !t->pod_set) return fail(e, SPX_ERR_ARG, "SySched: the pod table needs at least one set");
  int rc = set_pods(e, t->n_pods);
  if (rc) return rc;
  const size_t P = static_cast<size_t>(t->n_pods), S = static_cast<size_t>(t->n_sets), W = static_cast<size_t>(t->n_words);
  // Pod classes are the sets: a pod enters Score through getSyscalls(pod) alone (sysched.go:244).  The pods in (set, row) order, each
  // set's first position in that order, and the (row, representative) pairs of the pods that are not the first with their set.
  std::vector<int32_t> first(S + 1, 0), order(P), dups;
  for (size_t p = 0; p < P; ++p) {
    if (t->pod_set[p] < 0 || static_cast<size_t>(t->pod_set[p]) >= S) return fail(e, SPX_ERR_ARG, "SySched: pod_set out of range");
    ++first[static_cast<size_t>(t->pod_set[p]) + 1];
  }
  for (size_t s = 0; s < S; ++s) first[s + 1] += first[s];
  {
    std::vector<int32_t> at(first.begin(), first.end() - 1);
    for (size_t p = 0; p < P; ++p) order[static_cast<size_t>(at[static_cast<size_t>(t->pod_set[p])]++)] = static_cast<int32_t>(p);
  }
  for (size_t p = 0; p < P; ++p) {
    const int32_t rep = order[static_cast<size_t>(first[static_cast<size_t>(t->pod_set[p])])];
    if (rep != static_cast<int32_t>(p)) dups.push_back(static_cast<int32_t>(p)), dups.push_back(rep);
  }
  std::vector<uint8_t> empty(S);
  for (size_t s = 0; s < S; ++s) {
    uint64_t any = 0;
    for (size_t w = 0; w < W; ++w) any |= t->set_bits[s * W + w];
    empty[s] = any == 0;
  }
  e->sy_pods = false;
  e->sy_n_dups = static_cast<int64_t>(dups.size() / 2);
  e->sy_n_tasks = expand_tasks(dups, t->n_pods);
  if ((rc = upload(e, e->d_sy_sets, t->set_bits, S * W * 8)) || (rc = upload(e, e->d_sy_empty, empty.data(), S)) || (rc = upload(e, e->d_sy_pod_set, t->pod_set, P * 4)) ||
      (rc = upload(e, e->d_sy_order, order.data(), P * 4)) || (rc = upload(e, e->d_sy_first, first.data(), (S + 1) * 4)) ||
      (rc = upload(e, e->d_sy_dups, dups.data(), dups.size() * 4)))
    return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->h_sy_pod_set.assign(t->pod_set, t->pod_set + P);
  e->h_sy_first = std::move(first);
  e->sy_pod_words = t->n_words;
  e->sy_n_sets = t->n_sets;
  e->sy_pods = true;
  e->evaluated &= ~(1u << SPX_PLUGIN_SYSCHED);
  e->best_valid = false;
  return SPX_OK;
}

int spx_upload_cosched(spx_engine* e, const spx_cosched_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (t->n_slots < 1 || t->n_slots > SPX_COSCHED_MAX_SLOTS || !t->slot_res) return fail(e, SPX_ERR_ARG, "Coscheduling: n_slots must be in [1, SPX_COSCHED_MAX_SLOTS]");
  if (t->n_groups < 0 || t->n_nodes <= 0 || t->n_pods <= 0 || !t->left_base || !t->node_present || !t->pod_group) return fail(e, SPX_ERR_ARG, "NULL column in table");
  const size_t N = static_cast<size_t>(t->n_nodes), G = static_cast<size_t>(t->n_groups), P = static_cast<size_t>(t->n_pods), S = static_cast<size_t>(t->n_slots);
  if (G && (!t->g_exists || !t->min_member || !t->has_min_resources || !t->backed_off || !t->permitted || !t->listed || !t->gated || !t->req || !t->req_mask || !t->step_ptr))
    return fail(e, SPX_ERR_ARG, "NULL column in table");
  for (size_t p = 0; p < P; ++p)
    if (t->pod_group[p] < -1 || t->pod_group[p] >= t->n_groups) return fail(e, SPX_ERR_ARG, "Coscheduling: pod_group out of range");
  // the steps: strictly ascending present nodes per group, non-negative add-backs; summed per group on the way (the walk reads the
  // add-backs of every step up to a node as one number)
  const int32_t zero_ptr[1] = {0};
  const int32_t* sptr = G ? t->step_ptr : zero_ptr;
  if (sptr[0] != 0) return fail(e, SPX_ERR_ARG, "Coscheduling: step_ptr must start at 0");
  const size_t n_steps = static_cast<size_t>(sptr[G]);
  if (n_steps && (!t->step_node || !t->step_add)) return fail(e, SPX_ERR_ARG, "NULL column in table");
  std::vector<int32_t> walk;
  for (size_t g = 0; g < G; ++g) {
    if (sptr[g + 1] < sptr[g]) return fail(e, SPX_ERR_ARG, "Coscheduling: step_ptr is not monotone");
    if (t->req_mask[g] >> S) return fail(e, SPX_ERR_ARG, "Coscheduling: req_mask names a slot beyond n_slots");
    if (sptr[g + 1] > sptr[g]) walk.push_back(static_cast<int32_t>(g));
    for (int32_t k = sptr[g]; k < sptr[g + 1]; ++k) {
      const int32_t node = t->step_node[k];
      if (node < 0 || static_cast<size_t>(node) >= N || !t->node_present[node] || (k > sptr[g] && node <= t->step_node[k - 1]))
        return fail(e, SPX_ERR_ARG, "Coscheduling: a group's steps must be strictly ascending present nodes");
      for (size_t r = 0; r < S; ++r)
        if (t->step_add[static_cast<size_t>(k) * S + r] < 0) return fail(e, SPX_ERR_ARG, "Coscheduling: negative add-back");
    }
  }
  int32_t bad_slot = -1;
  if (spx_cosched_check(t, &bad_slot) != SPX_OK)
    return fail(e, SPX_ERR_ARG, "Coscheduling: slot " + std::to_string(bad_slot) + " (resource id " + std::to_string(bad_slot >= 0 ? t->slot_res[bad_slot] : -1) +
                                    "): the left-overs and add-backs sum to 2^62 or more, or a request does; the device sums are int64");
  std::vector<int64_t> cum(n_steps * S + 1, 0);
  for (size_t g = 0; g < G; ++g)
    for (int32_t k = sptr[g]; k < sptr[g + 1]; ++k)
      for (size_t r = 0; r < S; ++r)
        cum[static_cast<size_t>(k) * S + r] = t->step_add[static_cast<size_t>(k) * S + r] + (k > sptr[g] ? cum[static_cast<size_t>(k - 1) * S + r] : 0);
  int rc = set_nodes(e, t->n_nodes);
  if (rc) return rc;
  if ((rc = set_pods(e, t->n_pods))) return rc;
  e->cosched = e->cs_gate_valid = false;
  e->evaluated &= ~(1u << SPX_PLUGIN_COSCHED);
  e->best_valid = false;
  e->cs_row_begin = e->cs_row_end = 0;
  if ((rc = upload(e, e->d_cs_left, t->left_base, S * N * 8)) || (rc = upload(e, e->d_cs_present, t->node_present, N)) || (rc = ensure(e, e->d_cs_prefix, S * N * 8)) ||
      (rc = ensure(e, e->d_cs_smax, S * 8)) || (rc = ensure(e, e->d_cs_stotal, S * 8)) || (rc = ensure(e, e->d_cs_any, 4)) || (rc = upload(e, e->d_cs_req, t->req, G * S * 8)) ||
      (rc = upload(e, e->d_cs_mask, t->req_mask, G * 4)) || (rc = upload(e, e->d_cs_sptr, sptr, (G + 1) * 4)) || (rc = upload(e, e->d_cs_snode, t->step_node, n_steps * 4)) ||
      (rc = upload(e, e->d_cs_scum, cum.data(), n_steps * S * 8)) || (rc = upload(e, e->d_cs_walk, walk.data(), walk.size() * 4)) || (rc = ensure(e, e->d_cs_pass, G * 4)) ||
      (rc = ensure(e, e->d_cs_open, G * 4)) || (rc = ensure(e, e->d_cs_gap, G * S * 8)) || (rc = upload(e, e->d_cs_exists, t->g_exists, G)) ||
      (rc = upload(e, e->d_cs_minm, t->min_member, G * 4)) || (rc = upload(e, e->d_cs_hasres, t->has_min_resources, G)) || (rc = upload(e, e->d_cs_backoff, t->backed_off, G)) ||
      (rc = upload(e, e->d_cs_permit, t->permitted, G)) || (rc = upload(e, e->d_cs_listed, t->listed, G * 4)) || (rc = upload(e, e->d_cs_gated, t->gated, G * 4)) ||
      (rc = upload(e, e->d_cs_pod_group, t->pod_group, P * 4)) || (rc = ensure(e, e->d_cs_status, P)))
    return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));  // the host columns are only borrowed for the call
  e->cs_n_slots = t->n_slots;
  e->cs_n_groups = t->n_groups;
  e->cs_n_walk = static_cast<int32_t>(walk.size());
  e->cosched = true;
  return SPX_OK;
}

int spx_fetch_cosched_gap(spx_engine* e, int32_t group_begin, int32_t group_end, uint32_t* pass_mask, uint32_t* open_mask, int64_t* gap) {
  if (!e) return SPX_ERR_ARG;
  if (!e->cosched || !e->cs_gate_valid) return fail(e, SPX_ERR_STATE, "Coscheduling's gate has not been evaluated since its last upload");
  if (group_begin < 0 || group_end > e->cs_n_groups || group_begin > group_end) return fail(e, SPX_ERR_ARG, "group range out of bounds");
  SPX_HIP(e, hipSetDevice(e->device));
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  const size_t n = static_cast<size_t>(group_end - group_begin), S = static_cast<size_t>(e->cs_n_slots);
  if (n == 0) return SPX_OK;
  if (pass_mask) SPX_HIP(e, hipMemcpy(pass_mask, static_cast<const uint32_t*>(e->d_cs_pass.p) + group_begin, n * 4, hipMemcpyDeviceToHost));
  if (open_mask) SPX_HIP(e, hipMemcpy(open_mask, static_cast<const uint32_t*>(e->d_cs_open.p) + group_begin, n * 4, hipMemcpyDeviceToHost));
  if (gap) SPX_HIP(e, hipMemcpy(gap, static_cast<const int64_t*>(e->d_cs_gap.p) + static_cast<size_t>(group_begin) * S, n * S * 8, hipMemcpyDeviceToHost));
  return SPX_OK;
}

int spx_upload_trimaran_pods(spx_engine* e, const spx_trimaran_pods_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  int rc = set_pods(e, t->n_pods);
  if (rc) return rc;
  const size_t p = static_cast<size_t>(t->n_pods);
  e->tlp_order_valid = false;  // (before the column changes: a failed upload must not leave an order that describes the old one)
  if ((rc = upload(e, e->d_tlp_pod, t->tlp_pod_milli, p * 8))) return rc;
  if ((rc = upload(e, e->d_lv_rcpu, t->lv_req_cpu_milli, p * 8))) return rc;
  if ((rc = upload(e, e->d_lv_rmem, t->lv_req_mem, p * 8))) return rc;
  e->tri_pods = true;
  if ((rc = tlp_build_order(e))) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

int spx_set_nrt_params(spx_engine* e, const spx_nrt_params* p) {
  if (!e || !p) return SPX_ERR_ARG;
  if (p->strategy < SPX_NRT_MOST_ALLOCATED || p->strategy > SPX_NRT_LEAST_NUMA_NODES)
    return fail(e, SPX_ERR_ARG, "illegal scoring strategy found");  // score.go:137-139
  if (e->nrt_params.strategy != p->strategy) {  // the packed Score's table of exceptions and the fused walk's items are per strategy
    e->nrt_pk_tab_built = e->nrt_wsort_built = false;
    ++e->nrt_items_gen;
  }
  e->nrt_params.strategy = p->strategy;  // weights travel through the slot table (spx_flatten_nrt_slots)
  return SPX_OK;
}

int spx_upload_nrt_slots(spx_engine* e, const spx_nrt_slots* t) {
  if (!e || !t) return SPX_ERR_ARG;
  if (t->n_res < 0 || t->n_res > SPX_NRT_MAX_RES) return fail(e, SPX_ERR_ARG, "NRT: more resource slots than this build supports");
  if (e->nrt_wide) {  // back from the wide tables: nothing of the dense state survives them (spx_upload_nrt_slots_wide)
    e->nrt_wide = false;
    e->nrtw_slots = e->nrtw_nodes = e->nrtw_pods = false;
    e->nrt_fz_key = spx_engine::FzKey{};
    e->nrt_pk_tab_built = e->nrt_wsort_built = false;
  }
  e->nrt_n_res = t->n_res;
  for (int i = 0; i < t->n_res; ++i) {
    e->nrt_slot_flags[i] = t->slot_flags[i];
    e->nrt_slot_weight[i] = t->slot_weight[i];
    e->nrt_slot_res[i] = t->slot_res ? t->slot_res[i] : -1;
  }
  e->nrt_slots = true;
  ++e->nrt_items_gen;
  e->nrt_nodes = e->nrt_pods = false;  // tables are laid out by slot count
  e->h_nrt_tall_nodes.clear();         // (the tall nodes' side table too)
  e->nrt_tall_ok = true;
  e->nrt_tall_last = 0;
  // float64 formulation: weight-subset table, cpu slot, weight range
  SPX_HIP(e, hipSetDevice(e->device));
  NrtSlotWeights w = nrt_slot_weights(t);
  e->nrt_cpu_slot = w.cpu_slot;
  e->nrt_fast_slots = w.fast;
  e->nrt_wtab = std::move(w.wtab);
  return SPX_OK;
}

int spx_upload_nrt_nodes(spx_engine* e, const spx_nrt_nodes_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (!e->nrt_slots || t->n_res != e->nrt_n_res) return fail(e, SPX_ERR_STATE, "NRT: upload the slot table first (n_res mismatch)");
  int rc = set_nodes(e, t->n_nodes);
  if (rc) return rc;
  e->nrt_nodes = false;  // (a call that fails half-way leaves "no NRT node table", not a mix of two)
  const int64_t n = t->n_nodes;
  constexpr int64_t Zm = SPX_NRT_MAX_ZONES;
  const int64_t R = t->n_res;
  if (!t->flags || !t->max_numa || !t->n_zones || !t->zone_id || !t->zone_present || !t->zone_cost || !t->min_avg_dist || !t->node_present ||
      (!t->zone_avail && R))
    return fail(e, SPX_ERR_ARG, "NULL column in table");
  // tall nodes (n_zones = SPX_NRT_ZONES_TALL): their zones come with spx_upload_nrt_tall_nodes; the dense sweeps see them as nodes without
  // zones (every column of this call holds 0 for them), and kernels_nrt_tall.hip overwrites their columns afterwards.  An older side
  // table goes with the node table it described.
  e->h_nrt_tall_nodes.clear();
  for (int64_t i = 0; i < n; ++i)
    if (t->n_zones[i] == SPX_NRT_ZONES_TALL) e->h_nrt_tall_nodes.push_back(static_cast<int32_t>(i));
  e->nrt_tall_ok = e->h_nrt_tall_nodes.empty();
  e->nrt_tall_last = 0;
  e->nrt_tall_stride = 0;
  e->nrt_tall_ln_node = -1, e->nrt_tall_ln_zones = 0;
  std::vector<uint8_t> nz_dense;
  spx_nrt_nodes_soa dense = *t;
  if (!e->h_nrt_tall_nodes.empty()) {
    nz_dense.assign(t->n_zones, t->n_zones + n);
    for (const int32_t i : e->h_nrt_tall_nodes) nz_dense[static_cast<size_t>(i)] = 0;
    dense.n_zones = nz_dense.data();
    t = &dense;
  }
  // Round 4: the full upload takes the delta's road (ship_nrt_rows) with every node listed — the rows as they are into ONE pinned
  // blob, one DMA, and the device derives the rest (the derived columns used to be computed here, on the host, into five freshly
  // allocated vectors that were then copied from pageable memory: 12.6 of the 24 ms a full snapshot load took at 20 000 nodes).
  // What is this call's own: the buffers, the preconditions of the float64 formulation as a fresh start, the window-local node order,
  // the host copy LeastNUMANodes' tables are built from.
  const size_t m = static_cast<size_t>(n), cells = static_cast<size_t>(Zm * R) * m;
  if ((rc = ensure(e, e->d_nrt_flags, m)) || (rc = ensure(e, e->d_nrt_max_numa, m * 4)) || (rc = ensure(e, e->d_nrt_nz, m)) || (rc = ensure(e, e->d_nrt_np, m)) ||
      (rc = ensure(e, e->d_nrt_zid, m * Zm)) || (rc = ensure(e, e->d_nrt_zp, m * Zm)) || (rc = ensure(e, e->d_nrt_avail, cells * 8)) ||
      (rc = ensure(e, e->d_nrt_cost, m * Zm * Zm * 4)) || (rc = ensure(e, e->d_nrt_minavg, m * Zm * 4)) || (rc = ensure(e, e->d_nrt_fav, cells * 8)) ||
      (rc = ensure(e, e->d_nrt_frc, cells * 8)) || (rc = ensure(e, e->d_nrt_frcv, cells * 8)) || (rc = ensure(e, e->d_nrt_fcpu, m * Zm * 8)) ||
      (rc = ensure(e, e->d_nrt_fbraw, m * Zm * 8)) || (rc = ensure(e, e->d_nrt_frep, static_cast<size_t>(R > 0 ? R : 1) * m)))
    return rc;
  {
    NrtRowScan scan;
    std::mutex scan_mu;
    spx_host::parallel_rows(n, [&](int64_t row0, int64_t row1) {
      const NrtRowScan part = nrt_scan_rows(t, e->nrt_cpu_slot, row0, row1);
      std::lock_guard<std::mutex> g(scan_mu);
      scan.merge(part);
    }, 1024);
    e->nrt_fast_nodes = scan.ok;
    e->nrt_big_nodes = scan.big;
    e->nrt_qty_nodes = scan.qty;
    e->nrt_pk_tab_built = e->nrt_wsort_built = false;
    e->nrt_ln_ok = scan.ln_ok;
    e->nrt_ln_built = false;  // built when that strategy is first evaluated (build_ln_tab): more host time than everything else in this call
    // window-local node order: inside each run of 256 nodes, group the nodes by the code path their flags select
    // (not aligned / pod scope / container scope) so that wavefronts are mostly homogeneous; inside a group, by how tight the
    // node's two largest zones are (the smaller of its ranks, within the window, by the sum of the two largest zone quantities of
    // slot 0 and of slot 1 — cpu and memory): LeastNUMANodes' second pass runs for a wave when one of its lanes needs more than two
    // zones, and those lanes are the tight nodes — sorted, they share waves (config #3: 69 % -> 37 % of the waves)
    const int64_t n_slots = spx::round_up(n, 256);
    std::vector<int32_t> perm(static_cast<size_t>(n_slots), -1);
    spx_host::parallel_rows((n + 255) / 256, [&](int64_t win0, int64_t win1) {
    for (int64_t w0 = win0 * 256; w0 < std::min<int64_t>(win1 * 256, n); w0 += 256) {
      const int64_t w1 = std::min<int64_t>(w0 + 256, n);
      const int cnt = static_cast<int>(w1 - w0);
      int rank[2][256];
      for (int slot = 0; slot < 2; ++slot) {
        int64_t top2[256];
        int order[256];
        for (int k = 0; k < cnt; ++k) {
          const int64_t i = w0 + k;
          int64_t a = 0, b = 0;  // the two largest
          if (slot < R)
            for (int z = 0; z < t->n_zones[i] && z < Zm; ++z) {
              if (!((t->zone_present[i * Zm + z] >> slot) & 1u)) continue;
              const int64_t q = t->zone_avail[(i * Zm + z) * R + slot];
              if (q > a) b = a, a = q;
              else if (q > b) b = q;
            }
          top2[k] = a + b;
          order[k] = k;
        }
        std::stable_sort(order, order + cnt, [&](int x, int y) { return top2[x] < top2[y]; });
        for (int k = 0; k < cnt; ++k) rank[slot][order[k]] = k;
      }
      int order[256], cls_of[256], key[256];
      for (int k = 0; k < cnt; ++k) {
        const uint8_t f = t->flags[w0 + k];
        const bool aligned = (f & SPX_NRT_F_FRESH) && (f & SPX_NRT_F_HAS_NRT) && (f & SPX_NRT_F_SINGLE_NUMA);
        cls_of[k] = !aligned ? 0 : ((f & SPX_NRT_F_POD_SCOPE) ? 1 : 2);
        key[k] = std::min(rank[0][k], rank[1][k]);
        order[k] = k;
      }
      std::stable_sort(order, order + cnt, [&](int x, int y) { return cls_of[x] != cls_of[y] ? cls_of[x] < cls_of[y] : key[x] < key[y]; });
      for (int k = 0; k < cnt; ++k) perm[static_cast<size_t>(w0 + k)] = static_cast<int32_t>(w0 + order[k]);
    }
    }, 2);  // (three 256-key stable sorts per window, ~40 us: at 16 windows per thread config #5's 79 windows ran on 4 threads for 1 ms)
    std::vector<int32_t> all(m);
    for (size_t i = 0; i < m; ++i) all[i] = static_cast<int32_t>(i);
    DeltaBlob b{e};
    const size_t o_perm = b.add(perm.data(), perm.size() * sizeof(int32_t));
    if ((rc = ensure(e, e->d_nrt_perm, perm.size() * sizeof(int32_t)))) return rc;
    if ((rc = ship_nrt_rows(e, t, all, true, b))) return rc;
    e->h_nrt_cost.assign(t->zone_cost, t->zone_cost + m * Zm * Zm);  // (the host copies follow the shipped rows)
    e->h_nrt_nz.assign(t->n_zones, t->n_zones + m);
    SPX_HIP(e, hipMemcpyAsync(e->d_nrt_perm.p, b.dev(o_perm), perm.size() * sizeof(int32_t), hipMemcpyDeviceToDevice, e->stream));
    SPX_HIP(e, hipStreamSynchronize(e->stream));  // the blob is reused by the next staged call
  }
  e->nrt_nodes = true;
  return SPX_OK;
}

// LeastNUMANodes: per node the subsets of list positions at the node's minimum average distance for their size, and
// bit-planes of every subset's distance rank within its size (layout: LnLayout, spx_internal.h).  The average distance
// is nodesAvgDistance least_numa.go:115-138 — the sum over all ordered pairs, float32(sum) / float32(k*k); for one size
// the divisor is shared and sums below 2^14 stay distinct after the division, so ranking the integer sums ranks the
// reference's float32 values.  Only subsets of the node's own zones take part in the minimum (:102-113).
// Host-only; exported (not part of spx.h) so that tests/test_ln_tables.py can replay the kernel's selection against the
// reference's walk without a GPU.  zone_cost [n][Z][Z], n_zones [n], out [LnLayout.rows][n] zero-initialised by the callee.
int spx_internal_ln_tables(const int32_t* cost, const uint8_t* n_zones, int64_t n, uint32_t* tab) {
  if (!cost || !n_zones || !tab || n < 0) return SPX_ERR_ARG;
  constexpr int64_t Zm = SPX_NRT_MAX_ZONES;
  constexpr spx::LnLayout L = spx::make_ln_layout();
  std::fill(tab, tab + static_cast<size_t>(L.rows) * static_cast<size_t>(n), 0u);
  spx_host::parallel_rows(n, [&](int64_t row0, int64_t row1) {
    for (int64_t i = row0; i < row1; ++i) {
      const int nz = std::min<int>(n_zones[i], static_cast<int>(Zm));
      for (int k = 1; k <= 8; ++k) {
        int sums[70], order[70], cnt = 0;
        bool exists[70];
        for (int d = 0; d < L.nd[k]; ++d)
          for (int q = 0; q < L.cnt[L.first[k] + d]; ++q) {
            const unsigned m = L.subset[L.first[k] + d][q];
            int accu = 0;
            for (int za = 0; za < Zm; ++za)
              if (m >> za & 1u)
                for (int zb = 0; zb < Zm; ++zb)
                  if (m >> zb & 1u) accu += cost[(i * Zm + za) * Zm + zb];
            exists[cnt] = (m >> nz) == 0;
            sums[cnt] = accu;
            order[cnt] = cnt;
            ++cnt;
          }
        std::sort(order, order + cnt, [&](int x, int y) { return sums[x] < sums[y]; });
        int rank_of[70], level = -1, last = 0;
        for (int j = 0; j < cnt; ++j) rank_of[j] = (1 << L.bits[k]) - 1;  // subsets past the node's zones: never candidates
        for (int j = 0; j < cnt; ++j) {
          const int sidx = order[j];
          if (!exists[sidx]) continue;
          if (level < 0 || sums[sidx] != last) ++level, last = sums[sidx];
          rank_of[sidx] = level;
        }
        for (int pos = 0; pos < cnt; ++pos) {
          const size_t d = static_cast<size_t>(L.first[k] + pos / 32);
          const uint32_t bit = 1u << (pos % 32);
          if (exists[pos] && rank_of[pos] == 0) tab[d * static_cast<size_t>(n) + static_cast<size_t>(i)] |= bit;
          for (int b = 0; b < L.bits[k]; ++b)
            if ((rank_of[pos] >> b) & 1)
              tab[static_cast<size_t>(spx::kLnDwords + L.pbase[k] + b * L.nd[k] + pos / 32) * static_cast<size_t>(n) + static_cast<size_t>(i)] |= bit;
        }
      }
    }
  }, 512);
  return SPX_OK;
}

// the bit layout itself, for the same tests: subset[12][32] zone masks, then cnt[12], first[9], nd[9], bits[9], pbase[9], rows
int spx_internal_ln_layout(uint8_t* subset, uint8_t* cnt, uint8_t* first, uint8_t* nd, uint8_t* bits, uint8_t* pbase, int32_t* rows) {
  if (!subset || !cnt || !first || !nd || !bits || !pbase || !rows) return SPX_ERR_ARG;
  constexpr spx::LnLayout L = spx::make_ln_layout();
  std::memcpy(subset, L.subset, sizeof L.subset);
  std::memcpy(cnt, L.cnt, sizeof L.cnt);
  std::memcpy(first, L.first, sizeof L.first);
  std::memcpy(nd, L.nd, sizeof L.nd);
  std::memcpy(bits, L.bits, sizeof L.bits);
  std::memcpy(pbase, L.pbase, sizeof L.pbase);
  *rows = L.rows;
  return SPX_OK;
}

int build_ln_tab(spx_engine* e) {
  if (e->nrt_ln_built || !e->nrt_ln_ok) return SPX_OK;
  constexpr spx::LnLayout L = spx::make_ln_layout();
  // [L.rows][N] per-node tables, then what every workgroup keeps in LDS (spx::LnConst: it used to be rebuilt by every block from
  // the constant-memory layout — 384 dependent byte loads per thread, ~30 us per block)
  const size_t per_node = static_cast<size_t>(L.rows) * static_cast<size_t>(e->n_nodes);
  std::vector<uint32_t> tab(per_node + spx::kLnConstWords);
  int rc = spx_internal_ln_tables(e->h_nrt_cost.data(), e->h_nrt_nz.data(), e->n_nodes, tab.data());
  if (rc) return fail(e, rc, "LeastNUMANodes tables");
  {
    uint32_t* allow = tab.data() + per_node;  // [256 zone sets V][kLnDwords]: the subsets inside V, in the bit layout
    for (uint32_t vset = 0; vset < 256; ++vset)
      for (int d = 0; d < spx::kLnDwords; ++d) {
        uint32_t bits = 0;
        for (int q = 0; q < 32; ++q) {
          const uint32_t sub = L.subset[d][q];
          if (sub != 0 && (sub & ~vset) == 0) bits |= 1u << q;
        }
        allow[vset * spx::kLnDwords + d] = bits;
      }
    std::memcpy(allow + 256 * spx::kLnDwords, L.subset, sizeof L.subset);  // [kLnDwords][32] bytes: bit position -> zone mask
  }
  if ((rc = upload(e, e->d_nrt_ln, tab.data(), tab.size() * sizeof(uint32_t)))) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->nrt_ln_built = true;
  return SPX_OK;
}

// builds the stream of `list` and ships it; e->nrt_rk_kind = kind on success, 0 when it does not fit, -1 when the batch has none
int nrt_rank_stream_upload(spx_engine* e, const uint32_t* items, const int32_t* list, size_t n_list, int kind) {
  std::vector<uint32_t> rk, rk_off, rk_first;
  uint32_t rk_max = 0;
  bool rk_ok = false, all_narrow = false;
  nrt_build_rank_stream(items, list, n_list, static_cast<size_t>(e->nrt_n_res), rk, rk_off, rk_first, &rk_max, &rk_ok, &all_narrow, e->option[SPX_OPT_NRT_RANK_NARROW] != 0);
  e->nrt_rk_max_dwords = 0;
  e->nrt_rk_kind = rk_ok ? 0 : -1;
  if (rk_ok && rk_max * sizeof(uint32_t) <= spx::kRkMaxChunkBytes) {
    int rc;
    if ((rc = upload(e, e->d_nrt_rk, rk.data(), rk.size() * sizeof(uint32_t)))) return rc;
    if ((rc = upload(e, e->d_nrt_rk_off, rk_off.data(), rk_off.size() * sizeof(uint32_t)))) return rc;
    if ((rc = upload(e, e->d_nrt_rk_first, rk_first.data(), rk_first.size() * sizeof(uint32_t)))) return rc;
    SPX_HIP(e, hipStreamSynchronize(e->stream));
    e->nrt_rk_max_dwords = rk_max;
    e->nrt_rk_chunks = static_cast<uint32_t>(rk_first.size() - 1);
    e->nrt_rk_all_narrow = all_narrow;
    e->nrt_rk_kind = kind;
  }
  return SPX_OK;
}

// The rank stream over EVERY row of the uploaded batch, in order (a whole-batch sweep without pod classes: SPX_OPT_NRT_POD_CLASSES 0,
// or a queue with too few repeats for them): built the first time such a sweep runs after an upload — the record stream comes back
// from the device (the host copy was staging) — and kept until the next upload or until a sweep over the classes replaces it.
int nrt_rank_stream(spx_engine* e, int kind) {
  if (e->nrt_rk_kind == kind) return SPX_OK;
  if (e->nrt_rk_kind < 0 || !e->nrt_fast_pods || e->n_pods <= 0) return SPX_OK;  // no finite stream for this batch: the float64 Filter
  if (kind == 1 && e->nrt_n_dups == 0) return SPX_OK;
  const size_t p = static_cast<size_t>(e->n_pods), R = static_cast<size_t>(e->nrt_n_res), IW = R <= 4 ? 16 : 32;
  std::vector<uint32_t> items(p * 10 * IW);
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  SPX_HIP(e, hipMemcpy(items.data(), e->d_nrt_items.p, items.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  std::vector<int32_t> list;
  if (kind == 2) {
    list.resize(p);
    for (size_t i = 0; i < p; ++i) list[i] = static_cast<int32_t>(i);
  } else {
    list.resize(static_cast<size_t>(e->nrt_n_uniq));
    SPX_HIP(e, hipMemcpy(list.data(), e->d_nrt_uniq.p, list.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return nrt_rank_stream_upload(e, items.data(), list.data(), list.size(), kind);
}

// test hook (host only, no device): the representative row of every pod of a batch, as spx_upload_nrt_pods computes it
// (rep_out[i] == i for a representative); *fast_ok_out = whether the batch satisfies the float64 formulation's preconditions
// (the classes are only built, and only used, when it does)
int spx_internal_nrt_pod_classes(const spx_nrt_slots* slots, const spx_nrt_pods_soa* t, int32_t* rep_out, int32_t* fast_ok_out) {
  if (!slots || !t || !rep_out || !fast_ok_out || t->n_res != slots->n_res || t->n_pods <= 0) return SPX_ERR_ARG;
  const int R = t->n_res;
  const NrtSlotWeights w = nrt_slot_weights(slots);  // (the weights only decide *fast_ok_out: out of range, no classes are built)
  const size_t p = static_cast<size_t>(t->n_pods), IW = R <= 4 ? 16 : 32;
  std::vector<uint32_t> items(p * 10 * IW);
  std::vector<uint64_t> hash(p);
  bool ok = false;
  uint32_t big = 0;
  nrt_build_items(t, slots->slot_flags, w.cpu_slot, w.wtab, items.data(), &ok, &big, hash.data());
  *fast_ok_out = (ok && w.fast) ? 1 : 0;
  for (size_t i = 0; i < p; ++i) rep_out[i] = static_cast<int32_t>(i);
  if (ok && w.fast) nrt_build_classes(items.data(), hash.data(), p, static_cast<size_t>(R), rep_out);
  return SPX_OK;
}

int spx_upload_nrt_pods(spx_engine* e, const spx_nrt_pods_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (!e->nrt_slots || t->n_res != e->nrt_n_res) return fail(e, SPX_ERR_STATE, "NRT: upload the slot table first (n_res mismatch)");
  int rc = set_pods(e, t->n_pods);
  if (rc) return rc;
  const size_t p = static_cast<size_t>(t->n_pods);
  const size_t R = static_cast<size_t>(t->n_res);
  constexpr size_t Cm = SPX_NRT_MAX_CTRS;
  if ((rc = upload(e, e->d_nrt_qos, t->qos, p))) return rc;
  if ((rc = upload(e, e->d_nrt_nn, t->non_native, p))) return rc;
  // long rows (n_ctr = SPX_NRT_CTRS_LONG): their containers come with spx_upload_nrt_long_pods; the dense sweeps see them as pods without
  // containers (the device column holds 0), and kernels_nrt_long.hip overwrites their cells afterwards
  e->h_nrt_long_rows.clear();
  for (size_t i = 0; i < p; ++i)
    if (t->n_ctr && t->n_ctr[i] == SPX_NRT_CTRS_LONG) e->h_nrt_long_rows.push_back(static_cast<int32_t>(i));
  e->nrt_long_ok = e->h_nrt_long_rows.empty();
  e->nrt_long_last = 0;
  if (e->h_nrt_long_rows.empty()) {
    if ((rc = upload(e, e->d_nrt_nctr, t->n_ctr, p))) return rc;
  } else {
    std::vector<uint8_t> nctr(t->n_ctr, t->n_ctr + p);
    for (const int32_t r : e->h_nrt_long_rows) nctr[static_cast<size_t>(r)] = 0;
    if ((rc = upload(e, e->d_nrt_nctr, nctr.data(), p))) return rc;
    SPX_HIP(e, hipStreamSynchronize(e->stream));  // (a local vector)
  }
  if ((rc = upload(e, e->d_nrt_ckind, t->ctr_kind, p * Cm))) return rc;
  if ((rc = upload(e, e->d_nrt_cpres, t->ctr_present, p * Cm))) return rc;
  if (!t->ctr_req && p * R) return fail(e, SPX_ERR_ARG, "NULL column in table");
  if ((rc = upload(e, e->d_nrt_ppres, t->pod_present, p))) return rc;
  if ((rc = upload(e, e->d_nrt_preq, t->pod_req, p * R * 8))) return rc;
  {  // float64 formulation: the pod record stream (nrt_build_items) + its preconditions, then the pod equivalence classes
    const size_t IW = R <= 4 ? 16 : 32;
    const size_t items_bytes = p * 10 * IW * sizeof(uint32_t);
    if ((rc = ensure_pinned(e, e->h_items, e->h_items_bytes, items_bytes, items_bytes >> 3))) return rc;
    uint32_t* const items = static_cast<uint32_t*>(e->h_items);  // pinned: built in place (rows zeroed by the thread that fills them)
    bool ok = false;
    uint32_t big = 0;
    std::vector<uint64_t> hash(p);
    spx_engine::NrtQty qty;
    nrt_build_items(t, e->nrt_slot_flags, e->nrt_cpu_slot, e->nrt_wtab, items, &ok, &big, hash.data(), &qty);
    if ((rc = upload(e, e->d_nrt_items, items, items_bytes))) return rc;  // from pinned memory: one DMA at link speed, asynchronous
    e->nrt_fast_pods = ok;
    e->nrt_big_pods = big;
    e->nrt_qty_pods = qty;
    e->nrt_pk_tab_built = false;  // (the table's unit and length follow the batch)
    // the reference-arithmetic kernel's request column: shipped only when the record stream cannot stand in for it
    e->nrt_creq_valid = false;
    if (!e->nrt_fast_pods) {
      if ((rc = upload(e, e->d_nrt_creq, t->ctr_req, p * Cm * R * 8))) return rc;
      e->nrt_creq_valid = true;
    }
    e->nrt_n_uniq = e->nrt_n_dups = 0;
    e->nrt_rk_max_dwords = 0;
    e->nrt_rk_kind = 0;
    ++e->nrt_items_gen;
    if (e->nrt_fast_pods && p > 0) {
      std::vector<int32_t> rep(p);
      nrt_build_classes(items, hash.data(), p, R, rep.data());
      std::vector<int32_t> uniq, dups;
      uniq.reserve(p), dups.reserve(2 * p);
      for (size_t i = 0; i < p; ++i) {
        if (rep[i] == static_cast<int32_t>(i)) uniq.push_back(static_cast<int32_t>(i));
        else dups.push_back(static_cast<int32_t>(i)), dups.push_back(rep[i]);
      }
      if (!dups.empty()) {
        if ((rc = ship_classes(e, e->d_nrt_uniq, e->d_nrt_dups, uniq, dups, t->n_pods, e->nrt_n_uniq, e->nrt_n_dups, e->nrt_n_tasks))) return rc;
        // the representatives' requests as ranks, per chunk of up to 32 (kernels_nrt_rank.hip, kernels_nrt_fused.hip)
        if ((rc = nrt_rank_stream_upload(e, items, uniq.data(), uniq.size(), 1))) return rc;
      }
    }
  }
  e->nrt_pods = true;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

int spx_upload_nrt_long_pods(spx_engine* e, const spx_nrt_long_pods* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (!e->nrt_pods) return fail(e, SPX_ERR_STATE, "NRT: upload the pod table (spx_upload_nrt_pods) before its long rows");
  if (t->n_long < 0 || t->n_res != e->nrt_n_res) return fail(e, SPX_ERR_ARG, "NRT long rows: n_long < 0 or n_res differs from the slot table");
  const std::vector<int32_t>& rows = e->h_nrt_long_rows;
  if (static_cast<size_t>(t->n_long) != rows.size())
    return fail(e, SPX_ERR_ARG, "NRT long rows: the table must list exactly the batch rows whose n_ctr is SPX_NRT_CTRS_LONG");
  if (t->n_long == 0) {
    e->nrt_long_ok = true;
    return SPX_OK;
  }
  if (!t->pod_row || !t->ctr_ptr) return fail(e, SPX_ERR_ARG, "NULL column in table");
  const size_t L = static_cast<size_t>(t->n_long), R = static_cast<size_t>(t->n_res);
  for (size_t k = 0; k < L; ++k)
    if (t->pod_row[k] != rows[k]) return fail(e, SPX_ERR_ARG, "NRT long rows: the table must list exactly the batch rows whose n_ctr is SPX_NRT_CTRS_LONG");
  if (t->ctr_ptr[0] != 0) return fail(e, SPX_ERR_ARG, "NRT long rows: ctr_ptr[0] must be 0");
  for (size_t k = 0; k < L; ++k)
    if (t->ctr_ptr[k + 1] - t->ctr_ptr[k] <= SPX_NRT_MAX_CTRS) return fail(e, SPX_ERR_ARG, "NRT long rows: a long row holds more than 8 containers");
  const size_t n_ctr = static_cast<size_t>(t->ctr_ptr[L]);
  e->nrt_long_ok = false;
  int rc;
  if ((rc = upload(e, e->d_nrtl_row, t->pod_row, L * 4)) || (rc = upload(e, e->d_nrtl_ptr, t->ctr_ptr, (L + 1) * 4)) ||
      (rc = upload(e, e->d_nrtl_kind, t->ctr_kind, n_ctr)) || (rc = upload(e, e->d_nrtl_pres, t->ctr_present, n_ctr)) ||
      (rc = upload(e, e->d_nrtl_req, t->ctr_req, n_ctr * R * 8)))
    return rc;
  std::vector<int32_t> map(static_cast<size_t>(e->n_pods), -1);  // batch row -> long row (the commit loop's row_indirect launches)
  for (size_t k = 0; k < L; ++k) map[static_cast<size_t>(rows[k])] = static_cast<int32_t>(k);
  if ((rc = upload(e, e->d_nrtl_map, map.data(), map.size() * 4))) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->nrt_long_ok = true;
  return SPX_OK;
}

int spx_upload_nrt_tall_nodes(spx_engine* e, const spx_nrt_tall_nodes* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (e->nrt_wide) return fail(e, SPX_ERR_STATE, "NRT: a wide snapshot (more than 8 resource slots) takes no nodes with more than 8 NUMA zones");
  if (!e->nrt_nodes) return fail(e, SPX_ERR_STATE, "NRT: upload the node table (spx_upload_nrt_nodes) before its tall nodes");
  if (t->n_tall < 0 || t->n_res != e->nrt_n_res) return fail(e, SPX_ERR_ARG, "NRT tall nodes: n_tall < 0 or n_res differs from the slot table");
  const std::vector<int32_t>& tall = e->h_nrt_tall_nodes;
  const char* const listing = "NRT tall nodes: the table must list exactly the nodes whose n_zones is SPX_NRT_ZONES_TALL";
  if (static_cast<size_t>(t->n_tall) != tall.size()) return fail(e, SPX_ERR_ARG, listing);
  if (t->n_tall == 0) {
    e->nrt_tall_ok = true;
    return SPX_OK;
  }
  const int64_t T = t->n_tall, S = t->zone_stride, R = t->n_res;
  if (!t->node_idx || !t->flags || !t->max_numa || !t->node_present || !t->n_zones || !t->zone_id || !t->zone_present || !t->zone_cost ||
      !t->min_avg_dist || (!t->zone_avail && R))
    return fail(e, SPX_ERR_ARG, "NULL column in table");
  if (S <= SPX_NRT_MAX_ZONES || S > SPX_NRT_TALL_MAX_ZONES) return fail(e, SPX_ERR_ARG, "NRT tall nodes: zone_stride must lie in 9..64");
  e->nrt_tall_ok = false;
  int32_t ln_node = -1, ln_zones = 0;
  for (int64_t k = 0; k < T; ++k) {
    if (t->node_idx[k] != tall[static_cast<size_t>(k)]) return fail(e, SPX_ERR_ARG, listing);
    const int nz = t->n_zones[k];
    if (nz <= SPX_NRT_MAX_ZONES || nz > S)
      return fail(e, SPX_ERR_ARG, "NRT tall nodes: node " + std::to_string(t->node_idx[k]) + " lists " + std::to_string(nz) + " zones; a tall node holds 9 to zone_stride");
    for (int z = 0; z < nz; ++z)
      if (t->zone_id[k * S + z] > 63) return fail(e, SPX_ERR_ARG, "NRT tall nodes: node " + std::to_string(t->node_idx[k]) + " carries a NUMA id above 63");
    if (nz > SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA && ln_node < 0) ln_node = t->node_idx[k], ln_zones = nz;
  }
  int rc;
  if ((rc = upload(e, e->d_nrtt_idx, t->node_idx, static_cast<size_t>(T) * 4)) || (rc = upload(e, e->d_nrtt_flags, t->flags, static_cast<size_t>(T))) ||
      (rc = upload(e, e->d_nrtt_max, t->max_numa, static_cast<size_t>(T) * 4)) || (rc = upload(e, e->d_nrtt_np, t->node_present, static_cast<size_t>(T))) ||
      (rc = upload(e, e->d_nrtt_nz, t->n_zones, static_cast<size_t>(T))) || (rc = upload_transposed(e, e->d_nrtt_zid, t->zone_id, T, S)) ||
      (rc = upload_transposed(e, e->d_nrtt_zp, t->zone_present, T, S)) || (rc = upload_transposed(e, e->d_nrtt_cost, t->zone_cost, T, S * S)) ||
      (rc = upload_transposed(e, e->d_nrtt_minavg, t->min_avg_dist, T, S)))
    return rc;
  if (R) {
    if ((rc = upload_transposed(e, e->d_nrtt_avail, t->zone_avail, T, S * R))) return rc;
  } else if ((rc = ensure(e, e->d_nrtt_avail, 16))) {
    return rc;
  }
  // the dense table's n_zones column holds 0 for these nodes already (spx_upload_nrt_nodes wrote it so)
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->nrt_tall_stride = static_cast<int32_t>(S);
  e->nrt_tall_ln_node = ln_node, e->nrt_tall_ln_zones = ln_zones;
  e->nrt_tall_last = 0;
  e->nrt_tall_ok = true;
  e->evaluated = 0;
  e->best_valid = false;
  return SPX_OK;
}

// The wide form replaces the dense NRT state: its tables and every cache keyed on them (the fused walk's items, the packed Score's
// table, the windows' sorted quantities, the long rows) are invalidated; spx_upload_nrt_slots does the same the other way round.
int spx_upload_nrt_slots_wide(spx_engine* e, const spx_nrt_slots* t) {
  if (!e || !t) return SPX_ERR_ARG;
  if (t->n_res < 0 || t->n_res > SPX_NRT_MAX_RES_WIDE) return fail(e, SPX_ERR_ARG, "NRT: more resource slots than the wide tables hold (32)");
  if (t->n_res && (!t->slot_flags || !t->slot_weight)) return fail(e, SPX_ERR_ARG, "NULL column in table");
  SPX_HIP(e, hipSetDevice(e->device));
  e->nrt_slots = e->nrt_nodes = e->nrt_pods = false;
  ++e->nrt_items_gen;
  e->nrt_fz_key = spx_engine::FzKey{};
  e->nrt_pk_tab_built = e->nrt_wsort_built = false;
  e->h_nrt_long_rows.clear();
  e->nrt_long_ok = true;
  e->nrt_long_last = 0;
  e->h_nrt_tall_nodes.clear();
  e->nrt_tall_ok = true;
  e->nrt_tall_last = 0;
  e->nrt_wide = true;
  e->nrtw_slots = e->nrtw_nodes = e->nrtw_pods = false;
  const size_t R = static_cast<size_t>(t->n_res);
  int rc;
  if ((rc = upload(e, e->d_nrtw_sflags, t->slot_flags, R)) || (rc = upload(e, e->d_nrtw_sweight, t->slot_weight, R * 8))) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->nrtw_n_res = t->n_res;
  e->nrtw_slots = true;
  return SPX_OK;
}

int spx_upload_nrt_nodes_wide(spx_engine* e, const spx_nrt_nodes_wide* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (!e->nrt_wide || !e->nrtw_slots || t->n_res != e->nrtw_n_res) return fail(e, SPX_ERR_STATE, "NRT: upload the wide slot table first (n_res mismatch)");
  int rc = set_nodes(e, t->n_nodes);
  if (rc) return rc;
  e->nrtw_nodes = false;
  const int64_t n = t->n_nodes, R = t->n_res;
  constexpr int64_t Zm = SPX_NRT_MAX_ZONES;
  if (!t->flags || !t->max_numa || !t->n_zones || !t->zone_id || !t->zone_present || !t->zone_cost || !t->min_avg_dist || !t->node_present ||
      (!t->zone_avail && R))
    return fail(e, SPX_ERR_ARG, "NULL column in table");
  const size_t m = static_cast<size_t>(n);
  for (size_t i = 0; i < m; ++i) {  // the kernel indexes its subset table by the zone count and shifts by the NUMA ids
    if (t->n_zones[i] > Zm) return fail(e, SPX_ERR_ARG, "NRT wide nodes: more than 8 NUMA zones on a node");
    for (int64_t z = 0; z < Zm; ++z)
      if (t->zone_id[i * Zm + z] > 63) return fail(e, SPX_ERR_ARG, "NRT wide nodes: a NUMA id above 63");
  }
  if ((rc = upload(e, e->d_nrtw_flags, t->flags, m)) || (rc = upload(e, e->d_nrtw_max_numa, t->max_numa, m * 4)) || (rc = upload(e, e->d_nrtw_nz, t->n_zones, m)) ||
      (rc = upload(e, e->d_nrtw_np, t->node_present, m * 4)))
    return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  if ((rc = upload_transposed(e, e->d_nrtw_zid, t->zone_id, n, Zm)) || (rc = upload_transposed(e, e->d_nrtw_zp, t->zone_present, n, Zm)) ||
      (rc = upload_transposed(e, e->d_nrtw_cost, t->zone_cost, n, Zm * Zm)) || (rc = upload_transposed(e, e->d_nrtw_minavg, t->min_avg_dist, n, Zm)))
    return rc;
  if (R && (rc = upload_transposed(e, e->d_nrtw_avail, t->zone_avail, n, Zm * R))) return rc;
  if (!R && (rc = ensure(e, e->d_nrtw_avail, 8))) return rc;
  e->nrtw_nodes = true;
  return SPX_OK;
}

int spx_upload_nrt_pods_wide(spx_engine* e, const spx_nrt_pods_wide* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (!e->nrt_wide || !e->nrtw_slots || t->n_res != e->nrtw_n_res) return fail(e, SPX_ERR_STATE, "NRT: upload the wide slot table first (n_res mismatch)");
  if (!t->qos || !t->non_native || !t->req_ptr || !t->ctr_ptr || !t->ent_ptr) return fail(e, SPX_ERR_ARG, "NULL column in table");
  int rc = set_pods(e, t->n_pods);
  if (rc) return rc;
  e->nrtw_pods = false;
  const size_t P = static_cast<size_t>(t->n_pods);
  if (t->req_ptr[0] != 0 || t->ctr_ptr[0] != 0 || t->ent_ptr[0] != 0) return fail(e, SPX_ERR_ARG, "NRT wide pods: req_ptr / ctr_ptr / ent_ptr must start at 0");
  for (size_t i = 0; i < P; ++i) {
    const int32_t nc = t->ctr_ptr[i + 1] - t->ctr_ptr[i];
    if (nc < 0 || t->req_ptr[i + 1] < t->req_ptr[i]) return fail(e, SPX_ERR_ARG, "NRT wide pods: req_ptr / ctr_ptr must not decrease");
    if (nc > SPX_NRT_WIDE_MAX_CTRS) {
      char buf[160];
      std::snprintf(buf, sizeof buf, "NRT wide pods: pod row %zu has %d containers; a wide snapshot takes up to %d per pod", i, nc, SPX_NRT_WIDE_MAX_CTRS);
      return fail(e, SPX_ERR_ARG, buf);
    }
  }
  const size_t C = static_cast<size_t>(t->ctr_ptr[P]), Er = static_cast<size_t>(t->req_ptr[P]);
  for (size_t c = 0; c < C; ++c)
    if (t->ent_ptr[c + 1] < t->ent_ptr[c]) return fail(e, SPX_ERR_ARG, "NRT wide pods: ent_ptr must not decrease");
  const size_t Ec = static_cast<size_t>(t->ent_ptr[C]);
  // slots in range and every list ascending: the kernel indexes the slot columns by them and stops a search at the first larger slot
  auto lists_ok = [&](const int32_t* ptr, size_t n_lists, const uint8_t* slot) {
    for (size_t l = 0; l < n_lists; ++l)
      for (int32_t k = ptr[l]; k < ptr[l + 1]; ++k)
        if (slot[k] >= t->n_res || (k > ptr[l] && slot[k] <= slot[k - 1])) return false;
    return true;
  };
  if ((Er && (!t->req_slot || !t->req_qty)) || (Ec && (!t->ent_slot || !t->ent_qty)) || (C && !t->ctr_kind)) return fail(e, SPX_ERR_ARG, "NULL column in table");
  if (!lists_ok(t->req_ptr, P, t->req_slot) || !lists_ok(t->ent_ptr, C, t->ent_slot))
    return fail(e, SPX_ERR_ARG, "NRT wide pods: every list must name slots below n_res in ascending order");
  if ((rc = upload(e, e->d_nrtw_qos, t->qos, P)) || (rc = upload(e, e->d_nrtw_nn, t->non_native, P)) ||
      (rc = upload(e, e->d_nrtw_rptr, t->req_ptr, (P + 1) * 4)) || (rc = upload(e, e->d_nrtw_rslot, t->req_slot, Er)) ||
      (rc = upload(e, e->d_nrtw_rqty, t->req_qty, Er * 8)) || (rc = upload(e, e->d_nrtw_cptr, t->ctr_ptr, (P + 1) * 4)) ||
      (rc = upload(e, e->d_nrtw_ckind, t->ctr_kind, C)) || (rc = upload(e, e->d_nrtw_eptr, t->ent_ptr, (C + 1) * 4)) ||
      (rc = upload(e, e->d_nrtw_eslot, t->ent_slot, Ec)) || (rc = upload(e, e->d_nrtw_eqty, t->ent_qty, Ec * 8)))
    return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->nrtw_pods = true;
  return SPX_OK;
}

int spx_upload_net_nodes(spx_engine* e, const spx_net_nodes_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  int rc = set_nodes(e, t->n_nodes);
  if (rc) return rc;
  if (!t->region || !t->zone) return fail(e, SPX_ERR_ARG, "NULL column in table");
  const int64_t n = t->n_nodes;
  // topology classes: nodes with identical (region, zone) labels are interchangeable for every pair that is
  // not hosted on them
  std::vector<int32_t> cls(static_cast<size_t>(n)), cr, cz;
  {
    std::vector<std::pair<int64_t, int32_t>> seen;  // sorted (packed label pair -> class)
    std::vector<int64_t> keys(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) keys[i] = (static_cast<int64_t>(t->region[i]) << 32) ^ static_cast<uint32_t>(t->zone[i]);
    std::vector<int64_t> uniq(keys);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    for (int64_t i = 0; i < n; ++i)
      cls[i] = static_cast<int32_t>(std::lower_bound(uniq.begin(), uniq.end(), keys[i]) - uniq.begin());
    cr.resize(uniq.size());
    cz.resize(uniq.size());
    for (int64_t i = 0; i < n; ++i) {
      cr[cls[i]] = t->region[i];
      cz[cls[i]] = t->zone[i];
    }
  }
  int32_t n_classes = static_cast<int32_t>(cr.size());
  if (spx::net_lds_bytes(n_classes, n) > spx::kNetLdsBudget) n_classes = 0;  // too many label pairs for LDS (64 KB with a single-row launch's staged pairs): exact path only
  e->net_n_classes = n_classes;
  if ((rc = upload(e, e->d_net_region, t->region, static_cast<size_t>(n) * 4))) return rc;
  if ((rc = upload(e, e->d_net_zone, t->zone, static_cast<size_t>(n) * 4))) return rc;
  if ((rc = upload(e, e->d_net_class, cls.data(), static_cast<size_t>(n) * 4))) return rc;
  {
    std::vector<uint16_t> c16(static_cast<size_t>(spx::round_up(n, 16)), 0);  // (k_net_cls reads groups of 16)
    std::vector<int32_t> size(cr.size() ? cr.size() : 1, 0);
    e->net_class16 = cr.size() <= 65535;
    for (int64_t i = 0; i < n; ++i) {
      c16[static_cast<size_t>(i)] = static_cast<uint16_t>(cls[static_cast<size_t>(i)]);
      ++size[static_cast<size_t>(cls[static_cast<size_t>(i)])];
    }
    if ((rc = upload(e, e->d_net_class16, c16.data(), c16.size() * 2))) return rc;
    if ((rc = upload(e, e->d_net_cls_size, size.data(), size.size() * 4))) return rc;
    SPX_HIP(e, hipStreamSynchronize(e->stream));
  }
  if ((rc = upload(e, e->d_net_cls_region, cr.data(), cr.size() * 4))) return rc;
  if ((rc = upload(e, e->d_net_cls_zone, cz.data(), cz.size() * 4))) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->net_nodes = true;
  return SPX_OK;
}

int spx_upload_net_topo(spx_engine* e, const spx_net_topo_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  return upload_net_costs<int32_t>(e, t->n_regions, t->n_zones, t->region_cost, t->zone_cost);
}

int spx_upload_net_topo_wide(spx_engine* e, const spx_net_topo_wide* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  return upload_net_costs<int64_t>(e, t->n_regions, t->n_zones, t->region_cost, t->zone_cost);
}

int spx_upload_net_pods(spx_engine* e, const spx_net_pods_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  int rc = set_pods(e, t->n_pods);
  if (rc) return rc;
  if (t->n_keys <= 0 || !t->pair_ptr) return fail(e, SPX_ERR_ARG, "net pods: key table missing");
  const size_t pairs = static_cast<size_t>(t->pair_ptr[t->n_keys]);
  e->net_max_pairs = 0;
  for (int32_t k = 0; k < t->n_keys; ++k) e->net_max_pairs = std::max<int64_t>(e->net_max_pairs, t->pair_ptr[k + 1] - t->pair_ptr[k]);
  e->h_pair_ptr.assign(t->pair_ptr, t->pair_ptr + t->n_keys + 1);
  e->h_key_flag.assign(t->key_score_equally, t->key_score_equally + t->n_keys);
  e->net_n_keys = t->n_keys;
  e->net_commit = false;  // the commit effects refer to the previous key numbering
  if ((rc = upload(e, e->d_net_pod_key, t->pod_key, static_cast<size_t>(t->n_pods) * 4))) return rc;
  if ((rc = upload(e, e->d_net_key_flag, t->key_score_equally, static_cast<size_t>(t->n_keys)))) return rc;
  if ((rc = upload(e, e->d_net_pair_ptr, t->pair_ptr, static_cast<size_t>(t->n_keys + 1) * 4))) return rc;
  if ((rc = upload(e, e->d_net_pair_node, pairs ? static_cast<const void*>(t->pair_node) : static_cast<const void*>(&rc), pairs * 4))) return rc;
  if ((rc = upload(e, e->d_net_pair_max, pairs ? static_cast<const void*>(t->pair_max_cost) : static_cast<const void*>(&rc), pairs * 8))) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->net_pods = true;
  return SPX_OK;
}

int spx_upload_sort_keys(spx_engine* e, const spx_sort_keys_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (t->n_pods <= 0 || t->n_pods >= (int64_t{1} << 31)) return fail(e, SPX_ERR_ARG, "sort keys: n_pods must be in [1, 2^31)");
  const size_t p = static_cast<size_t>(t->n_pods);
  int rc;
  if ((rc = upload(e, e->d_sort_prio, t->priority, p * 4))) return rc;
  if ((rc = upload(e, e->d_sort_ts, t->queue_ts, p * 8))) return rc;
  if ((rc = upload(e, e->d_sort_group, t->appgroup, p * 4))) return rc;
  if ((rc = upload(e, e->d_sort_topo, t->topo_order, p * 4))) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->sort_n = t->n_pods;
  return SPX_OK;
}

int spx_sort_keys(spx_engine* e, int32_t* perm_out) {
  if (!e || !perm_out) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (e->sort_n <= 0) return fail(e, SPX_ERR_STATE, "TopologicalSort: spx_upload_sort_keys not called");
  int rc;
  if ((rc = ensure(e, e->d_sort_scratch, spx::sort_scratch_bytes(e->sort_n)))) return rc;
  if (!e->h_sort_hist) SPX_HIP(e, hipHostMalloc(reinterpret_cast<void**>(&e->h_sort_hist), 16 * 256 * sizeof(unsigned), hipHostMallocDefault));
  spx::SortArgs a{};
  a.n = e->sort_n;
  a.priority = static_cast<const int32_t*>(e->d_sort_prio.p);
  a.queue_ts = static_cast<const int64_t*>(e->d_sort_ts.p);
  a.appgroup = static_cast<const int32_t*>(e->d_sort_group.p);
  a.topo_order = static_cast<const int32_t*>(e->d_sort_topo.p);
  SPX_HIP(e, hipEventRecord(e->ev0, e->stream));
  hipError_t st = hipSuccess;
  const int32_t* perm = spx::launch_sort_keys(a, e->d_sort_scratch.p, e->h_sort_hist, e->stream, &st);
  if (st != hipSuccess || !perm) return fail(e, SPX_ERR_HIP, std::string("spx_sort_keys: ") + hipGetErrorString(st));
  SPX_HIP(e, hipEventRecord(e->ev1, e->stream));
  e->timed = true;
  SPX_HIP(e, hipMemcpyAsync(perm_out, perm, static_cast<size_t>(e->sort_n) * 4, hipMemcpyDeviceToHost, e->stream));
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

// NodeMetadata's / PodState's raw column: one int64 per node, whole (no row delta: the column is n_nodes x 8 bytes)
static int upload_node_column(spx_engine* e, const spx_node_column_soa* t, int plugin, DevBuf& col, bool& ready) {
  SPX_HIP(e, hipSetDevice(e->device));
  if (!t->raw) return fail(e, SPX_ERR_ARG, "NULL column in table");
  if (plugin == SPX_PLUGIN_PODSTATE)
    for (int64_t i = 0; i < t->n_nodes; ++i)
      if (t->raw[i] >= (int64_t{1} << 31) || t->raw[i] <= -(int64_t{1} << 31))
        return fail(e, SPX_ERR_ARG, "PodState: a node's terminating minus nominated pod count must lie inside (-2^31, 2^31)");
  int rc = set_nodes(e, t->n_nodes);
  if (rc) return rc;
  ready = false;
  if ((rc = upload(e, col, t->raw, static_cast<size_t>(t->n_nodes) * sizeof(int64_t)))) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  ready = true;
  e->evaluated &= ~(1u << plugin);
  e->best_valid = false;
  return SPX_OK;
}

int spx_upload_nodemeta_nodes(spx_engine* e, const spx_node_column_soa* t, int64_t now_unused) {
  if (!e || !t) return SPX_ERR_ARG;
  if (now_unused != 0) return fail(e, SPX_ERR_ARG, "NodeMetadata: now_unused is reserved and must be 0 (spx_flatten_nodemeta takes the time)");
  return upload_node_column(e, t, SPX_PLUGIN_NODEMETA, e->d_nm_raw, e->nm_nodes);
}

int spx_upload_podstate_nodes(spx_engine* e, const spx_node_column_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  return upload_node_column(e, t, SPX_PLUGIN_PODSTATE, e->d_ps_raw, e->ps_nodes);
}

int spx_upload_qos_sort_keys(spx_engine* e, const spx_qos_sort_keys_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (t->n_pods <= 0 || t->n_pods >= (int64_t{1} << 31)) return fail(e, SPX_ERR_ARG, "QOSSort keys: n_pods must be in [1, 2^31)");
  if (!t->priority || !t->qos || !t->queue_ts) return fail(e, SPX_ERR_ARG, "NULL column in table");
  const size_t p = static_cast<size_t>(t->n_pods);
  for (size_t i = 0; i < p; ++i)
    if (t->qos[i] < SPX_QOSSORT_BEST_EFFORT || t->qos[i] > SPX_QOSSORT_GUARANTEED)
      return fail(e, SPX_ERR_ARG, "QOSSort keys: qos must be 1 (BestEffort), 2 (Burstable) or 3 (Guaranteed)");
  int rc;
  e->qos_n = 0;
  if ((rc = upload(e, e->d_qos_prio, t->priority, p * 4))) return rc;
  if ((rc = upload(e, e->d_qos_cls, t->qos, p))) return rc;
  if ((rc = upload(e, e->d_qos_ts, t->queue_ts, p * 8))) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->qos_n = t->n_pods;
  return SPX_OK;
}

int spx_qos_sort(spx_engine* e, int32_t* perm_out) {
  if (!e || !perm_out) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if (e->qos_n <= 0) return fail(e, SPX_ERR_STATE, "QOSSort: spx_upload_qos_sort_keys not called");
  const size_t p = static_cast<size_t>(e->qos_n);
  int rc;
  if ((rc = ensure(e, e->d_qos_scratch, spx::sort_scratch_bytes(e->qos_n))) || (rc = ensure(e, e->d_qos_key, p * 4)) || (rc = ensure(e, e->d_qos_none, p * 4)) ||
      (rc = ensure(e, e->d_qos_zero, p * 4)) || (rc = ensure(e, e->d_qos_rank, p * 8)))
    return rc;
  if (!e->h_sort_hist) SPX_HIP(e, hipHostMalloc(reinterpret_cast<void**>(&e->h_sort_hist), 16 * 256 * sizeof(unsigned), hipHostMallocDefault));
  // Less orders by (priority descending, class descending, timestamp ascending).  kernels_sort.hip's passes order int32 descending then
  // int64 ascending, stably from the row order, so: sort by (class, timestamp); the rank in that order stands for both keys and
  // is unique; sort by (priority, rank).  No pod belongs to an AppGroup, so that sort's second stage leaves the order as it is.
  spx::SortArgs a{};
  a.n = e->qos_n;
  a.priority = static_cast<const int32_t*>(e->d_qos_key.p);
  a.queue_ts = static_cast<const int64_t*>(e->d_qos_ts.p);
  a.appgroup = static_cast<const int32_t*>(e->d_qos_none.p);
  a.topo_order = static_cast<const int32_t*>(e->d_qos_zero.p);
  SPX_HIP(e, hipEventRecord(e->ev0, e->stream));
  spx::launch_qos_class_keys(static_cast<const uint8_t*>(e->d_qos_cls.p), e->qos_n, static_cast<int32_t*>(e->d_qos_key.p), static_cast<int32_t*>(e->d_qos_none.p),
                             static_cast<int32_t*>(e->d_qos_zero.p), e->stream);
  hipError_t st = hipSuccess;
  const int32_t* perm = spx::launch_sort_keys(a, e->d_qos_scratch.p, e->h_sort_hist, e->stream, &st);
  if (st != hipSuccess || !perm) return fail(e, SPX_ERR_HIP, std::string("spx_qos_sort: ") + hipGetErrorString(st));
  spx::launch_qos_rank_keys(perm, e->qos_n, static_cast<int64_t*>(e->d_qos_rank.p), e->stream);
  a.priority = static_cast<const int32_t*>(e->d_qos_prio.p);
  a.queue_ts = static_cast<const int64_t*>(e->d_qos_rank.p);
  perm = spx::launch_sort_keys(a, e->d_qos_scratch.p, e->h_sort_hist, e->stream, &st);
  if (st != hipSuccess || !perm) return fail(e, SPX_ERR_HIP, std::string("spx_qos_sort: ") + hipGetErrorString(st));
  SPX_HIP(e, hipEventRecord(e->ev1, e->stream));
  e->timed = true;
  SPX_HIP(e, hipMemcpyAsync(perm_out, perm, p * 4, hipMemcpyDeviceToHost, e->stream));
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

int spx_upload_quota(spx_engine* e, const spx_quota_soa* t) {
  if (!e || !t) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  int rc = set_pods(e, t->n_pods);
  if (rc) return rc;
  if (t->n_namespaces < 0 || !t->nom_ptr) return fail(e, SPX_ERR_ARG, "quota: namespace tables missing");
  const size_t P = static_cast<size_t>(t->n_pods), NS = static_cast<size_t>(t->n_namespaces), S = SPX_QUOTA_SLOTS;
  const size_t nn = static_cast<size_t>(t->nom_ptr[t->n_namespaces]);
  // a column may be NULL only when it has no entries (no namespaces / no nominated pods); upload() rejects the rest.  Every exit
  // after the first asynchronous copy waits for the stream: the host columns are only borrowed for the call.
  const int64_t dummy[SPX_QUOTA_SLOTS] = {0};
  auto col = [&](const void* p) { return p ? p : static_cast<const void*>(dummy); };
  struct Drain {
    spx_engine* e;
    ~Drain() { (void)hipStreamSynchronize(e->stream); }
  } drain{e};
  if ((NS > 0 && (!t->has_quota || !t->used || !t->max || !t->max_present || !t->other_nominated || !t->other_nominated_present)) ||
      (nn > 0 && (!t->nom_priority || !t->nom_pending_index || !t->nom_req || !t->nom_req_present)))
    return fail(e, SPX_ERR_ARG, "quota: NULL column in a non-empty table");
  if ((rc = upload(e, e->d_q_pod_ns, t->pod_ns, P * 4))) return rc;
  if ((rc = upload(e, e->d_q_pod_prio, t->pod_priority, P * 4))) return rc;
  if ((rc = upload(e, e->d_q_pod_req, t->pod_req, P * S * 8))) return rc;
  if ((rc = upload(e, e->d_q_pod_reqp, t->pod_req_present, P))) return rc;
  if ((rc = upload(e, e->d_q_has, col(t->has_quota), NS))) return rc;
  if ((rc = upload(e, e->d_q_used, col(t->used), NS * S * 8))) return rc;
  if (NS > 0 && !t->used_present) return fail(e, SPX_ERR_ARG, "quota: NULL column in a non-empty table");
  if ((rc = upload(e, e->d_q_usedp, col(t->used_present), NS))) return rc;
  e->pre_marks_valid = e->pre_valid = false;  // the preemption dry run read the old tables
  e->q_has_min = t->min && t->min_present;
  if (e->q_has_min) {
    if ((rc = upload(e, e->d_q_min, t->min, NS * S * 8))) return rc;
    if ((rc = upload(e, e->d_q_minp, t->min_present, NS))) return rc;
  }
  if ((rc = upload(e, e->d_q_max, col(t->max), NS * S * 8))) return rc;
  if ((rc = upload(e, e->d_q_maxp, col(t->max_present), NS))) return rc;
  if ((rc = upload(e, e->d_q_other, col(t->other_nominated), NS * S * 8))) return rc;
  if ((rc = upload(e, e->d_q_otherp, col(t->other_nominated_present), NS))) return rc;
  if ((rc = upload(e, e->d_q_nom_ptr, t->nom_ptr, (NS + 1) * 4))) return rc;
  if ((rc = upload(e, e->d_q_nom_prio, col(t->nom_priority), nn * 4))) return rc;
  if ((rc = upload(e, e->d_q_nom_idx, col(t->nom_pending_index), nn * 8))) return rc;
  if ((rc = upload(e, e->d_q_nom_req, col(t->nom_req), nn * S * 8))) return rc;
  if ((rc = upload(e, e->d_q_nom_reqp, col(t->nom_req_present), nn))) return rc;
  if (!t->agg_used || !t->agg_min || !t->agg_used_present || !t->agg_min_present) return fail(e, SPX_ERR_ARG, "quota: aggregate vectors missing");
  std::memcpy(e->q_agg_used, t->agg_used, sizeof e->q_agg_used);
  std::memcpy(e->q_agg_min, t->agg_min, sizeof e->q_agg_min);
  e->q_agg_used_present = *t->agg_used_present;
  e->q_agg_min_present = *t->agg_min_present;
  e->q_n_namespaces = t->n_namespaces;
  e->q_n_nominated = nn;
  {
    int64_t agg[SPX_QUOTA_SLOTS + 1];
    std::memcpy(agg, t->agg_used, sizeof e->q_agg_used);
    agg[SPX_QUOTA_SLOTS] = *t->agg_used_present;
    if ((rc = upload(e, e->d_q_agg, agg, sizeof agg))) return rc;
    SPX_HIP(e, hipStreamSynchronize(e->stream));  // agg is a stack array
  }
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->quota = true;
  return SPX_OK;
}

int spx_fetch_prefilter(spx_engine* e, int plugin, int64_t row_begin, int64_t row_end, uint8_t* out) {
  if (!e || !out) return SPX_ERR_ARG;
  if (plugin == SPX_PLUGIN_COSCHED) {
    if (!e->cosched || !e->cs_gate_valid || !(e->evaluated & (1u << SPX_PLUGIN_COSCHED)))
      return fail(e, SPX_ERR_STATE, "Coscheduling's PreFilter has not been evaluated since its last upload");
    if (row_begin < 0 || row_end > e->n_pods || row_begin > row_end) return fail(e, SPX_ERR_ARG, "row range out of bounds");
    if (row_end > row_begin && (row_begin < e->cs_row_begin || row_end > e->cs_row_end))
      return fail(e, SPX_ERR_STATE, "rows requested have not been evaluated for this plugin (spx_eval covers [" + std::to_string(e->cs_row_begin) + ", " +
                                        std::to_string(e->cs_row_end) + "))");
    SPX_HIP(e, hipSetDevice(e->device));
    SPX_HIP(e, hipStreamSynchronize(e->stream));
    SPX_HIP(e, hipMemcpy(out, static_cast<const uint8_t*>(e->d_cs_status.p) + row_begin, static_cast<size_t>(row_end - row_begin), hipMemcpyDeviceToHost));
    return SPX_OK;
  }
  if (plugin != SPX_PLUGIN_CAPACITY || !(e->evaluated & (1u << SPX_PLUGIN_CAPACITY)))
    return fail(e, SPX_ERR_STATE, "CapacityScheduling.PreFilter has not been evaluated");
  if (row_begin < 0 || row_end > e->n_pods || row_begin > row_end) return fail(e, SPX_ERR_ARG, "row range out of bounds");
  if (int rc = rows_evaluated(e, SPX_PLUGIN_CAPACITY, row_begin, row_end)) return rc;
  SPX_HIP(e, hipSetDevice(e->device));
  SPX_HIP(e, hipMemcpy(out, static_cast<const uint8_t*>(e->d_q_status.p) + row_begin, static_cast<size_t>(row_end - row_begin),
                       hipMemcpyDeviceToHost));
  return SPX_OK;
}

int spx_upload_feasible_mask(spx_engine* e, const uint8_t* mask, int64_t n_pods, int64_t n_nodes) {
  if (!e) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  ++e->ext_gen;
  if (!mask) {  // clear
    e->ext_mask = false;
    return SPX_OK;
  }
  int rc = set_nodes(e, n_nodes);
  if (rc) return rc;
  if ((rc = set_pods(e, n_pods))) return rc;
  // stored like a Filter plugin's status table: 0 = passed, so that every consumer treats filters uniformly
  std::vector<uint8_t> st(static_cast<size_t>(n_pods) * static_cast<size_t>(e->row_stride), 1);
  for (int64_t p = 0; p < n_pods; ++p)
    for (int64_t n = 0; n < n_nodes; ++n) st[static_cast<size_t>(p * e->row_stride + n)] = mask[p * n_nodes + n] ? 0 : 1;
  if ((rc = upload(e, e->d_ext_status, st.data(), st.size()))) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->ext_mask = true;
  return SPX_OK;
}
}  // extern "C"
