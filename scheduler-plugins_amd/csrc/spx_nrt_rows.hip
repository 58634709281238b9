// spx_nrt_rows.hip — NodeResourceTopologyMatch beside the dense sweep: the launches of the long rows (kernels_nrt_long.hip), the tall
// nodes (kernels_nrt_tall.hip) and the wide tables (kernels_nrt_wide.hip), with what they need in place first (nrt_tall_ready,
// ensure_nrt_creq).  spx_eval and spx_fetch_raw (spx_engine.hip) call them after their dense launch.  Declared in spx_engine.h; no
// kernel and no entry point lives here.
#include "spx_engine.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace {

// combin.Combinations(n, k) for n = 9 .. 16 as 16-bit masks over list positions, size-major then lexicographic (the 16-bit sibling
// of nrt_combinations; 131 064 masks, built once on the host and uploaded: the 64 KB constant segment does not hold them)
struct NrtTallCombos {
  std::vector<uint16_t> mask;
  uint32_t start[8][SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA + 1];
};
NrtTallCombos make_nrt_tall_combos() {
  NrtTallCombos t;
  for (int n = 9; n <= SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA; ++n) {
    for (int k = 1; k <= SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA; ++k) {
      t.start[n - 9][k - 1] = static_cast<uint32_t>(t.mask.size());
      if (k > n) continue;
      int c[SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA];
      for (int i = 0; i < k; ++i) c[i] = i;
      while (true) {
        unsigned m = 0;
        for (int i = 0; i < k; ++i) m |= 1u << c[i];
        t.mask.push_back(static_cast<uint16_t>(m));
        int i = k - 1;
        while (i >= 0 && c[i] == n - k + i) --i;
        if (i < 0) break;
        ++c[i];
        for (int j = i + 1; j < k; ++j) c[j] = c[j - 1] + 1;
      }
    }
    t.start[n - 9][SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA] = static_cast<uint32_t>(t.mask.size());
  }
  return t;
}

}  // namespace

namespace spx_eng {

// the long rows of [row_begin, row_end) (kernels_nrt_long.hip) after the dense sweep `na` wrote their cells as those of an empty pod
// (no containers, no request): their status and score rows are overwritten (or, with na.out_raw, the raw row).  Inside the sequential commit loop
// (row_indirect) the launch reads the row from the device and leaves at once when it is not long.  No launch without long rows.
int launch_nrt_long_rows(spx_engine* e, const spx::NrtArgs& na, int64_t row_begin, int64_t row_end) {
  e->nrt_long_last = 0;
  const std::vector<int32_t>& rows = e->h_nrt_long_rows;
  if (rows.empty()) return SPX_OK;
  if (!e->nrt_long_ok) return fail(e, SPX_ERR_STATE, "NRT: the pod batch has pods with more than 8 containers: call spx_upload_nrt_long_pods after spx_upload_nrt_pods");
  const int64_t k0 = std::lower_bound(rows.begin(), rows.end(), row_begin) - rows.begin();
  const int64_t k1 = std::lower_bound(rows.begin(), rows.end(), row_end) - rows.begin();
  if (k1 <= k0 && !e->row_indirect) return SPX_OK;
  spx::NrtLongArgs l{};
  l.n_nodes = na.n_nodes;
  l.n_pods = na.n_pods;
  l.row_stride = na.row_stride;
  l.n_res = na.n_res;
  l.strategy = na.strategy;
  std::memcpy(l.slot_flags, na.slot_flags, sizeof l.slot_flags);
  std::memcpy(l.slot_weight, na.slot_weight, sizeof l.slot_weight);
  l.flags = na.flags, l.max_numa = na.max_numa, l.n_zones = na.n_zones, l.zone_id = na.zone_id, l.zone_present = na.zone_present;
  l.zone_avail = na.zone_avail, l.zone_cost = na.zone_cost, l.min_avg = na.min_avg, l.node_present = na.node_present;
  l.qos = na.qos, l.non_native = na.non_native, l.pod_present = na.pod_present, l.pod_req = na.pod_req;
  l.pod_row = static_cast<const int32_t*>(e->d_nrtl_row.p);
  l.ctr_ptr = static_cast<const int32_t*>(e->d_nrtl_ptr.p);
  l.ctr_kind = static_cast<const uint8_t*>(e->d_nrtl_kind.p);
  l.ctr_present = static_cast<const uint8_t*>(e->d_nrtl_pres.p);
  l.ctr_req = static_cast<const int64_t*>(e->d_nrtl_req.p);
  l.long_begin = k0;
  l.long_end = k1;
  if (e->row_indirect) {
    l.row_ptr = e->row_indirect;
    l.long_of_row = static_cast<const int32_t*>(e->d_nrtl_map.p);
  }
  l.out_status = na.out_status;
  l.out_score = na.out_score;
  l.out_raw = na.out_raw;
  spx::launch_nrt_long(l, e->stream);
  SPX_HIP(e, hipGetLastError());
  e->nrt_long_last = k1 - k0;
  return SPX_OK;
}

// what an NRT evaluation of an engine with tall nodes needs before its first launch, from host state alone: the side table, and with
// LeastNUMANodes no tall node above that strategy's zone limit.  spx_eval and spx_fetch_raw ask before they write anything.
int nrt_tall_ready(const spx_engine* e) {
  if (e->h_nrt_tall_nodes.empty()) return SPX_OK;
  if (!e->nrt_tall_ok)
    return fail(e, SPX_ERR_STATE, "NRT: the node table has nodes with more than 8 NUMA zones: call spx_upload_nrt_tall_nodes after spx_upload_nrt_nodes");
  if (e->nrt_params.strategy == SPX_NRT_LEAST_NUMA_NODES && e->nrt_tall_ln_node >= 0) {
    char buf[200];
    std::snprintf(buf, sizeof buf, "NRT: LeastNUMANodes takes nodes of up to %d NUMA zones; node %d lists %d", SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA,
                  e->nrt_tall_ln_node, e->nrt_tall_ln_zones);
    return fail(e, SPX_ERR_STATE, buf);
  }
  return SPX_OK;
}

// the tall nodes' columns of rows [row_begin, row_end) (kernels_nrt_tall.hip) after the dense sweep `na` and the long rows wrote them as
// those of a node without an NRT object: status and score are overwritten (or, with na.out_raw, the raw row's entries).  It runs for
// every row of the range — class copies, short and long rows — in reference arithmetic, whatever form the dense sweep took.  No launch
// and no allocation without tall nodes.
int launch_nrt_tall_rows(spx_engine* e, const spx::NrtArgs& na, int64_t row_begin, int64_t row_end) {
  e->nrt_tall_last = 0;
  const std::vector<int32_t>& tall = e->h_nrt_tall_nodes;
  if (tall.empty()) return SPX_OK;
  if (e->row_indirect) return fail(e, SPX_ERR_STATE, "NRT: the sequential commit loop does not take nodes with more than 8 NUMA zones");
  int rc;
  if ((rc = nrt_tall_ready(e))) return rc;  // (the callers checked before their first launch; a direct call must not get past it either)
  if (row_end <= row_begin) return SPX_OK;
  spx::NrtTallArgs t{};
  t.n_nodes = na.n_nodes, t.n_pods = na.n_pods, t.row_stride = na.row_stride, t.n_res = na.n_res, t.strategy = na.strategy;
  std::memcpy(t.slot_flags, na.slot_flags, sizeof t.slot_flags);
  std::memcpy(t.slot_weight, na.slot_weight, sizeof t.slot_weight);
  t.n_tall = static_cast<int32_t>(tall.size());
  t.zone_stride = e->nrt_tall_stride;
  t.node_idx = static_cast<const int32_t*>(e->d_nrtt_idx.p);
  t.flags = static_cast<const uint8_t*>(e->d_nrtt_flags.p);
  t.max_numa = static_cast<const int32_t*>(e->d_nrtt_max.p);
  t.node_present = static_cast<const uint8_t*>(e->d_nrtt_np.p);
  t.n_zones = static_cast<const uint8_t*>(e->d_nrtt_nz.p);
  t.zone_id = static_cast<const uint8_t*>(e->d_nrtt_zid.p);
  t.zone_present = static_cast<const uint8_t*>(e->d_nrtt_zp.p);
  t.zone_avail = static_cast<const int64_t*>(e->d_nrtt_avail.p);
  t.zone_cost = static_cast<const int32_t*>(e->d_nrtt_cost.p);
  t.min_avg = static_cast<const float*>(e->d_nrtt_minavg.p);
  // the per-container request column: a batch the float64 formulation takes does not ship it, and the dense sweep that just ran did
  // not need it (ensure_nrt_creq) — this kernel reads it whatever form the dense sweep took, so it is rebuilt from the record stream here
  if ((rc = ensure_nrt_creq(e, true))) return rc;
  t.qos = na.qos, t.non_native = na.non_native, t.n_ctr = na.n_ctr, t.ctr_kind = na.ctr_kind, t.ctr_present = na.ctr_present;
  t.ctr_req = static_cast<const int64_t*>(e->d_nrt_creq.p);
  t.pod_present = na.pod_present, t.pod_req = na.pod_req;
  if (!e->h_nrt_long_rows.empty()) {
    t.long_of_row = static_cast<const int32_t*>(e->d_nrtl_map.p);
    t.long_ptr = static_cast<const int32_t*>(e->d_nrtl_ptr.p);
    t.long_kind = static_cast<const uint8_t*>(e->d_nrtl_kind.p);
    t.long_present = static_cast<const uint8_t*>(e->d_nrtl_pres.p);
    t.long_req = static_cast<const int64_t*>(e->d_nrtl_req.p);
  }
  t.row_begin = row_begin, t.row_end = row_end;
  if (na.strategy == SPX_NRT_LEAST_NUMA_NODES) {
    if (!e->nrt_tall_combos) {
      const NrtTallCombos c = make_nrt_tall_combos();
      if ((rc = upload(e, e->d_nrtt_cmask, c.mask.data(), c.mask.size() * sizeof(uint16_t))) || (rc = upload(e, e->d_nrtt_cstart, c.start, sizeof c.start))) return rc;
      SPX_HIP(e, hipStreamSynchronize(e->stream));  // (a local table)
      e->nrt_tall_combos = true;
    }
    t.combo_mask = static_cast<const uint16_t*>(e->d_nrtt_cmask.p);
    t.combo_start = static_cast<const uint32_t*>(e->d_nrtt_cstart.p);
  }
  t.n_waves = spx::nrt_tall_waves(row_end - row_begin, t.n_tall, t.zone_stride, t.n_res);
  if ((rc = ensure(e, e->d_nrtt_work, static_cast<size_t>(spx::nrt_tall_work_bytes(t.zone_stride, t.n_res, t.n_waves))))) return rc;
  t.work = static_cast<int64_t*>(e->d_nrtt_work.p);
  t.out_status = na.out_status, t.out_score = na.out_score, t.out_raw = na.out_raw;
  spx::launch_nrt_tall(t, e->stream);
  SPX_HIP(e, hipGetLastError());
  e->nrt_tall_last = static_cast<int64_t>(tall.size());
  return SPX_OK;
}

// NodeResourceTopologyMatch over the wide tables, rows [row_begin, row_end) into the status / score tables (or, with out_raw, the one
// row's raw scores).  Replaces the whole dense machinery: no pod classes, rank stream, fused walk, redo lists or long rows.
int launch_nrt_wide_rows(spx_engine* e, int64_t row_begin, int64_t row_end, int64_t* out_raw) {
  if (!(e->nrtw_slots && e->nrtw_nodes && e->nrtw_pods)) return fail(e, SPX_ERR_STATE, "NRT wide slot/node/pod tables not uploaded");
  spx::NrtWideArgs w{};
  w.n_nodes = e->n_nodes;
  w.n_pods = e->n_pods;
  w.row_stride = e->row_stride;
  w.n_res = e->nrtw_n_res;
  w.strategy = e->nrt_params.strategy;
  w.slot_flags = static_cast<const uint8_t*>(e->d_nrtw_sflags.p);
  w.slot_weight = static_cast<const int64_t*>(e->d_nrtw_sweight.p);
  w.flags = static_cast<const uint8_t*>(e->d_nrtw_flags.p);
  w.max_numa = static_cast<const int32_t*>(e->d_nrtw_max_numa.p);
  w.n_zones = static_cast<const uint8_t*>(e->d_nrtw_nz.p);
  w.zone_id = static_cast<const uint8_t*>(e->d_nrtw_zid.p);
  w.zone_present = static_cast<const uint32_t*>(e->d_nrtw_zp.p);
  w.zone_avail = static_cast<const int64_t*>(e->d_nrtw_avail.p);
  w.zone_cost = static_cast<const int32_t*>(e->d_nrtw_cost.p);
  w.min_avg = static_cast<const float*>(e->d_nrtw_minavg.p);
  w.node_present = static_cast<const uint32_t*>(e->d_nrtw_np.p);
  w.qos = static_cast<const uint8_t*>(e->d_nrtw_qos.p);
  w.non_native = static_cast<const uint8_t*>(e->d_nrtw_nn.p);
  w.req_ptr = static_cast<const int32_t*>(e->d_nrtw_rptr.p);
  w.req_slot = static_cast<const uint8_t*>(e->d_nrtw_rslot.p);
  w.req_qty = static_cast<const int64_t*>(e->d_nrtw_rqty.p);
  w.ctr_ptr = static_cast<const int32_t*>(e->d_nrtw_cptr.p);
  w.ctr_kind = static_cast<const uint8_t*>(e->d_nrtw_ckind.p);
  w.ent_ptr = static_cast<const int32_t*>(e->d_nrtw_eptr.p);
  w.ent_slot = static_cast<const uint8_t*>(e->d_nrtw_eslot.p);
  w.ent_qty = static_cast<const int64_t*>(e->d_nrtw_eqty.p);
  w.row_begin = row_begin;
  w.row_end = row_end;
  w.out_status = static_cast<uint8_t*>(e->status[SPX_PLUGIN_NRT].p);
  w.out_score = static_cast<uint8_t*>(e->score[SPX_PLUGIN_NRT].p);
  w.out_raw = out_raw;
  spx::launch_nrt_wide(w, e->stream);
  SPX_HIP(e, hipGetLastError());
  return SPX_OK;
}

// the reference-arithmetic NRT kernel's request column, when the coming launch may take that kernel and the batch did not ship it
// (`force`: whatever form the dense sweep takes — the tall nodes' kernel reads the column in every case)
int ensure_nrt_creq(spx_engine* e, bool force) {
  const bool fast = e->nrt_fast_slots && e->nrt_fast_nodes && e->nrt_fast_pods && !forced_reference(e, SPX_PLUGIN_NRT) &&
                    !(e->nrt_params.strategy == SPX_NRT_LEAST_NUMA_NODES && !(e->nrt_ln_ok && e->nrt_ln_built));
  if ((fast && !force) || e->nrt_creq_valid) return SPX_OK;
  const size_t bytes = static_cast<size_t>(e->n_pods) * SPX_NRT_MAX_CTRS * static_cast<size_t>(e->nrt_n_res) * sizeof(int64_t);
  int rc = ensure(e, e->d_nrt_creq, bytes);
  if (rc) return rc;
  spx::launch_nrt_creq_from_items(static_cast<const uint32_t*>(e->d_nrt_items.p), e->nrt_n_res, e->n_pods, static_cast<int64_t*>(e->d_nrt_creq.p), e->stream);
  SPX_HIP(e, hipGetLastError());
  e->nrt_creq_valid = true;
  return SPX_OK;
}

}  // namespace spx_eng
