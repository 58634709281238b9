// spx_engine.h — the engine's state and the helpers its translation units share (round 6: csrc/spx_engine.hip, one file of 3 900 lines
// in round 5, is now spx_engine.hip (lifecycle, options, parameters, evaluation, fetch), spx_uploads.hip (tables and deltas into HBM),
// spx_loads.hip (the one-call loaders) and spx_commit.hip (the one-pod-at-a-time loops)).  Not part of the ABI.  The helpers sit in an anonymous namespace:
// every translation unit gets its own copy of the small ones it uses; the three thread-local error slots exist once (spx_engine.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <unordered_map>
#include <vector>

#include <atomic>
#include <mutex>
#include <thread>

#include "spx_internal.h"
#include "../host/lroc_form.hpp"
#include "../host/nrt_streams.hpp"
#include "../host/parallel.hpp"

extern thread_local std::string g_create_error;          // spx_create's failure (no engine to hold it)
extern thread_local std::string tl_err;                  // this thread's last failure ...
extern thread_local const spx_engine* tl_err_engine;     // ... and on which engine

namespace {


struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  bool external = false;
};

}  // namespace

struct spx_engine {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool alloc_compact = false;     // k_alloc_prepare found the raw scores spanning less than 2^32 (AllocPrepArgs.rel is valid)
  bool timed = false;
  // last error: the engine's own copy (whoever failed last) under a lock; every thread also keeps the text of ITS last failure
  // (spx_last_error returns thread-local storage: concurrent readers may fail concurrently)
  mutable std::string err;
  mutable std::mutex err_mu;
  std::mutex raw_mu;  // spx_fetch_raw launches on the engine stream into one scratch row: concurrent callers take turns

  int64_t n_nodes = -1;
  int64_t n_pods = -1;
  int64_t row_stride = 0;

  // spx_set_option state (per engine; nothing is read from the environment)
  int64_t option[SPX_NUM_OPTIONS] = {spx::kRowPad, 0, 0, 0, 0, 0, 44, 1, 1, 375, 1, 1, 0, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1};

  // params
  int32_t alloc_mode = SPX_MODE_LEAST;
  std::vector<int32_t> alloc_res{SPX_RES_MEMORY, SPX_RES_CPU};
  std::vector<int64_t> alloc_weight{1, 1 << 20};  // defaultResourcesToWeightMap resource_allocation.go:36
  spx_tlp_params tlp{40, 1000, 1.5};             // apis/config/v1/defaults.go:51-55
  spx_lvrb_params lvrb{1.0, 1.0};                // defaults.go:65-67
  int64_t plugin_weight[SPX_NUM_PLUGINS] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};  // (Coscheduling's entry is never read)

  // device tables
  DevBuf d_alloc, d_alloc_w, d_alloc_raw, d_alloc_norm, d_alloc_rel;
  int32_t alloc_n_res = 0;
  bool alloc_ready = false;  // raw/norm computed for the current table + params
  DevBuf d_alloc_prev;       // the d_alloc_norm before the last recomputation (prepare_alloc compares the two)
  uint64_t alloc_epoch = 0;  // generation of d_alloc_norm's content: prepare_alloc bumps it when the row it computes differs from the one before
  DevBuf d_cap_cpu, d_tlp_util, d_tlp_missing, d_tlp_valid;
  DevBuf d_lv_acpu, d_lv_amem, d_lv_cavg, d_lv_cstd, d_lv_mavg, d_lv_mstd, d_lv_flags;
  bool tri_nodes = false;
  DevBuf d_tlp_pod, d_lv_rcpu, d_lv_rmem;
  bool tri_pods = false;
  DevBuf d_raw_row;  // int64 [n_nodes] staging for spx_fetch_raw
  DevBuf d_lv_exact; // double [n_nodes][8] scratch of the LVRB fast kernel
  DevBuf d_lv_fast, d_tlp_fast;  // float32 per-node constants of the fast sweeps (recomputed per launch)
  DevBuf d_tlp_amb;              // k_tlp_amb_build's table: per pod value, the node tiles holding a cell the float32 sweep cannot prove
  DevBuf d_lv_amb;               // k_lvrb_amb_build's table
  bool lv_amb_built = false;     // ... and whether d_lv_exact / d_lv_fast / d_lv_amb still describe the LVRB node columns and parameters
  int64_t tlp_amb_geom[3] = {0, 0, 0}, lv_amb_geom[3] = {0, 0, 0};  // the tiling / stride / target the tables were built for (tlp_prepare compares)
  bool tlp_amb_built = false;    // ... and whether it still describes d_cap_cpu / d_tlp_util / d_tlp_missing / d_tlp_valid and the target (cleared by every writer of those)
  // TargetLoadPacking's pod classes (SPX_OPT_TLP_POD_CLASSES): the rows of d_tlp_pod sorted by value, built by every writer of that
  // column (tlp_build_order) and invalidated by it first, so that no sweep can meet an order of another batch
  DevBuf d_tlp_order, d_tlp_order_scratch;
  bool tlp_order_valid = false;
  int64_t tlp_rows_evaluated = 0;  // of the batch in the class form: chunk starts of the order + changes of value
  int tlp_last_form = 0;           // spx_tlp_form: what the last spx_eval of TargetLoadPacking launched (0 none, 1 plain, 2 classes)
  DevBuf d_commit;               // scratch of spx_commit_sequential
  DevBuf d_decide;               // per-tile partial decisions of spx_decide
  DevBuf d_stats;                // uint64 [SPX_NUM_PLUGINS]: cells re-evaluated by the fast sweeps' exact fallback

  // LowRiskOverCommitment (reads the LVRB node columns above as well)
  spx_lroc_params lroc{5, 0.5, 0.5};  // apis/config/v1/defaults.go:72-80
  DevBuf d_lroc_nreq_c, d_lroc_nreq_m, d_lroc_nlim_c, d_lroc_nlim_m, d_lroc_preq_c, d_lroc_preq_m, d_lroc_plim_c, d_lroc_plim_m, d_lroc_tab, d_lroc_podf;
  bool lroc_nodes = false, lroc_pods = false, lroc_tab_ready = false;
  bool lroc_nodes_exact = false, lroc_pods_exact = false, lv_alloc_exact = false;  // all values in [0, 2^52)
  // the float32 sweep's preconditions (kernels_lroc.hip): all values in [0, 2^47), limits not below requests
  bool lroc_nodes_f32 = false, lroc_pods_f32 = false, lv_alloc_f32 = false;
  // what selects the form a sequential commit of a batch runs (lroc_commit_form, host/lroc_form.hpp): per column {req cpu, req mem,
  // lim cpu, lim mem} the largest node sum and the pods' values, and "no limit below its request" for the node sums / the pods
  int64_t lroc_node_max[4] = {0, 0, 0, 0};
  std::vector<int64_t> h_lroc_pod[4];
  bool lroc_nodes_cover = false, lroc_pods_cover = false;
  int lroc_loop_form = -1;  // spx::kLrocForm* while the sequential commit loop evaluates LowRiskOverCommitment, -1 otherwise (spx_eval)
  bool peaks_loop_row = false;  // the sequential commit loop evaluates Peaks per pod, against the pod's current status rows (Filter plugins in the mask)
  int lroc_last_form = -1;  // the form the last sequential commit ran, until the next spx_eval of the plugin or upload (spx_kernel_path)

  // Peaks
  DevBuf d_pk_cap, d_pk_util, d_pk_valid, d_pk_k1, d_pk_k2, d_pk_pod, d_pk_min, d_pk_max, d_pk_rowc, d_pk_tab, d_pk_seg, d_pk_segn;
  bool peaks_nodes = false, peaks_pods = false;

  // SySched: node columns, the stale CSR (host copy: a delta rebuilds it whole — the lists are short and rare), the distinct sets,
  // the pods ordered by set (classes = sets), the chunked raw table and the sets' maxima
  DevBuf d_sy_host, d_sy_present, d_sy_k, d_sy_a, d_sy_sptr, d_sy_sbit, d_sy_scnt;
  DevBuf d_sy_sets, d_sy_empty, d_sy_pod_set, d_sy_order, d_sy_first, d_sy_dups, d_sy_raw, d_sy_max;
  bool sy_nodes = false, sy_pods = false;
  int32_t sy_node_words = 0, sy_pod_words = 0, sy_n_sets = 0;
  std::vector<int32_t> h_sy_sptr, h_sy_sbit, h_sy_scnt, h_sy_pod_set, h_sy_first;
  int64_t sy_n_dups = 0, sy_n_tasks = 0;
  int sy_last_chunks = 0;  // spx_kernel_path(SYSCHED)

  // NodeMetadata / PodState: the raw int64 column per node and the scratch row the pod-independent normalisation is broadcast from
  DevBuf d_nm_raw, d_ps_raw, d_ncol_row;
  bool nm_nodes = false, ps_nodes = false;

  // Coscheduling: the snapshot's left-overs and their scan, the groups' requests / steps / flags, the verdicts and the pods' status.
  // cs_gate_valid: scan and gate hold for the tables in place (any upload clears it); cs_rows: the pod rows whose status is current
  DevBuf d_cs_left, d_cs_present, d_cs_prefix, d_cs_smax, d_cs_stotal, d_cs_any, d_cs_req, d_cs_mask, d_cs_sptr, d_cs_snode, d_cs_scum, d_cs_walk;
  DevBuf d_cs_pass, d_cs_open, d_cs_gap, d_cs_exists, d_cs_minm, d_cs_hasres, d_cs_backoff, d_cs_permit, d_cs_listed, d_cs_gated, d_cs_pod_group, d_cs_status;
  bool cosched = false, cs_gate_valid = false;
  int32_t cs_n_slots = 0, cs_n_groups = 0, cs_n_walk = 0;
  int cs_last_walk = 0;  // spx_kernel_path(COSCHED)
  int64_t cs_row_begin = 0, cs_row_end = 0;

  // NodeResourceTopologyMatch
  spx_nrt_params nrt_params{SPX_NRT_LEAST_ALLOCATED, 0, nullptr, nullptr};  // defaults.go:87-90
  int32_t nrt_n_res = 0;
  uint8_t nrt_slot_flags[SPX_NRT_MAX_RES] = {0};
  int64_t nrt_slot_weight[SPX_NRT_MAX_RES] = {0};
  bool nrt_slots = false, nrt_nodes = false, nrt_pods = false;
  DevBuf d_nrt_flags, d_nrt_max_numa, d_nrt_nz, d_nrt_zid, d_nrt_zp, d_nrt_avail, d_nrt_cost, d_nrt_minavg, d_nrt_np;
  DevBuf d_nrt_qos, d_nrt_nn, d_nrt_nctr, d_nrt_ckind, d_nrt_cpres, d_nrt_creq, d_nrt_ppres, d_nrt_preq;
  // float64 formulation of the NRT sweep (kernels_nrt_fast.hip): derived tables + whether its preconditions hold
  DevBuf d_nrt_fav, d_nrt_frc, d_nrt_frcv, d_nrt_fcpu, d_nrt_fbraw, d_nrt_frep, d_nrt_items, d_nrt_perm, d_nrt_ln;
  std::vector<double> nrt_wtab;  // [2^n_res][2]: sum of the weights of a slot subset, its biased reciprocal
  bool nrt_fast_slots = false, nrt_fast_nodes = false, nrt_fast_pods = false;
  DevBuf d_nrt_lnrec;      // LeastNUMANodes: the nodes' tables as one record each (scratch of a batch launch)
  DevBuf d_nrt_redo;       // BalancedAllocation: list of the cells the float32 Score launch leaves to the float64 form
  uint32_t nrt_redo_cap = 0;
  uint32_t nrt_big_nodes = ~0u, nrt_big_pods = ~0u;  // slots with a capacity / a request (Value() form) that float32 does not hold exactly
  // per slot, Value() form: OR and maximum of the zone capacities / of the requests in place (the packed float32 LeastAllocated Score's
  // preconditions, nrt_packed_score; delta uploads only ever add to them)
  using NrtQty = spx_host::NrtQty;
  NrtQty nrt_qty_nodes, nrt_qty_pods;
  int32_t nrt_slot_res[SPX_NRT_MAX_RES] = {0};       // canonical resource id of each slot (the packed Score's table slot is memory's)
  DevBuf d_nrt_pk_tab;                               // k_nrt_pk_tab_build's table ...
  bool nrt_pk_tab_built = false;                     // ... and whether it describes the zone capacities in place
  // pod equivalence classes (spx_upload_nrt_pods): rows whose NRT records agree in everything the sweep reads
  bool nrt_creq_valid = false;   // d_nrt_creq (read by the reference-arithmetic kernel only) holds this batch's column
  void* h_stage = nullptr;       // pinned staging of the blob uploads (DeltaBlob: node tables and deltas) and spx_load_trimaran_pods
  size_t h_stage_bytes = 0;
  void* h_items = nullptr;       // pinned staging of the NRT pod record stream, built in place (its own buffer: spx_load_nrt's node and pod halves run side by side)
  size_t h_items_bytes = 0;
  DevBuf d_delta;                // staged rows of a node-table delta (spx_update_*_nodes)
  // long rows (pods with more than SPX_NRT_MAX_CTRS containers): their containers in CSR (spx_upload_nrt_long_pods), evaluated by
  // kernels_nrt_long.hip after the dense sweep
  std::vector<int32_t> h_nrt_long_rows;  // rows of the uploaded batch whose n_ctr is SPX_NRT_CTRS_LONG, ascending
  bool nrt_long_ok = true;               // the long table describes those rows (trivially true without any)
  int64_t nrt_long_last = 0;             // spx_nrt_long_rows
  DevBuf d_nrtl_row, d_nrtl_ptr, d_nrtl_kind, d_nrtl_pres, d_nrtl_req, d_nrtl_map;
  // tall nodes (more than SPX_NRT_MAX_ZONES zones): their zones in a side table (spx_upload_nrt_tall_nodes), evaluated by
  // kernels_nrt_tall.hip after the dense sweep and the long rows
  std::vector<int32_t> h_nrt_tall_nodes;  // nodes of the uploaded table whose n_zones is SPX_NRT_ZONES_TALL, ascending
  bool nrt_tall_ok = true;                // the side table describes those nodes (trivially true without any)
  int64_t nrt_tall_last = 0;              // spx_nrt_tall_count
  int32_t nrt_tall_stride = 0;            // the side table's zone_stride
  int32_t nrt_tall_ln_node = -1, nrt_tall_ln_zones = 0;  // the first tall node with more zones than LeastNUMANodes takes, its count
  DevBuf d_nrtt_idx, d_nrtt_flags, d_nrtt_max, d_nrtt_np, d_nrtt_nz, d_nrtt_zid, d_nrtt_zp, d_nrtt_avail, d_nrtt_cost, d_nrtt_minavg;
  DevBuf d_nrtt_work, d_nrtt_cmask, d_nrtt_cstart;  // the waves' working copies; LeastNUMANodes' subset table (built when first needed)
  bool nrt_tall_combos = false;
  // the wide NRT tables (more than SPX_NRT_MAX_RES slots, or SPX_OPT_NRT_WIDE; kernels_nrt_wide.hip).  nrt_wide: they, not the dense
  // tables above, are the engine's NRT state (spx_upload_nrt_slots_wide sets it, spx_upload_nrt_slots clears it)
  bool nrt_wide = false;
  bool nrtw_slots = false, nrtw_nodes = false, nrtw_pods = false;
  int32_t nrtw_n_res = 0;
  DevBuf d_nrtw_sflags, d_nrtw_sweight;
  DevBuf d_nrtw_flags, d_nrtw_max_numa, d_nrtw_nz, d_nrtw_zid, d_nrtw_zp, d_nrtw_avail, d_nrtw_cost, d_nrtw_minavg, d_nrtw_np;
  DevBuf d_nrtw_qos, d_nrtw_nn, d_nrtw_rptr, d_nrtw_rslot, d_nrtw_rqty, d_nrtw_cptr, d_nrtw_ckind, d_nrtw_eptr, d_nrtw_eslot, d_nrtw_eqty;
  DevBuf d_nrt_uniq, d_nrt_dups;  // int32 [n_uniq] representative rows, ascending; int32 [n_dups][2] (row, its representative)
  int64_t nrt_n_uniq = 0, nrt_n_dups = 0, nrt_n_tasks = 0;  // (d_nrt_dups: the pairs sorted by representative, then the copy tasks — expand_tasks)
  DevBuf d_nrt_rk, d_nrt_rk_off;  // rank-space Filter: the chunk stream of the listed rows (nrt_build_rank_stream) and its chunk offsets
  uint32_t nrt_rk_max_dwords = 0;  // largest chunk block; 0 = no stream (the float64 Filter runs)
  // which rows the stream lists: 1 = the class representatives (d_nrt_uniq), 2 = every row in order (sweeps without pod classes:
  // built when such a sweep first asks for it, nrt_rank_stream_all); 0 = none, -1 = the batch has no finite stream (> 3 app containers)
  int nrt_rk_kind = 0;
  DevBuf d_nrt_rk_first;          // [chunks + 1] list position of each chunk's first row (a chunk holds up to 32)
  uint32_t nrt_rk_chunks = 0;
  bool nrt_rk_all_narrow = false;  // every chunk keeps four zones' counts per register (the only layout the fused sweep has)
  DevBuf d_nrt_wsort, d_nrt_wrank;  // the fused walk's per-window sorted cell quantities and the cells' ranks (k_nrt_window_sort) ...
  bool nrt_wsort_built = false;     // ... and whether they describe the zone tables in place (cleared with nrt_pk_tab_built: every writer of the zone quantities)
  DevBuf d_nrt_fz;  // fused Filter + Score sweep: the packed Score items of the listed rows (k_nrt_fused_pack)
  // what d_nrt_fz was packed from: generation of the pod records / slot table (bumped by their uploads), the row list's kind, the table
  // slot, the buffer — a sweep whose key matches skips the pack launch
  uint64_t nrt_items_gen = 1;
  struct FzKey {
    uint64_t gen = 0;
    int kind = 0, tab_slot = -2;
    const void* buf = nullptr;
    bool operator==(const FzKey& o) const { return gen == o.gen && kind == o.kind && tab_slot == o.tab_slot && buf == o.buf; }
  } nrt_fz_key;
  int last_nrt_filter = 0;         // spx_nrt_filter_path
  DevBuf d_pk_uniq, d_pk_dups;    // the same for Peaks: classes of pods with equal cpu requests
  int64_t pk_n_uniq = 0, pk_n_dups = 0, pk_n_tasks = 0;
  bool pk_negative = false;  // a Peaks pod row with a negative cpu request (never from a v1.Pod): the interval estimate's bounds assume >= 0
  bool nrt_ln_ok = false;  // LeastNUMANodes tables can be built: every zone cost within [0, 255]
  bool nrt_ln_built = false;
  std::vector<int32_t> h_nrt_cost;  // [N][Z][Z] host copy of the zone costs, what build_ln_tab works from
  std::vector<uint8_t> h_nrt_nz;
  int32_t nrt_cpu_slot = -1;
  DevBuf status[SPX_NUM_PLUGINS];

  // NetworkOverhead / TopologicalSort
  bool net_nodes = false, net_topo = false, net_pods = false;
  int32_t net_n_regions = 0, net_n_zones = 0, net_n_classes = 0;
  int64_t net_max_cost = SPX_NET_MAX_COST, net_max_pairs = 0;  // bound of a row's accumulated cost: their product (net_cost_bound) selects the 32- or the 64-bit sweep
  bool net_wide_dev = false;                  // d_net_rcost / d_net_zcost hold int64 entries (a wide upload, or widened by net_prepare); never both widths
  std::vector<int64_t> h_net_rcost, h_net_zcost;  // host copy of the cost matrices (net_prepare widens from it)
  DevBuf d_net_region, d_net_zone, d_net_class, d_net_class16, d_net_cls_size, d_net_cls_region, d_net_cls_zone, d_net_rcost, d_net_zcost;
  bool net_class16 = false;
  DevBuf d_net_pod_key, d_net_key_flag, d_net_pair_ptr, d_net_pair_node, d_net_pair_max;
  // TopologicalSort keys
  DevBuf d_sort_prio, d_sort_ts, d_sort_group, d_sort_topo, d_sort_scratch;
  int64_t sort_n = 0;
  unsigned* h_sort_hist = nullptr;  // pinned (scratch of both sorts)
  // QOSSort keys (independent of TopologicalSort's): priority, class, timestamp as uploaded; the derived columns and the passes' scratch
  DevBuf d_qos_prio, d_qos_cls, d_qos_ts, d_qos_key, d_qos_none, d_qos_zero, d_qos_rank, d_qos_scratch;
  int64_t qos_n = 0;

  // profile-level state
  DevBuf d_ext_status;  // caller's feasibility mask, stored as a status table (0 = feasible)
  bool ext_mask = false;
  DevBuf d_best;              // [score int64 P | node int32 P | ties int32 P | feasible int32 P], one allocation
  void* h_best = nullptr;     // pinned staging of the same layout: one D2H per spx_fetch_best
  size_t h_best_bytes = 0;
  bool best_valid = false;

  // CapacityScheduling.PreFilter
  bool quota = false;
  int32_t q_n_namespaces = 0;
  int64_t q_agg_used[SPX_QUOTA_SLOTS] = {0}, q_agg_min[SPX_QUOTA_SLOTS] = {0};
  uint32_t q_agg_used_present = 0, q_agg_min_present = 0;
  DevBuf d_q_pod_ns, d_q_pod_prio, d_q_pod_req, d_q_pod_reqp, d_q_has, d_q_used, d_q_max, d_q_maxp, d_q_other, d_q_otherp;
  DevBuf d_q_nom_ptr, d_q_nom_prio, d_q_nom_idx, d_q_nom_req, d_q_nom_reqp, d_q_status;
  DevBuf d_q_usedp, d_q_min, d_q_minp, d_q_agg;  // commit loop: Used key presence, Min per namespace, [8 aggregate used | presence]
  bool q_has_min = false;
  size_t q_n_nominated = 0;
  const int64_t* q_agg_dyn = nullptr;  // set while the sequential commit loop runs: k_quota reads the aggregate from the device
  // CapacityScheduling.PostFilter, the preemption dry run (spx_preempt.hip): the uploaded tables (k_preempt_marks completes the pods' marks), and the
  // last dry run's row list, node mask, row records, cells and picks.  pre_marks_valid: the marks describe the quota and node tables
  // in place; pre_valid: so do the results (every upload of either clears both)
  DevBuf d_pre_nodes, d_pre_podrec, d_pre_noms, d_pre_pdb_allowed;  // spx::PreemptNode / PreemptPod / PreemptNom records, packed by the upload
  DevBuf d_pre_pod_fit, d_pre_rows, d_pre_mask, d_pre_rec, d_pre_cells, d_pre_pick, d_pre_one;
  bool pre_nodes = false, pre_pods = false, pre_marks_valid = false, pre_valid = false, pre_has_mask = false;
  int64_t pre_n_rows = 0, pre_row_stride = 0;
  std::vector<int32_t> h_pre_pod_ptr, h_pre_hi;  // host copies: spx_fetch_preempt_victims orders a cell's victim set by them
  // PreemptionToleration's dry run shares the tables, the cells and the picks above.  ptol_table: spx_upload_preempt_toleration's records
  // describe the node table in place (spx_upload_preempt_nodes clears it); pre_toleration: the last dry run was the toleration one, so
  // the fetches read ptol's row records and spx_fetch_preempt_victims recomputes with k_ptol_cells at ptol_now
  DevBuf d_ptol_pods, d_ptol_meta, d_ptol_rec;
  bool ptol_table = false, pre_toleration = false;
  int64_t ptol_now = 0;
  // The sequential loop (spx_preempt_toleration_sequential) is the third mode: pre_sequential with pre_toleration.  d_pseq: the
  // overlay, the stored victim sets and the dirty lists, carved from one allocation; d_pseq_nom: the host-built CSR of each row's own
  // uploaded nominations.  pseq_victims: where the victim sets start.  h_pre_nom_*: host copies of the nominated records' node CSR and
  // pending rows, from which that CSR is built.
  DevBuf d_pseq, d_pseq_nom;
  bool pre_sequential = false;
  const uint32_t* pseq_victims = nullptr;
  std::vector<int32_t> h_pre_nom_ptr;
  std::vector<int64_t> h_pre_nom_row;
  // CapacityScheduling's loop (spx_preempt_sequential) is the fourth mode: pre_sequential without pre_toleration.  It carves its
  // overlay from d_pseq and puts its rows' own nominations into d_pseq_nom as the other loop does.  d_pre_nomq: the side table of
  // spx_upload_preempt_nominated_quota, [ns int32 | quota_req 8 x int64 | present uint8] per nominated record, carved; pre_nomq: it
  // describes the node table in place (spx_upload_preempt_nodes clears it).  d_pre_elig: the loop's eligible column.
  DevBuf d_pre_nomq, d_pre_elig;
  bool pre_nomq = false;
  // The toleration dry run with NRT's Filter in the refit (spx_preempt_toleration_nrt_dry_run) is the fifth mode: pre_toleration with
  // pre_nrt; CapacityScheduling's with it (spx_preempt_nrt_dry_run) the sixth: pre_nrt alone.  Every staging clears pre_nrt and the two
  // entry points set it.  d_pnrt_*: spx_upload_preempt_nrt's side table as spx::PnrtNode / PnrtRel records and the preemptors' columns carved from
  // one allocation (pnrt_pod_off: qos, non_native, n_ctr, ctr_kind, ctr_present, pod_present, ctr_req, pod_req); pnrt_table: it
  // describes the node and pod tables in place (an upload of either clears it); pnrt_mode: the last run's preemption mode, for the
  // victims fetch.  The toleration loop with that Filter (spx_preempt_toleration_nrt_sequential) is the seventh mode: pre_toleration,
  // pre_nrt and pre_sequential; the fetches branch on pre_sequential first, so its victims are the stored sets of the third mode.
  // CapacityScheduling's loop with it (spx_preempt_nrt_sequential) is the eighth: pre_nrt and pre_sequential without pre_toleration, its
  // victims the stored sets likewise.  Every run's staging (preempt_stage) clears pre_nrt, so a loop without the Filter after one
  // with it is not taken for an NRT result.
  DevBuf d_pnrt_nodes, d_pnrt_contrib, d_pnrt_rel_ptr, d_pnrt_rel, d_pnrt_pods, d_pnrt_rec;
  bool pnrt_table = false, pre_nrt = false;
  int32_t pnrt_n_res = 0, pnrt_mode = 0, pnrt_max_zones = 0;
  uint64_t pnrt_slot_flags = 0;
  size_t pnrt_pod_off[8] = {0};
  // NetworkOverhead in the commit loop: per-pod effects + the workload pair lists rebuilt with room to grow
  std::vector<int32_t> h_pair_ptr, h_eff_ptr, h_eff_key;
  std::vector<uint8_t> h_key_flag;            // host copy of key_score_equally (spx_update_net_placed edits it)
  DevBuf d_net_pair_node2, d_net_pair_max2;   // the other half of the pair lists' ping-pong (spx_update_net_placed)
  std::vector<int64_t> h_eff_cost;
  DevBuf d_net_eff_ptr, d_net_eff_key, d_net_eff_cost, d_net_dyn_ptr, d_net_dyn_end, d_net_dyn_node, d_net_dyn_max;
  bool net_commit = false, net_dyn_active = false;
  int32_t net_n_keys = 0;
  DevBuf d_commit_save;  // backup of every table the commit loop mutates
  DevBuf d_coop_sync, d_coop_node, d_coop_max;  // cooperative commit kernel: granules + error flag, the workgroups' private pair lists
  double load_nrt_ms[6] = {0};  // stages of the last spx_load_nrt (spx_last_load_nrt_ms)
  bool in_commit_loop = false;  // commit_with_filters' per-pod launches are running on mutated zone tables (fill_nrt)
  int coop_gave_up = 0;      // cooperative commit launches that ended with a workgroup giving up (served by the per-pod loop instead)
  int last_commit_path = 0;  // what the last spx_commit_sequential ran: 1 one-workgroup trimaran chain, 2 per-pod launches, 3 cooperative kernel
  DevBuf d_row_counter;  // int64: the row the replayed per-pod graph works on
  const int64_t* row_indirect = nullptr;  // non-NULL while that graph is captured: sweeps read their row from the device

  DevBuf score[SPX_NUM_PLUGINS];
  int64_t score_rows[SPX_NUM_PLUGINS] = {0};
  int64_t score_stride[SPX_NUM_PLUGINS] = {0};
  uint32_t evaluated = 0;  // plugins with valid rows
  // what each plugin's table currently holds: the row range evaluated, and under which feasibility context — the Filter
  // plugins of that spx_eval call and the caller's mask generation — NormalizeScore-type plugins ran (upstream normalises over
  // the nodes that passed every Filter of the cycle, so a table is only meaningful together with that set)
  struct EvalInfo {
    int64_t begin = 0, end = 0;
    uint32_t filters = 0;
    uint64_t ext_gen = 0;
  } eval_info[SPX_NUM_PLUGINS];
  uint64_t ext_gen = 0;
  // SPX_OPT_ALLOC_TABLE_KEEP: the rows of Allocatable's engine-owned score table that hold the unmasked broadcast of d_alloc_norm —
  // which buffer and stride they were written to and from which generation of the row (alloc_epoch).  Recorded by spx_eval once the
  // launch that writes them has been issued; an spx_eval whose rows lie inside, with the same buffer, stride and epoch, leaves
  // Allocatable's stores out of the sweep.  Buffer, stride and epoch are compared at use; everything else that writes into the
  // table (the masked normalisations, a bound table, a reallocation) resets the record: alloc_table_dirty.
  struct AllocKept {
    int64_t begin = 0, end = 0;
    const void* buf = nullptr;
    int64_t stride = 0;
    uint64_t epoch = 0;
  } alloc_kept;
  int last_alloc_table = 0;  // spx_alloc_table_path
};


namespace {


int fail(const spx_engine* e, int code, const std::string& msg) {
  if (e) {
    {
      std::lock_guard<std::mutex> g(e->err_mu);
      e->err = msg;
    }
    tl_err = msg;
    tl_err_engine = e;
  } else {
    g_create_error = msg;
  }
  return code;
}

#define SPX_HIP(e, call)                                                                          \
  do {                                                                                            \
    hipError_t _st = (call);                                                                      \
    if (_st != hipSuccess)                                                                        \
      return fail((e), SPX_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_st));          \
  } while (0)

int ensure(spx_engine* e, DevBuf& b, size_t bytes) {
  if (b.external) return fail(e, SPX_ERR_STATE, "internal: resize of an externally bound buffer");
  if (bytes == 0) bytes = 16;
  if (b.bytes >= bytes) return SPX_OK;
  if (b.p) SPX_HIP(e, hipFree(b.p));
  b.p = nullptr;
  b.bytes = 0;
  SPX_HIP(e, hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  return SPX_OK;
}

int upload(spx_engine* e, DevBuf& b, const void* src, size_t bytes) {
  if (!src && bytes) return fail(e, SPX_ERR_ARG, "NULL column in table");  // an empty column (e.g. no resource slots) may be NULL
  int rc = ensure(e, b, bytes);
  if (rc) return rc;
  if (bytes) SPX_HIP(e, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, e->stream));
  return SPX_OK;
}

// a pinned host buffer of at least `want` bytes; a buffer that has to grow is allocated with `slack` bytes to spare
int ensure_pinned(spx_engine* e, void*& p, size_t& bytes, size_t want, size_t slack) {
  if (bytes >= want) return SPX_OK;
  if (p) SPX_HIP(e, hipHostFree(p));
  p = nullptr, bytes = 0;
  SPX_HIP(e, hipHostMalloc(&p, want + slack, hipHostMallocDefault));
  bytes = want + slack;
  return SPX_OK;
}

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

int set_nodes(spx_engine* e, int64_t n) {
  if (n <= 0) return fail(e, SPX_ERR_ARG, "n_nodes must be positive");
  if (e->n_nodes != -1 && e->n_nodes != n)
    return fail(e, SPX_ERR_STATE, "n_nodes differs from tables already uploaded (one snapshot per engine; destroy and re-create to change shape)");
  e->n_nodes = n;
  e->row_stride = spx::round_up(n, e->option[SPX_OPT_ROW_ALIGN]);
  return SPX_OK;
}

int set_pods(spx_engine* e, int64_t p) {
  if (p <= 0) return fail(e, SPX_ERR_ARG, "n_pods must be positive");
  if (e->n_pods != -1 && e->n_pods != p)
    return fail(e, SPX_ERR_STATE, "n_pods differs from tables already uploaded");
  e->n_pods = p;
  return SPX_OK;
}

// The order of TargetLoadPacking's class form for the pod column in place (n_pods rows of d_tlp_pod, queued on the stream before
// this call): built on the stream, the count of evaluated rows read back.  The caller has cleared tlp_order_valid before it wrote the
// column and synchronises the stream afterwards anyway; this synchronises for the one number.
int tlp_build_order(spx_engine* e) {
  e->tlp_order_valid = false;
  if (e->n_pods <= 0 || e->n_pods > std::numeric_limits<int32_t>::max()) return SPX_OK;  // (rows are int32 in the order: such a batch sweeps plain)
  int rc;
  const size_t words = spx::tlp_order_scratch_words(spx::kTlpAmbSize, e->n_pods);
  if ((rc = ensure(e, e->d_tlp_order, static_cast<size_t>(e->n_pods) * sizeof(int32_t))) || (rc = ensure(e, e->d_tlp_order_scratch, words * sizeof(uint32_t))))
    return rc;
  uint32_t* scratch = static_cast<uint32_t*>(e->d_tlp_order_scratch.p);
  // (SPX_OPT_TLP_CHUNK_SCHED is read here: the order in place keeps the schedule it was built with)
  spx::launch_tlp_order(static_cast<const int64_t*>(e->d_tlp_pod.p), e->n_pods, spx::kTlpAmbSize, e->option[SPX_OPT_TLP_CHUNK_SCHED] != 0,
                        static_cast<int32_t*>(e->d_tlp_order.p), scratch, e->stream);
  SPX_HIP(e, hipGetLastError());
  uint32_t evaluated = 0;
  SPX_HIP(e, hipMemcpyAsync(&evaluated, scratch + spx::tlp_order_evaluated_word(spx::kTlpAmbSize), sizeof evaluated, hipMemcpyDeviceToHost, e->stream));
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->tlp_rows_evaluated = evaluated;
  e->tlp_order_valid = true;
  return SPX_OK;
}

// something other than the unmasked broadcast wrote (or may have written) into Allocatable's score table, or the buffer changed
void alloc_table_dirty(spx_engine* e) { e->alloc_kept = spx_engine::AllocKept{}; }

// The checks of a plugin's tables that write nothing (spx_eval makes them all before its first allocation): a table the caller bound
// must hold n_pods x row_stride ...
int score_table_fits(const spx_engine* e, int plugin) {
  if (e->score[plugin].external && (e->score_rows[plugin] < e->n_pods || e->score_stride[plugin] < e->row_stride))
    return fail(e, SPX_ERR_STATE, "bound score table is smaller than n_pods x row_stride");
  return SPX_OK;
}
int status_table_fits(const spx_engine* e, int plugin) {
  if (e->status[plugin].external && e->status[plugin].bytes < static_cast<size_t>(e->n_pods) * static_cast<size_t>(e->row_stride))
    return fail(e, SPX_ERR_STATE, "bound status table is smaller than n_pods x row_stride");
  return SPX_OK;
}
// ... and use the engine's row stride (an engine-owned table has it by construction: ensure_score_table)
int score_table_stride(const spx_engine* e, int plugin) {
  if (e->score[plugin].external && e->score_stride[plugin] != e->row_stride)
    return fail(e, SPX_ERR_STATE, "bound score table must use the engine row stride (spx_score_table reports it)");
  return SPX_OK;
}

int ensure_score_table(spx_engine* e, int plugin) {
  DevBuf& b = e->score[plugin];
  if (b.external) return score_table_fits(e, plugin);
  const size_t had = b.p ? b.bytes : 0;
  int rc = ensure(e, b, static_cast<size_t>(e->n_pods) * static_cast<size_t>(e->row_stride));
  if (plugin == SPX_PLUGIN_ALLOCATABLE && (rc || b.bytes != had)) alloc_table_dirty(e);  // (a new allocation may come back at the old address)
  if (rc) return rc;
  e->score_rows[plugin] = e->n_pods;
  e->score_stride[plugin] = e->row_stride;
  return SPX_OK;
}

constexpr uint32_t kFilterPlugins = (1u << SPX_PLUGIN_NRT) | (1u << SPX_PLUGIN_NETOVERHEAD);
// plugins whose NormalizeScore depends on the feasible set of the cycle
constexpr uint32_t kNormalizingPlugins =
    (1u << SPX_PLUGIN_ALLOCATABLE) | (1u << SPX_PLUGIN_NETOVERHEAD) | (1u << SPX_PLUGIN_PEAKS) | (1u << SPX_PLUGIN_SYSCHED) | (1u << SPX_PLUGIN_NODEMETA) |
    (1u << SPX_PLUGIN_PODSTATE);
// plugins that own a uint8 score table
constexpr bool plugin_has_score(int k) {
  return k <= SPX_PLUGIN_NETOVERHEAD || k == SPX_PLUGIN_LROC || k == SPX_PLUGIN_PEAKS || k == SPX_PLUGIN_SYSCHED || k == SPX_PLUGIN_NODEMETA || k == SPX_PLUGIN_PODSTATE;
}

// The status tables that narrow a pod's node list when `mask` is evaluated or summed: {NRT's, NetworkOverhead's, the caller's mask},
// NULL = not in play (the layout of ProfileArgs.status and the scorers' other_status; NetworkOverhead's own sweep takes [0] and [2])
void feasibility_status(const spx_engine* e, uint32_t mask, const uint8_t* out[3]) {
  out[0] = (mask & (1u << SPX_PLUGIN_NRT)) ? static_cast<const uint8_t*>(e->status[SPX_PLUGIN_NRT].p) : nullptr;
  out[1] = (mask & (1u << SPX_PLUGIN_NETOVERHEAD)) ? static_cast<const uint8_t*>(e->status[SPX_PLUGIN_NETOVERHEAD].p) : nullptr;
  out[2] = e->ext_mask ? static_cast<const uint8_t*>(e->d_ext_status.p) : nullptr;
}

// d_best's four columns, [score int64 P | node int32 P | ties int32 P | feasible int32 P]
struct BestRows {
  int64_t* score;
  int32_t *node, *ties, *feasible;
};
BestRows best_rows(const spx_engine* e) {
  int64_t* score = static_cast<int64_t*>(e->d_best.p);
  int32_t* node = reinterpret_cast<int32_t*>(score + e->n_pods);
  return BestRows{score, node, node + e->n_pods, node + 2 * e->n_pods};
}
int ensure_best(spx_engine* e, BestRows* out) {
  int rc = ensure(e, e->d_best, static_cast<size_t>(e->n_pods) * 20);
  if (rc == SPX_OK) *out = best_rows(e);
  return rc;
}

// What one evaluation is asked for besides its mask and rows (spx_decide's preparatory sweeps; spx_eval itself passes the defaults)
struct EvalCall {
  bool hold_ev0 = false;           // the caller has recorded ev0 and times this evaluation together with its own sweep
  bool skip_alloc_masked = false;  // the caller folds Allocatable's masked normalisation into its argmax kernel: the table is not written
};

// rows [b, e) of `plugin` hold results of an spx_eval
int rows_evaluated(const spx_engine* e, int plugin, int64_t b, int64_t en) {
  const spx_engine::EvalInfo& i = e->eval_info[plugin];
  if (!(e->evaluated & (1u << plugin)) || b < i.begin || en > i.end)
    return fail(e, SPX_ERR_STATE, "rows requested have not been evaluated for this plugin (spx_eval covers [" + std::to_string(i.begin) + ", " +
                                      std::to_string(i.end) + "))");
  return SPX_OK;
}

int ensure_status_table(spx_engine* e, int plugin) {
  DevBuf& b = e->status[plugin];
  if (b.external) return status_table_fits(e, plugin);
  return ensure(e, b, static_cast<size_t>(e->n_pods) * static_cast<size_t>(e->row_stride));
}

// what prepare_alloc refuses, from host state alone
int alloc_check(const spx_engine* e) {
  if (e->alloc_ready) return SPX_OK;
  if (!e->d_alloc.p) return fail(e, SPX_ERR_STATE, "Allocatable: spx_upload_alloc_nodes not called");
  if (e->alloc_n_res != static_cast<int32_t>(e->alloc_res.size()))
    return fail(e, SPX_ERR_STATE, "Allocatable: uploaded table has a different resource count than the params");
  return SPX_OK;
}

int prepare_alloc(spx_engine* e) {
  if (e->alloc_ready) return SPX_OK;
  int rc = alloc_check(e);
  if (rc) return rc;
  if ((rc = upload(e, e->d_alloc_w, e->alloc_weight.data(), e->alloc_weight.size() * sizeof(int64_t)))) return rc;
  if ((rc = ensure(e, e->d_alloc_raw, static_cast<size_t>(e->n_nodes) * sizeof(int64_t)))) return rc;
  if ((rc = ensure(e, e->d_alloc_rel, static_cast<size_t>(e->row_stride + 4) * sizeof(uint32_t)))) return rc;
  // (The comparison is a launch of its own, kernels_delta.hip's k_rows_equal, on a copy of the old row — not a few lines inside
  // k_alloc_prepare, which has both rows in hand: that kernel lives in kernels_trimaran.hip, whose machine code stamps the counter
  // profiles of every trimaran workload, and this runs once per node table, off the sweep.)
  // the row in place (if one was ever computed) is set aside: a recomputation that ends with the same row — a node re-list with
  // unchanged allocatable — keeps alloc_epoch, and with it the score table that broadcasts the row (SPX_OPT_ALLOC_TABLE_KEEP)
  const bool had_norm = e->alloc_epoch != 0 && e->d_alloc_norm.p && e->d_alloc_norm.bytes >= static_cast<size_t>(e->row_stride);
  if ((rc = ensure(e, e->d_alloc_norm, static_cast<size_t>(e->row_stride)))) return rc;
  if (had_norm) {
    if ((rc = ensure(e, e->d_alloc_prev, static_cast<size_t>(e->row_stride)))) return rc;
    SPX_HIP(e, hipMemcpyAsync(e->d_alloc_prev.p, e->d_alloc_norm.p, static_cast<size_t>(e->row_stride), hipMemcpyDeviceToDevice, e->stream));
  }
  const uint64_t epoch_before = e->alloc_epoch++;  // a failure below leaves the row unknown: the old epoch comes back only once the rows are known to agree
  spx::AllocPrepArgs a{};
  a.n_nodes = e->n_nodes;
  a.row_stride = e->row_stride;
  a.n_res = e->alloc_n_res;
  a.mode = e->alloc_mode;
  a.alloc = static_cast<const int64_t*>(e->d_alloc.p);
  a.weight = static_cast<const int64_t*>(e->d_alloc_w.p);
  a.raw = static_cast<int64_t*>(e->d_alloc_raw.p);
  a.rel = static_cast<uint32_t*>(e->d_alloc_rel.p);
  a.norm = static_cast<uint8_t*>(e->d_alloc_norm.p);
  spx::launch_alloc_prepare(a, e->stream);
  SPX_HIP(e, hipGetLastError());
  uint32_t* const flags = static_cast<uint32_t*>(e->d_alloc_rel.p) + e->row_stride;
  if (had_norm) {
    spx::launch_rows_equal(a.norm, static_cast<const uint8_t*>(e->d_alloc_prev.p), e->row_stride, flags + 1, e->stream);
    SPX_HIP(e, hipGetLastError());
  }
  // once per node table, in one copy: the flag the kernel leaves behind the offsets, and behind it "the row is the one before"
  uint32_t back[2] = {0, 0};
  SPX_HIP(e, hipMemcpyAsync(back, flags, had_norm ? sizeof back : sizeof back[0], hipMemcpyDeviceToHost, e->stream));
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->alloc_compact = back[0] != 0;
  if (had_norm && back[1] != 0) e->alloc_epoch = epoch_before;
  e->alloc_ready = true;
  return SPX_OK;
}

bool forced_reference(const spx_engine* e, int plugin) { return (e->option[SPX_OPT_REFERENCE_KERNELS] >> plugin) & 1; }

// the engine's options as the launch-level switches the kernel translation units read
uint32_t launch_opts(const spx_engine* e) {
  uint32_t o = 0;
  if (forced_reference(e, SPX_PLUGIN_TLP) || forced_reference(e, SPX_PLUGIN_LVRB)) o |= spx::kOptTrimaranExact;
  if (forced_reference(e, SPX_PLUGIN_NRT)) o |= spx::kOptNrtGeneric;
  if (forced_reference(e, SPX_PLUGIN_NETOVERHEAD)) o |= spx::kOptNetGeneric;
  if (e->option[SPX_OPT_NRT_SINGLE_LAUNCH]) o |= spx::kOptNrtSingleLaunch;
  if (e->option[SPX_OPT_COMMIT_FROM_MEMORY]) o |= spx::kOptCommitFromMemory;
  if (e->option[SPX_OPT_PEAKS_TILE] / 10 == 8) o |= spx::kOptPeaksWideA;
  if (e->option[SPX_OPT_PEAKS_TILE] % 10 == 8) o |= spx::kOptPeaksWideB;
  if (!e->option[SPX_OPT_TLP_AMB_TABLE]) o |= spx::kOptTlpNoAmbTable;
  if (e->option[SPX_OPT_PEAKS_ESTIMATE]) o |= spx::kOptPeaksEstimate;
  if (e->option[SPX_OPT_PEAKS_ESTIMATE] == 8) o |= spx::kOptPeaksEst8;
  return o;
}

bool lroc_exact53(const spx_engine* e) {
  return e->lroc_nodes_exact && e->lroc_pods_exact && e->lv_alloc_exact && !forced_reference(e, SPX_PLUGIN_LROC);
}
// the float32 sweep (k_lroc_fast) may run: exact columns, below 2^47, every limit at least its request (SetMaxLimits, resourcestats.go:227-231)
bool lroc_f32_ok(const spx_engine* e) {
  return lroc_exact53(e) && e->lroc_nodes_f32 && e->lroc_pods_f32 && e->lv_alloc_f32 && !e->option[SPX_OPT_LROC_FLOAT64];
}

void fill_lroc(const spx_engine* e, spx::LrocArgs& a) {
  a.n_nodes = e->n_nodes;
  a.row_stride = e->row_stride;
  a.alloc_cpu_milli = static_cast<const int64_t*>(e->d_lv_acpu.p);
  a.alloc_mem = static_cast<const int64_t*>(e->d_lv_amem.p);
  a.cpu_avg = static_cast<const double*>(e->d_lv_cavg.p);
  a.cpu_std = static_cast<const double*>(e->d_lv_cstd.p);
  a.mem_avg = static_cast<const double*>(e->d_lv_mavg.p);
  a.mem_std = static_cast<const double*>(e->d_lv_mstd.p);
  a.flags = static_cast<const uint8_t*>(e->d_lv_flags.p);
  a.node_req_cpu = static_cast<const int64_t*>(e->d_lroc_nreq_c.p);
  a.node_req_mem = static_cast<const int64_t*>(e->d_lroc_nreq_m.p);
  a.node_lim_cpu = static_cast<const int64_t*>(e->d_lroc_nlim_c.p);
  a.node_lim_mem = static_cast<const int64_t*>(e->d_lroc_nlim_m.p);
  a.pod_req_cpu = static_cast<const int64_t*>(e->d_lroc_preq_c.p);
  a.pod_req_mem = static_cast<const int64_t*>(e->d_lroc_preq_m.p);
  a.pod_lim_cpu = static_cast<const int64_t*>(e->d_lroc_plim_c.p);
  a.pod_lim_mem = static_cast<const int64_t*>(e->d_lroc_plim_m.p);
  a.sqrt_window = std::sqrt(static_cast<double>(e->lroc.smoothing_window_size));  // math.Pow(x, 0.5) = Sqrt(x)
  a.w_cpu = e->lroc.risk_limit_weight_cpu;
  a.w_mem = e->lroc.risk_limit_weight_mem;
  a.node_tab = static_cast<double*>(e->d_lroc_tab.p);
  a.exact53 = lroc_exact53(e) ? 1 : 0;
  a.pod_f32 = lroc_f32_ok(e) ? static_cast<const float*>(e->d_lroc_podf.p) : nullptr;
  a.n_pods_total = e->n_pods;
  a.stats = static_cast<unsigned long long*>(e->d_stats.p);
}

void fill_peaks(const spx_engine* e, spx::PeaksArgs& a) {
  a.opts = launch_opts(e);
  a.n_nodes = e->n_nodes;
  a.row_stride = e->row_stride;
  a.cap_cpu_milli = static_cast<const int64_t*>(e->d_pk_cap.p);
  a.cpu_util = static_cast<const double*>(e->d_pk_util.p);
  a.valid = static_cast<const uint8_t*>(e->d_pk_valid.p);
  a.k1 = static_cast<const double*>(e->d_pk_k1.p);
  a.k2 = static_cast<const double*>(e->d_pk_k2.p);
  a.pod_cpu_milli = static_cast<const int64_t*>(e->d_pk_pod.p);
  a.row_min = static_cast<int64_t*>(e->d_pk_min.p);
  a.row_max = static_cast<int64_t*>(e->d_pk_max.p);
  a.row_c = static_cast<float*>(e->d_pk_rowc.p);
  a.node_tab = static_cast<double*>(e->d_pk_tab.p);
}

void fill_sysched(const spx_engine* e, spx::SyschedArgs& a) {
  a.n_nodes = e->n_nodes;
  a.row_stride = e->row_stride;
  a.n_words = e->sy_node_words;
  a.host_bits = static_cast<const uint64_t*>(e->d_sy_host.p);
  a.present = static_cast<const uint8_t*>(e->d_sy_present.p);
  a.n_resident = static_cast<const int32_t*>(e->d_sy_k.p);
  a.resident_missing = static_cast<const int32_t*>(e->d_sy_a.p);
  a.stale_ptr = static_cast<const int32_t*>(e->d_sy_sptr.p);
  a.stale_bit = static_cast<const int32_t*>(e->d_sy_sbit.p);
  a.stale_count = static_cast<const int32_t*>(e->d_sy_scnt.p);
  a.set_bits = static_cast<const uint64_t*>(e->d_sy_sets.p);
  a.set_empty = static_cast<const uint8_t*>(e->d_sy_empty.p);
  a.pod_set = static_cast<const int32_t*>(e->d_sy_pod_set.p);
  a.order = static_cast<const int32_t*>(e->d_sy_order.p);
  a.set_first = static_cast<const int32_t*>(e->d_sy_first.p);
  a.raw = static_cast<int32_t*>(e->d_sy_raw.p);
  a.set_max = static_cast<int32_t*>(e->d_sy_max.p);
}

void fill_cosched(const spx_engine* e, spx::CoschedArgs& a) {
  a.n_nodes = e->n_nodes;
  a.n_slots = e->cs_n_slots;
  a.n_groups = e->cs_n_groups;
  a.n_walk = e->cs_n_walk;
  a.left_base = static_cast<const int64_t*>(e->d_cs_left.p);
  a.node_present = static_cast<const uint8_t*>(e->d_cs_present.p);
  a.prefix = static_cast<int64_t*>(e->d_cs_prefix.p);
  a.slot_max = static_cast<int64_t*>(e->d_cs_smax.p);
  a.slot_total = static_cast<int64_t*>(e->d_cs_stotal.p);
  a.any_present = static_cast<int32_t*>(e->d_cs_any.p);
  a.req = static_cast<const int64_t*>(e->d_cs_req.p);
  a.req_mask = static_cast<const uint32_t*>(e->d_cs_mask.p);
  a.step_ptr = static_cast<const int32_t*>(e->d_cs_sptr.p);
  a.step_node = static_cast<const int32_t*>(e->d_cs_snode.p);
  a.step_cum = static_cast<const int64_t*>(e->d_cs_scum.p);
  a.walk_group = static_cast<const int32_t*>(e->d_cs_walk.p);
  a.pass_mask = static_cast<uint32_t*>(e->d_cs_pass.p);
  a.open_mask = static_cast<uint32_t*>(e->d_cs_open.p);
  a.gap = static_cast<int64_t*>(e->d_cs_gap.p);
  a.g_exists = static_cast<const uint8_t*>(e->d_cs_exists.p);
  a.min_member = static_cast<const int32_t*>(e->d_cs_minm.p);
  a.has_min_resources = static_cast<const uint8_t*>(e->d_cs_hasres.p);
  a.backed_off = static_cast<const uint8_t*>(e->d_cs_backoff.p);
  a.permitted = static_cast<const uint8_t*>(e->d_cs_permit.p);
  a.listed = static_cast<const int32_t*>(e->d_cs_listed.p);
  a.gated = static_cast<const int32_t*>(e->d_cs_gated.p);
  a.pod_group = static_cast<const int32_t*>(e->d_cs_pod_group.p);
  a.out_status = static_cast<uint8_t*>(e->d_cs_status.p);
}

void fill_trimaran(const spx_engine* e, spx::TrimaranArgs& a) {
  a.opts = launch_opts(e);
  a.row_ptr = e->row_indirect;
  a.n_nodes = e->n_nodes;
  a.row_stride = e->row_stride;
  a.alloc_norm = static_cast<const uint8_t*>(e->d_alloc_norm.p);
  a.cap_cpu_milli = static_cast<const int64_t*>(e->d_cap_cpu.p);
  a.tlp_cpu_util = static_cast<const double*>(e->d_tlp_util.p);
  a.tlp_missing_milli = static_cast<const int64_t*>(e->d_tlp_missing.p);
  a.tlp_valid = static_cast<const uint8_t*>(e->d_tlp_valid.p);
  a.tlp_pod_milli = static_cast<const int64_t*>(e->d_tlp_pod.p);
  a.tlp_target = static_cast<double>(e->tlp.target_utilization);
  a.lv_alloc_cpu_milli = static_cast<const int64_t*>(e->d_lv_acpu.p);
  a.lv_alloc_mem = static_cast<const int64_t*>(e->d_lv_amem.p);
  a.lv_cpu_avg = static_cast<const double*>(e->d_lv_cavg.p);
  a.lv_cpu_std = static_cast<const double*>(e->d_lv_cstd.p);
  a.lv_mem_avg = static_cast<const double*>(e->d_lv_mavg.p);
  a.lv_mem_std = static_cast<const double*>(e->d_lv_mstd.p);
  a.lv_flags = static_cast<const uint8_t*>(e->d_lv_flags.p);
  a.lv_req_cpu_milli = static_cast<const int64_t*>(e->d_lv_rcpu.p);
  a.lv_req_mem = static_cast<const int64_t*>(e->d_lv_rmem.p);
  a.lv_margin = e->lvrb.safe_variance_margin;
  a.lv_sensitivity = e->lvrb.safe_variance_sensitivity;
  a.stats = static_cast<unsigned long long*>(e->d_stats.p);
}

// The packed float32 form of LeastAllocated's Score launch (nrt_fast_device.h, score_least_packed) needs every weighted slot to be
// "small" — with 2^s the largest power of two dividing all its capacities and requests, capacity / 2^s <= 32768 and request / 2^s < 2^24 —
// or, one slot at most and not cpu, to go through k_nrt_pk_tab_build's table indexed by request / unit, unit = the largest power of
// two dividing all its requests.  false = the float64 form.
struct NrtPacked {
  uint32_t small_slots = 0;
  int32_t tab_slot = -1;
  uint32_t tab_kmax = 0, tab_words = 0;
  double tab_inv_unit = 1.0;
};
constexpr int64_t kNrtSmallCap = 32768;
bool nrt_packed_score(const spx_engine* e, NrtPacked* out) {
  *out = NrtPacked{};
  // (MostAllocated: the same float32 products serve x = 100 v / c as serve 100 - x; only the fused walk consumes the answer for that strategy)
  if (!e->option[SPX_OPT_NRT_PACKED_SCORE] || !e->nrt_nodes || !e->nrt_pods || e->in_commit_loop ||
      (e->nrt_params.strategy != SPX_NRT_LEAST_ALLOCATED && !(e->nrt_params.strategy == SPX_NRT_MOST_ALLOCATED && e->option[SPX_OPT_NRT_FUSED])))
    return false;
  int64_t wsum = 0;
  for (int i = 0; i < e->nrt_n_res && i < SPX_NRT_MAX_RES; ++i) {
    if (e->nrt_slot_weight[i] < 0) return false;
    wsum += e->nrt_slot_weight[i];
  }
  if (wsum > spx::kNrtPkMaxWeightSum) return false;
  auto low_zeros = [](uint64_t bits) { return bits ? __builtin_ctzll(bits) : 63; };
  for (int i = 0; i < e->nrt_n_res && i < SPX_NRT_MAX_RES; ++i) {
    if (e->nrt_slot_weight[i] == 0) continue;  // contributes 0 whatever its resource score
    const uint64_t pod_bits = e->nrt_qty_pods.bits[i];
    if (pod_bits == 0) {  // no request but zeros: the resource score is 100 or 0 in both forms
      out->small_slots |= 1u << i;
      continue;
    }
    const int s = low_zeros(pod_bits | e->nrt_qty_nodes.bits[i]);
    if ((e->nrt_qty_nodes.most[i] >> s) <= kNrtSmallCap && (e->nrt_qty_pods.most[i] >> s) < (int64_t{1} << 24)) {
      out->small_slots |= 1u << i;
      continue;
    }
    const int su = low_zeros(pod_bits);
    const int64_t kmax = e->nrt_qty_pods.most[i] >> su;
    const size_t words = static_cast<size_t>((e->n_nodes + 255) / 256 + 31) / 32;
    if (out->tab_slot >= 0 || i == e->nrt_cpu_slot || kmax > spx::kNrtPkTabMaxK || (static_cast<size_t>(kmax) + 1) * words * 4 > spx::kNrtPkTabMaxBytes)
      return false;
    out->tab_slot = i, out->tab_kmax = static_cast<uint32_t>(kmax), out->tab_words = static_cast<uint32_t>(words);
    out->tab_inv_unit = std::ldexp(1.0, -su);
  }
  return true;
}

void fill_nrt(const spx_engine* e, spx::NrtArgs& na) {
  na.opts = launch_opts(e);
  na.row_ptr = e->row_indirect;
  na.n_nodes = e->n_nodes;
  na.n_pods = e->n_pods;
  na.row_stride = e->row_stride;
  na.n_res = e->nrt_n_res;
  na.strategy = e->nrt_params.strategy;
  std::memcpy(na.slot_flags, e->nrt_slot_flags, sizeof na.slot_flags);
  std::memcpy(na.slot_weight, e->nrt_slot_weight, sizeof na.slot_weight);
  na.flags = static_cast<const uint8_t*>(e->d_nrt_flags.p);
  na.max_numa = static_cast<const int32_t*>(e->d_nrt_max_numa.p);
  na.n_zones = static_cast<const uint8_t*>(e->d_nrt_nz.p);
  na.zone_id = static_cast<const uint8_t*>(e->d_nrt_zid.p);
  na.zone_present = static_cast<const uint8_t*>(e->d_nrt_zp.p);
  na.zone_avail = static_cast<const int64_t*>(e->d_nrt_avail.p);
  na.zone_cost = static_cast<const int32_t*>(e->d_nrt_cost.p);
  na.min_avg = static_cast<const float*>(e->d_nrt_minavg.p);
  na.node_present = static_cast<const uint8_t*>(e->d_nrt_np.p);
  na.qos = static_cast<const uint8_t*>(e->d_nrt_qos.p);
  na.non_native = static_cast<const uint8_t*>(e->d_nrt_nn.p);
  na.n_ctr = static_cast<const uint8_t*>(e->d_nrt_nctr.p);
  na.ctr_kind = static_cast<const uint8_t*>(e->d_nrt_ckind.p);
  na.ctr_present = static_cast<const uint8_t*>(e->d_nrt_cpres.p);
  na.ctr_req = static_cast<const int64_t*>(e->d_nrt_creq.p);
  na.pod_present = static_cast<const uint8_t*>(e->d_nrt_ppres.p);
  na.pod_req = static_cast<const int64_t*>(e->d_nrt_preq.p);
  na.fast = e->nrt_fast_slots && e->nrt_fast_nodes && e->nrt_fast_pods;
  na.cpu_slot = e->nrt_cpu_slot;
  for (int i = 0; i < SPX_NRT_MAX_RES; ++i) na.slot_weight_f[i] = static_cast<double>(e->nrt_slot_weight[i]);
  na.f_av = static_cast<const double*>(e->d_nrt_fav.p);
  na.f_rc = static_cast<const double*>(e->d_nrt_frc.p);
  na.f_rcv = static_cast<const double*>(e->d_nrt_frcv.p);
  na.f_cpu = static_cast<const double*>(e->d_nrt_fcpu.p);
  na.f_braw = static_cast<const double*>(e->d_nrt_fbraw.p);
  na.f_rep = static_cast<const uint8_t*>(e->d_nrt_frep.p);
  na.pod_items = static_cast<const uint32_t*>(e->d_nrt_items.p);
  na.perm = static_cast<const int32_t*>(e->d_nrt_perm.p);
  na.stats = static_cast<unsigned long long*>(e->d_stats.p);
  na.exact32_slots = ~(e->nrt_big_nodes | e->nrt_big_pods);
  na.pk_mode = 0, na.pk_tab_slot = -1;  // (spx_eval's NRT section turns the packed Score on)
  // inside the per-pod commit loop k_commit_apply subtracts requests from the zone table: "every quantity is a float32 value" is
  // not closed under subtraction (2^30 and 1 are, 2^30 - 1 is not) and the masks above describe the uploaded tables, so
  // BalancedAllocation's float32 "request > capacity" test gives way to the undecided -> float64 redo route there
  if (e->in_commit_loop) na.exact32_slots = 0;
  na.redo_list = static_cast<uint32_t*>(e->d_nrt_redo.p);
  na.redo_cap = e->nrt_redo_cap;
  na.ln_tab = (e->nrt_ln_ok && e->nrt_ln_built) ? static_cast<const uint32_t*>(e->d_nrt_ln.p) : nullptr;
  na.ln_const = na.ln_tab ? na.ln_tab + static_cast<size_t>(spx::make_ln_layout().rows) * static_cast<size_t>(e->n_nodes) : nullptr;
}

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

// combin.Combinations(n, k) for n = 9 .. 16 as 16-bit masks over list positions, size-major then lexicographic (the 16-bit sibling
// of nrt_combinations; 131 064 masks, built once on the host and uploaded: the 64 KB constant segment does not hold them)
struct NrtTallCombos {
  std::vector<uint16_t> mask;
  uint32_t start[8][SPX_NRT_TALL_MAX_ZONES_LEAST_NUMA + 1];
};
inline NrtTallCombos make_nrt_tall_combos() {
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

int ensure_nrt_creq(spx_engine* e, bool force = false);

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

using spx_host::kNrtFastLimit;
using spx_host::kNrtWeightLimit;
using spx_host::nrt_biased_rcp;
using spx_host::nrt_exact_f32;
using spx_host::nrt_fast_qty;
using spx_host::nrt_value_of;
using spx_host::nrt_build_classes;
using spx_host::nrt_build_items;
using spx_host::nrt_build_rank_stream;

void fill_net(const spx_engine* e, spx::NetArgs& g) {
  g.opts = launch_opts(e);
  g.row_ptr = e->row_indirect;
  g.n_nodes = e->n_nodes;
  g.row_stride = e->row_stride;
  g.n_regions = e->net_n_regions;
  g.n_zones = e->net_n_zones;
  g.n_classes = e->net_n_classes;
  g.region = static_cast<const int32_t*>(e->d_net_region.p);
  g.zone = static_cast<const int32_t*>(e->d_net_zone.p);
  g.node_class = static_cast<const int32_t*>(e->d_net_class.p);
  g.node_class16 = e->net_class16 ? static_cast<const uint16_t*>(e->d_net_class16.p) : nullptr;
  g.cls_size = static_cast<const int32_t*>(e->d_net_cls_size.p);
  g.cls_region = static_cast<const int32_t*>(e->d_net_cls_region.p);
  g.cls_zone = static_cast<const int32_t*>(e->d_net_cls_zone.p);
  if (e->net_wide_dev) {
    g.cost_wide = 1;
    g.region_cost64 = static_cast<const int64_t*>(e->d_net_rcost.p);
    g.zone_cost64 = static_cast<const int64_t*>(e->d_net_zcost.p);
  } else {
    g.region_cost = static_cast<const int32_t*>(e->d_net_rcost.p);
    g.zone_cost = static_cast<const int32_t*>(e->d_net_zcost.p);
  }
  g.pod_key = static_cast<const int32_t*>(e->d_net_pod_key.p);
  g.key_flag = static_cast<const uint8_t*>(e->d_net_key_flag.p);
  g.pair_ptr = static_cast<const int32_t*>(e->d_net_pair_ptr.p);
  g.pair_node = static_cast<const int32_t*>(e->d_net_pair_node.p);
  g.pair_max = static_cast<const int64_t*>(e->d_net_pair_max.p);
  if (e->net_dyn_active) {  // sequential commit: lists with slack that grow as pods are bound
    g.pair_ptr = static_cast<const int32_t*>(e->d_net_dyn_ptr.p);
    g.pair_end = static_cast<const int32_t*>(e->d_net_dyn_end.p);
    g.pair_node = static_cast<const int32_t*>(e->d_net_dyn_node.p);
    g.pair_max = static_cast<const int64_t*>(e->d_net_dyn_max.p);
  }
}

// NetworkOverhead: the bound of a node's accumulated cost, (largest cost entry) x (most pairs of any workload key, `extra_pairs`
// more once a batch is bound), INT64_MAX when the product does not fit int64
int64_t net_cost_bound(const spx_engine* e, int64_t extra_pairs) {
  int64_t b;
  return __builtin_mul_overflow(e->net_max_cost, std::max<int64_t>(e->net_max_pairs + extra_pairs, 1), &b) ? std::numeric_limits<int64_t>::max() : b;
}

// the 64-bit sweep (kernels_network_wide.hip) runs when the device holds int64 cost matrices or the bound reaches 2^31
bool net_wide(const spx_engine* e, int64_t extra_pairs) { return e->net_wide_dev || net_cost_bound(e, extra_pairs) >= (int64_t{1} << 31); }

// Before a NetworkOverhead launch: net_bound_check refuses a snapshot whose bound reaches 2^63 (host state alone), and net_prepare
// then widens narrow cost matrices on the device (once: they stay int64 until the next topology upload) when the bound asks for the
// 64-bit sweep.  `when`: which bound, for the message.
int net_bound_check(const spx_engine* e, int64_t extra_pairs, const char* when) {
  if (net_cost_bound(e, extra_pairs) == std::numeric_limits<int64_t>::max())
    return fail(e, SPX_ERR_ARG, std::string("NetworkOverhead: accumulated cost of a node may reach 2^63 (cost entries x dependency pairs") + when +
                                    "); the reference's own int64 sum would wrap there");
  return SPX_OK;
}
int net_prepare(spx_engine* e, int64_t extra_pairs, const char* when) {
  int rc = net_bound_check(e, extra_pairs, when);
  if (rc || e->net_wide_dev || !net_wide(e, extra_pairs)) return rc;
  if ((rc = upload(e, e->d_net_rcost, e->h_net_rcost.data(), e->h_net_rcost.size() * 8)) || (rc = upload(e, e->d_net_zcost, e->h_net_zcost.data(), e->h_net_zcost.size() * 8)))
    return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->net_wide_dev = true;
  return SPX_OK;
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
inline int64_t expand_tasks(std::vector<int32_t>& dups, int64_t n_rows) {
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

}  // namespace

// defined in spx_uploads.hip, used by the evaluation and the commit loops (not exported)
extern "C" {
__attribute__((visibility("hidden"))) int build_ln_tab(spx_engine* e);
__attribute__((visibility("hidden"))) int nrt_rank_stream(spx_engine* e, int kind);
// defined with spx_decide (spx_engine.hip), also the commit loops' per-pod step
__attribute__((visibility("hidden"))) int decide_masked(spx_engine* e, uint32_t eval_mask, uint32_t score_mask, int64_t row_begin, int64_t row_end, bool* done);
}
