// spx_engine.h — the engine's state (struct spx_engine) and the declarations of what crosses its translation units.  Not part of the
// ABI.  The entry points live in spx_engine.hip (lifecycle, options, parameters, evaluation, fetch), spx_uploads.hip (tables and
// deltas into HBM), spx_loads.hip (the one-call loaders), spx_commit.hip (the one-pod-at-a-time loops) and spx_preempt.hip (the
// preemption dry runs and loops).  A helper that two or more of them call is declared below with hidden visibility and defined once:
// spx_state.hip, spx_eval_args.hip, spx_nrt_rows.hip.  A helper with one user is not here: it sits in that unit's anonymous
// namespace.  Only functions of a line or two are inline.  The three thread-local error slots exist once (spx_engine.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "spx_internal.h"
#include "../host/nrt_streams.hpp"  // (spx_host::NrtQty, a member below)

extern thread_local std::string g_create_error;          // spx_create's failure (no engine to hold it)
extern thread_local std::string tl_err;                  // this thread's last failure ...
extern thread_local const spx_engine* tl_err_engine;     // ... and on which engine

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  bool external = false;
};

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

// d_best's four columns, [score int64 P | node int32 P | ties int32 P | feasible int32 P]
struct BestRows {
  int64_t* score;
  int32_t *node, *ties, *feasible;
};

// A function that crosses the engine's translation units and never leaves libspx.so.  Each is defined once, in the unit its group
// names; the comments on what it does stand at the definition.
#define SPX_LOCAL __attribute__((visibility("hidden")))

// a HIP call whose failure ends the calling function with SPX_ERR_HIP and the call's text as the message
#define SPX_HIP(e, call)                                                                          \
  do {                                                                                            \
    hipError_t _st = (call);                                                                      \
    if (_st != hipSuccess)                                                                        \
      return fail((e), SPX_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_st));          \
  } while (0)

namespace spx_eng {

// ---- spx_state.hip: errors, buffers, the snapshot's shape, the tables every evaluation sizes
SPX_LOCAL int fail(const spx_engine* e, int code, const std::string& msg);
SPX_LOCAL int ensure(spx_engine* e, DevBuf& b, size_t bytes);
SPX_LOCAL int upload(spx_engine* e, DevBuf& b, const void* src, size_t bytes);
SPX_LOCAL int ensure_pinned(spx_engine* e, void*& p, size_t& bytes, size_t want, size_t slack);
SPX_LOCAL int set_nodes(spx_engine* e, int64_t n);
SPX_LOCAL int set_pods(spx_engine* e, int64_t p);
SPX_LOCAL int tlp_build_order(spx_engine* e);
SPX_LOCAL int score_table_fits(const spx_engine* e, int plugin);
SPX_LOCAL int ensure_score_table(spx_engine* e, int plugin);
SPX_LOCAL BestRows best_rows(const spx_engine* e);
SPX_LOCAL int ensure_best(spx_engine* e, BestRows* out);
SPX_LOCAL int rows_evaluated(const spx_engine* e, int plugin, int64_t b, int64_t en);

// ---- spx_eval_args.hip: what the evaluation and the commit loops both do before a launch
SPX_LOCAL int alloc_check(const spx_engine* e);
SPX_LOCAL int prepare_alloc(spx_engine* e);
SPX_LOCAL uint32_t launch_opts(const spx_engine* e);
SPX_LOCAL void fill_lroc(const spx_engine* e, spx::LrocArgs& a);
SPX_LOCAL void fill_trimaran(const spx_engine* e, spx::TrimaranArgs& a);
SPX_LOCAL void fill_nrt(const spx_engine* e, spx::NrtArgs& na);
SPX_LOCAL void fill_net(const spx_engine* e, spx::NetArgs& g);
SPX_LOCAL int64_t net_cost_bound(const spx_engine* e, int64_t extra_pairs);
SPX_LOCAL int net_bound_check(const spx_engine* e, int64_t extra_pairs, const char* when);
SPX_LOCAL int net_prepare(spx_engine* e, int64_t extra_pairs, const char* when);

// ---- spx_nrt_rows.hip: NodeResourceTopologyMatch's launches beside the dense sweep
SPX_LOCAL int launch_nrt_long_rows(spx_engine* e, const spx::NrtArgs& na, int64_t row_begin, int64_t row_end);
SPX_LOCAL int nrt_tall_ready(const spx_engine* e);
SPX_LOCAL int launch_nrt_tall_rows(spx_engine* e, const spx::NrtArgs& na, int64_t row_begin, int64_t row_end);
SPX_LOCAL int launch_nrt_wide_rows(spx_engine* e, int64_t row_begin, int64_t row_end, int64_t* out_raw);
SPX_LOCAL int ensure_nrt_creq(spx_engine* e, bool force = false);

// something other than the unmasked broadcast wrote (or may have written) into Allocatable's score table, or the buffer changed
inline void alloc_table_dirty(spx_engine* e) { e->alloc_kept = spx_engine::AllocKept{}; }

inline bool forced_reference(const spx_engine* e, int plugin) { return (e->option[SPX_OPT_REFERENCE_KERNELS] >> plugin) & 1; }

inline bool lroc_exact53(const spx_engine* e) {
  return e->lroc_nodes_exact && e->lroc_pods_exact && e->lv_alloc_exact && !forced_reference(e, SPX_PLUGIN_LROC);
}
// the float32 sweep (k_lroc_fast) may run: exact columns, below 2^47, every limit at least its request (SetMaxLimits, resourcestats.go:227-231)
inline bool lroc_f32_ok(const spx_engine* e) {
  return lroc_exact53(e) && e->lroc_nodes_f32 && e->lroc_pods_f32 && e->lv_alloc_f32 && !e->option[SPX_OPT_LROC_FLOAT64];
}

// the 64-bit sweep (kernels_network_wide.hip) runs when the device holds int64 cost matrices or the bound reaches 2^31
inline bool net_wide(const spx_engine* e, int64_t extra_pairs) { return e->net_wide_dev || net_cost_bound(e, extra_pairs) >= (int64_t{1} << 31); }

}  // namespace spx_eng

using namespace spx_eng;  // (the call sites say fail, ensure, upload, ...)

extern "C" {
// ---- spx_uploads.hip: derived NRT tables the evaluation and the commit loops ask for
SPX_LOCAL int build_ln_tab(spx_engine* e);
SPX_LOCAL int nrt_rank_stream(spx_engine* e, int kind);
// ---- spx_engine.hip: defined with spx_decide, also the commit loops' per-pod step
SPX_LOCAL int decide_masked(spx_engine* e, uint32_t eval_mask, uint32_t score_mask, int64_t row_begin, int64_t row_end, bool* done);
}
