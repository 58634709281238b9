// spx_engine.hip — the C-ABI engine of libspx.so: lifecycle, options and parameters, the evaluation (spx_eval, spx_decide, spx_eval_best)
// and the fetch calls.  Tables and deltas into HBM: spx_uploads.hip; the one-call loaders: spx_loads.hip; the one-pod-at-a-time loops:
// spx_commit.hip; the preemption runs: spx_preempt.hip.  State and what crosses the units: spx_engine.h (defined in spx_state.hip,
// spx_eval_args.hip, spx_nrt_rows.hip); the helpers only this file calls open it, in the first namespace below.  See include/spx.h
// for the contract.
//
// There is deliberately no CPU fallback: spx_create() fails with SPX_ERR_NOGPU when no HIP device
// is usable, and every compute entry point needs an engine.
#include "spx_engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

thread_local std::string g_create_error;
thread_local std::string tl_err;
thread_local const spx_engine* tl_err_engine = nullptr;

// ---- this file's own helpers: the plugin sets, the bound-table checks, the argument builders and the packed Score's preconditions
namespace {

constexpr uint32_t kFilterPlugins = (1u << SPX_PLUGIN_NRT) | (1u << SPX_PLUGIN_NETOVERHEAD);
// plugins whose NormalizeScore depends on the feasible set of the cycle
constexpr uint32_t kNormalizingPlugins =
    (1u << SPX_PLUGIN_ALLOCATABLE) | (1u << SPX_PLUGIN_NETOVERHEAD) | (1u << SPX_PLUGIN_PEAKS) | (1u << SPX_PLUGIN_SYSCHED) | (1u << SPX_PLUGIN_NODEMETA) |
    (1u << SPX_PLUGIN_PODSTATE);
// plugins that own a uint8 score table
constexpr bool plugin_has_score(int k) {
  return k <= SPX_PLUGIN_NETOVERHEAD || k == SPX_PLUGIN_LROC || k == SPX_PLUGIN_PEAKS || k == SPX_PLUGIN_SYSCHED || k == SPX_PLUGIN_NODEMETA || k == SPX_PLUGIN_PODSTATE;
}

// The checks of a plugin's tables that write nothing (spx_eval makes them all before its first allocation): a table the caller bound
// must hold n_pods x row_stride (a score table: score_table_fits, spx_state.hip) ...
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

int ensure_status_table(spx_engine* e, int plugin) {
  DevBuf& b = e->status[plugin];
  if (b.external) return status_table_fits(e, plugin);
  return ensure(e, b, static_cast<size_t>(e->n_pods) * static_cast<size_t>(e->row_stride));
}

// The status tables that narrow a pod's node list when `mask` is evaluated or summed: {NRT's, NetworkOverhead's, the caller's mask},
// NULL = not in play (the layout of ProfileArgs.status and the scorers' other_status; NetworkOverhead's own sweep takes [0] and [2])
void feasibility_status(const spx_engine* e, uint32_t mask, const uint8_t* out[3]) {
  out[0] = (mask & (1u << SPX_PLUGIN_NRT)) ? static_cast<const uint8_t*>(e->status[SPX_PLUGIN_NRT].p) : nullptr;
  out[1] = (mask & (1u << SPX_PLUGIN_NETOVERHEAD)) ? static_cast<const uint8_t*>(e->status[SPX_PLUGIN_NETOVERHEAD].p) : nullptr;
  out[2] = e->ext_mask ? static_cast<const uint8_t*>(e->d_ext_status.p) : nullptr;
}

// What one evaluation is asked for besides its mask and rows (spx_decide's preparatory sweeps; spx_eval itself passes the defaults)
struct EvalCall {
  bool hold_ev0 = false;           // the caller has recorded ev0 and times this evaluation together with its own sweep
  bool skip_alloc_masked = false;  // the caller folds Allocatable's masked normalisation into its argmax kernel: the table is not written
};

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

}  // namespace

extern "C" {

int spx_abi_version(void) { return 1; }

const char* spx_last_error(const spx_engine* e) {
  if (!e) return g_create_error.c_str();
  if (tl_err_engine != e) {  // this thread has not failed on this engine: hand out a private copy of the engine's last message
    std::lock_guard<std::mutex> g(e->err_mu);
    tl_err = e->err;
    tl_err_engine = e;
  }
  return tl_err.c_str();
}

int spx_create(int device_id, spx_engine** out) {
  if (!out) return fail(nullptr, SPX_ERR_ARG, "out is NULL");
  *out = nullptr;
  int count = 0;
  hipError_t st = hipGetDeviceCount(&count);
  if (st != hipSuccess || count <= 0)
    return fail(nullptr, SPX_ERR_NOGPU, std::string("no HIP device available (") + hipGetErrorString(st) +
                                            "); libspx has no CPU fallback");
  if (device_id < 0 || device_id >= count) return fail(nullptr, SPX_ERR_ARG, "device_id out of range");
  spx_engine* e = new spx_engine();
  e->device = device_id;
  // ev0 / ev1 only time (spx_last_eval_ms, spx_multi's per-rank figures): nothing is read on the strength of them, so their packets carry
  // no system-scope fence — of the 0.0074 ms that the two packets between two sweeps cost the headline step, 0.0030 is the fences'
  // (tools/micro/evgap.hip, profiles/tlp_pairs/tlp_pairs_ab.md)
  if ((st = hipSetDevice(device_id)) != hipSuccess || (st = hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking)) != hipSuccess ||
      (st = hipEventCreateWithFlags(&e->ev0, hipEventDisableSystemFence)) != hipSuccess ||
      (st = hipEventCreateWithFlags(&e->ev1, hipEventDisableSystemFence)) != hipSuccess) {
    std::string msg = std::string("engine init: ") + hipGetErrorString(st);
    delete e;
    return fail(nullptr, SPX_ERR_HIP, msg);
  }
  e->stream = e->own_stream;
  if ((st = hipMalloc(&e->d_stats.p, spx::kStatBytes)) != hipSuccess || (st = hipMemset(e->d_stats.p, 0, spx::kStatBytes)) != hipSuccess) {
    std::string msg = std::string("engine init: ") + hipGetErrorString(st);
    delete e;
    return fail(nullptr, SPX_ERR_HIP, msg);
  }
  e->d_stats.bytes = spx::kStatBytes;
  *out = e;
  return SPX_OK;
}

int spx_destroy(spx_engine* e) {
  if (!e) return SPX_OK;
  (void)hipSetDevice(e->device);
  (void)hipStreamSynchronize(e->stream);
  DevBuf* bufs[] = {&e->d_alloc,   &e->d_alloc_w,  &e->d_alloc_raw, &e->d_alloc_norm, &e->d_alloc_rel, &e->d_alloc_prev, &e->d_cap_cpu, &e->d_tlp_util,
                    &e->d_tlp_missing, &e->d_tlp_valid, &e->d_lv_acpu, &e->d_lv_amem, &e->d_lv_cavg, &e->d_lv_cstd,
                    &e->d_lv_mavg, &e->d_lv_mstd,  &e->d_lv_flags,  &e->d_tlp_pod,    &e->d_lv_rcpu, &e->d_lv_rmem,
                    &e->d_raw_row,   &e->d_lv_exact, &e->d_lv_fast, &e->d_tlp_fast, &e->d_tlp_amb, &e->d_tlp_order, &e->d_tlp_order_scratch, &e->d_lv_amb, &e->d_nrt_pk_tab, &e->d_commit, &e->d_nrt_flags, &e->d_nrt_max_numa, &e->d_nrt_nz, &e->d_nrt_zid, &e->d_nrt_zp,
                    &e->d_nrt_avail, &e->d_nrt_cost,  &e->d_nrt_minavg, &e->d_nrt_np,    &e->d_nrt_qos, &e->d_nrt_nn,
                    &e->d_nrt_nctr,  &e->d_nrt_ckind, &e->d_nrt_cpres,  &e->d_nrt_creq,  &e->d_nrt_ppres, &e->d_nrt_preq,
                    &e->d_nrt_frcv, &e->d_nrt_fav,   &e->d_nrt_frc,   &e->d_nrt_fcpu,   &e->d_nrt_frep,  &e->d_nrt_items, &e->d_nrt_perm, &e->d_nrt_ln, &e->d_nrt_fbraw, &e->d_nrt_redo,
                    &e->d_net_region, &e->d_net_zone, &e->d_net_class, &e->d_net_class16, &e->d_net_cls_size, &e->d_net_cls_region, &e->d_net_cls_zone,
                    &e->d_net_rcost, &e->d_net_zcost, &e->d_net_pod_key, &e->d_net_key_flag, &e->d_net_pair_ptr,
                    &e->d_net_pair_node, &e->d_net_pair_max, &e->d_q_pod_ns, &e->d_q_pod_prio, &e->d_q_pod_req, &e->d_q_pod_reqp,
                    &e->d_q_has, &e->d_q_used, &e->d_q_max, &e->d_q_maxp, &e->d_q_other, &e->d_q_otherp, &e->d_q_nom_ptr,
                    &e->d_q_nom_prio, &e->d_q_nom_idx, &e->d_q_nom_req, &e->d_q_nom_reqp, &e->d_q_status, &e->d_ext_status,
                    &e->d_q_usedp, &e->d_q_min, &e->d_q_minp, &e->d_q_agg, &e->d_net_eff_ptr, &e->d_net_eff_key, &e->d_net_eff_cost, &e->d_net_dyn_ptr,
                    &e->d_net_dyn_end, &e->d_net_dyn_node, &e->d_net_dyn_max, &e->d_commit_save, &e->d_row_counter, &e->d_coop_sync, &e->d_coop_node, &e->d_coop_max,
                    &e->d_sort_prio, &e->d_sort_ts, &e->d_sort_group, &e->d_sort_topo, &e->d_sort_scratch,
                    &e->d_qos_prio, &e->d_qos_cls, &e->d_qos_ts, &e->d_qos_key, &e->d_qos_none, &e->d_qos_zero, &e->d_qos_rank, &e->d_qos_scratch, &e->d_nm_raw, &e->d_ps_raw, &e->d_ncol_row,
                    &e->d_best, &e->d_stats, &e->d_decide, &e->d_lroc_nreq_c, &e->d_lroc_nreq_m, &e->d_lroc_nlim_c, &e->d_lroc_nlim_m,
                    &e->d_lroc_preq_c, &e->d_lroc_preq_m, &e->d_lroc_plim_c, &e->d_lroc_plim_m, &e->d_lroc_tab, &e->d_lroc_podf,
                    &e->d_pk_cap, &e->d_pk_util, &e->d_pk_valid, &e->d_pk_k1, &e->d_pk_k2, &e->d_pk_pod, &e->d_pk_min, &e->d_pk_max, &e->d_pk_rowc, &e->d_pk_tab, &e->d_pk_seg, &e->d_pk_segn,
                    &e->d_nrt_uniq, &e->d_nrt_dups, &e->d_pk_uniq, &e->d_pk_dups, &e->d_delta, &e->d_nrt_lnrec, &e->d_net_pair_node2, &e->d_net_pair_max2, &e->d_nrt_rk, &e->d_nrt_rk_off, &e->d_nrt_rk_first, &e->d_nrt_fz, &e->d_nrt_wsort, &e->d_nrt_wrank,
                    &e->d_nrtl_row, &e->d_nrtl_ptr, &e->d_nrtl_kind, &e->d_nrtl_pres, &e->d_nrtl_req, &e->d_nrtl_map,
                    &e->d_nrtw_sflags, &e->d_nrtw_sweight, &e->d_nrtw_flags, &e->d_nrtw_max_numa, &e->d_nrtw_nz, &e->d_nrtw_zid, &e->d_nrtw_zp,
                    &e->d_nrtw_avail, &e->d_nrtw_cost, &e->d_nrtw_minavg, &e->d_nrtw_np, &e->d_nrtw_qos, &e->d_nrtw_nn, &e->d_nrtw_rptr,
                    &e->d_nrtw_rslot, &e->d_nrtw_rqty, &e->d_nrtw_cptr, &e->d_nrtw_ckind, &e->d_nrtw_eptr, &e->d_nrtw_eslot, &e->d_nrtw_eqty,
                    &e->d_sy_host, &e->d_sy_present, &e->d_sy_k, &e->d_sy_a, &e->d_sy_sptr, &e->d_sy_sbit, &e->d_sy_scnt, &e->d_sy_sets, &e->d_sy_empty,
                    &e->d_sy_pod_set, &e->d_sy_order, &e->d_sy_first, &e->d_sy_dups, &e->d_sy_raw, &e->d_sy_max,
                    &e->d_cs_left, &e->d_cs_present, &e->d_cs_prefix, &e->d_cs_smax, &e->d_cs_stotal, &e->d_cs_any, &e->d_cs_req, &e->d_cs_mask, &e->d_cs_sptr,
                    &e->d_cs_snode, &e->d_cs_scum, &e->d_cs_walk, &e->d_cs_pass, &e->d_cs_open, &e->d_cs_gap, &e->d_cs_exists, &e->d_cs_minm, &e->d_cs_hasres,
                    &e->d_cs_backoff, &e->d_cs_permit, &e->d_cs_listed, &e->d_cs_gated, &e->d_cs_pod_group, &e->d_cs_status,
                    &e->d_pre_nodes, &e->d_pre_podrec, &e->d_pre_noms, &e->d_pre_pdb_allowed, &e->d_pre_pod_fit, &e->d_pre_rows, &e->d_pre_mask, &e->d_pre_rec, &e->d_pre_cells,
                    &e->d_pre_pick, &e->d_pre_one, &e->d_ptol_pods, &e->d_ptol_meta, &e->d_ptol_rec, &e->d_pseq, &e->d_pseq_nom,
                    &e->d_pnrt_nodes, &e->d_pnrt_contrib, &e->d_pnrt_rel_ptr, &e->d_pnrt_rel, &e->d_pnrt_pods, &e->d_pnrt_rec};
  for (DevBuf* b : bufs)
    if (b->p && !b->external) (void)hipFree(b->p);
  for (int i = 0; i < SPX_NUM_PLUGINS; ++i) {
    if (e->score[i].p && !e->score[i].external) (void)hipFree(e->score[i].p);
    if (e->status[i].p && !e->status[i].external) (void)hipFree(e->status[i].p);
  }
  if (e->ev0) (void)hipEventDestroy(e->ev0);
  if (e->ev1) (void)hipEventDestroy(e->ev1);
  if (e->h_best) (void)hipHostFree(e->h_best);
  if (e->h_stage) (void)hipHostFree(e->h_stage);
  if (e->h_items) (void)hipHostFree(e->h_items);
  if (e->h_sort_hist) (void)hipHostFree(e->h_sort_hist);
  if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
  delete e;
  return SPX_OK;
}

int spx_set_stream(spx_engine* e, void* hip_stream) {
  if (!e) return SPX_ERR_ARG;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  e->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->own_stream;
  return SPX_OK;
}

int spx_get_stream(spx_engine* e, void** hip_stream) {
  if (!e || !hip_stream) return SPX_ERR_ARG;
  *hip_stream = static_cast<void*>(e->stream);
  return SPX_OK;
}

int spx_set_option(spx_engine* e, int option, int64_t value) {
  if (!e) return SPX_ERR_ARG;
  switch (option) {
    case SPX_OPT_ROW_ALIGN:
      if (value < spx::kRowAlign || value % spx::kRowAlign || value > 4096) return fail(e, SPX_ERR_ARG, "SPX_OPT_ROW_ALIGN: a multiple of 16 in [16, 4096]");
      if (e->n_nodes != -1) return fail(e, SPX_ERR_STATE, "SPX_OPT_ROW_ALIGN must be set before the first table upload");
      break;
    case SPX_OPT_REFERENCE_KERNELS:
      if (value < 0 || value >= (int64_t{1} << SPX_NUM_PLUGINS)) return fail(e, SPX_ERR_ARG, "SPX_OPT_REFERENCE_KERNELS: a mask of plugin ids");
      if (((value ^ e->option[option]) >> SPX_PLUGIN_LROC) & 1) e->lroc_tab_ready = false;
      break;
    case SPX_OPT_LROC_FLOAT64:
    case SPX_OPT_DECIDE_UNFUSED:
    case SPX_OPT_NRT_SINGLE_LAUNCH:
    case SPX_OPT_COMMIT_FROM_MEMORY:
    case SPX_OPT_NRT_POD_CLASSES:
    case SPX_OPT_PEAKS_POD_CLASSES:
    case SPX_OPT_COMMIT_COOP:
    case SPX_OPT_NRT_RANK_FILTER:
    case SPX_OPT_ROW_WORKGROUP:
    case SPX_OPT_TLP_AMB_TABLE:
    case SPX_OPT_NRT_PACKED_SCORE:
    case SPX_OPT_NET_ALLOC_FUSED:
    case SPX_OPT_NRT_RANK_NARROW:
    case SPX_OPT_NRT_FUSED:
    case SPX_OPT_NRT_WIDE:
    case SPX_OPT_ALLOC_TABLE_KEEP:
    case SPX_OPT_TLP_CHUNK_SCHED:
      if (value != 0 && value != 1) return fail(e, SPX_ERR_ARG, "option takes 0 or 1");
      break;
    case SPX_OPT_TLP_POD_CLASSES:
      if (value < 0 || value > 2) return fail(e, SPX_ERR_ARG, "SPX_OPT_TLP_POD_CLASSES: 0, 1 or 2");
      break;
    case SPX_OPT_NRT_LN_LIST_PERMILLE:
      if (value < 1 || value > 1000) return fail(e, SPX_ERR_ARG, "SPX_OPT_NRT_LN_LIST_PERMILLE: 1..1000");
      break;
    case SPX_OPT_PEAKS_ESTIMATE:
      if (value != 0 && value != 1 && value != 8) return fail(e, SPX_ERR_ARG, "SPX_OPT_PEAKS_ESTIMATE: 0, 1 or 8");
      break;
    case SPX_OPT_PEAKS_TILE:
      if (value != 44 && value != 84 && value != 48 && value != 88) return fail(e, SPX_ERR_ARG, "SPX_OPT_PEAKS_TILE: 44, 84, 48 or 88");
      break;
    default:
      return fail(e, SPX_ERR_ARG, "unknown option");
  }
  e->option[option] = value;
  return SPX_OK;
}

int spx_nrt_pod_classes(const spx_engine* e, int64_t* n_unique, int64_t* n_copies) {
  if (!e || !n_unique || !n_copies) return SPX_ERR_ARG;
  *n_copies = e->nrt_pods ? e->nrt_n_dups : 0;
  *n_unique = e->nrt_pods ? e->n_pods - *n_copies : 0;
  return SPX_OK;
}

int spx_peaks_pod_classes(const spx_engine* e, int64_t* n_unique, int64_t* n_copies) {
  if (!e || !n_unique || !n_copies) return SPX_ERR_ARG;
  *n_copies = e->peaks_pods ? e->pk_n_dups : 0;
  *n_unique = e->peaks_pods ? e->n_pods - *n_copies : 0;
  return SPX_OK;
}

int spx_sysched_pod_classes(const spx_engine* e, int64_t* n_unique, int64_t* n_copies) {
  if (!e || !n_unique || !n_copies) return SPX_ERR_ARG;
  *n_copies = e->sy_pods ? e->sy_n_dups : 0;
  *n_unique = e->sy_pods ? e->n_pods - *n_copies : 0;
  return SPX_OK;
}

int spx_get_option(const spx_engine* e, int option, int64_t* value) {
  if (!e || !value || option < 0 || option >= SPX_NUM_OPTIONS) return SPX_ERR_ARG;
  *value = e->option[option];
  return SPX_OK;
}

int spx_set_allocatable_params(spx_engine* e, const spx_allocatable_params* p) {
  if (!e || !p) return SPX_ERR_ARG;
  if (p->mode != SPX_MODE_LEAST && p->mode != SPX_MODE_MOST) return fail(e, SPX_ERR_ARG, "invalid mode");
  if (p->n_res <= 0) return fail(e, SPX_ERR_ARG, "n_res must be positive");
  for (int32_t r = 0; r < p->n_res; ++r) {
    if (p->weight[r] <= 0) {  // validateResources allocatable.go:53-61
      char buf[160];
      std::snprintf(buf, sizeof buf, "resource Weight of %d should be a positive value, got %lld", p->res[r],
                    static_cast<long long>(p->weight[r]));
      return fail(e, SPX_ERR_ARG, buf);
    }
  }
  e->alloc_mode = p->mode;
  e->alloc_res.assign(p->res, p->res + p->n_res);
  e->alloc_weight.assign(p->weight, p->weight + p->n_res);
  e->alloc_ready = false;
  return SPX_OK;
}

int spx_set_tlp_params(spx_engine* e, const spx_tlp_params* p) {
  if (!e || !p) return SPX_ERR_ARG;
  e->tlp = *p;
  e->tlp_amb_built = false;  // the table depends on the target utilisation
  return SPX_OK;
}

int spx_set_lvrb_params(spx_engine* e, const spx_lvrb_params* p) {
  if (!e || !p) return SPX_ERR_ARG;
  e->lvrb = *p;
  e->lv_amb_built = false;  // sigma (margin, sensitivity) is inside the per-node constants and the table
  return SPX_OK;
}

int spx_set_plugin_weights(spx_engine* e, const int64_t* weights) {
  if (!e || !weights) return SPX_ERR_ARG;
  // the argmax sums weight x byte (<= 255) over the score tables in int64 (k_best): weights whose totals could leave it are refused
  unsigned __int128 bound = 0;
  for (int k = 0; k < SPX_NUM_PLUGINS; ++k)
    if (plugin_has_score(k)) bound += static_cast<unsigned __int128>(weights[k] < 0 ? 0 - static_cast<uint64_t>(weights[k]) : static_cast<uint64_t>(weights[k])) * 255u;
  if (bound > static_cast<unsigned __int128>(std::numeric_limits<int64_t>::max()))
    return fail(e, SPX_ERR_ARG, "plugin weights: sum of |weight| * 255 over the scoring plugins exceeds int64 (a weighted total could overflow)");
  std::memcpy(e->plugin_weight, weights, sizeof e->plugin_weight);
  return SPX_OK;
}

}  // extern "C"

// ---- spx_eval: eval_rows checks the call (eval_check), readies the tables and the scratch (prepare_*), and issues the launches
// between ev0 and ev1 (launch_*), one function per plugin.  Nothing is allocated, launched or written before eval_check has passed.
namespace {

// the plugins of one evaluation's mask
struct EvalPlugins {
  uint32_t mask;
  bool alloc, tlp, lvrb, nrt, net, quota, lroc, peaks, sysched, cosched, nodemeta, podstate;
  bool masked;  // Allocatable's (NodeMetadata's, PodState's) NormalizeScore runs over each pod's feasible nodes as soon as any Filter is in play
};

EvalPlugins eval_plugins(const spx_engine* e, uint32_t mask) {
  auto has = [mask](int plugin) { return ((mask >> plugin) & 1u) != 0; };
  const bool nrt = has(SPX_PLUGIN_NRT), net = has(SPX_PLUGIN_NETOVERHEAD);
  return EvalPlugins{mask, has(SPX_PLUGIN_ALLOCATABLE), has(SPX_PLUGIN_TLP), has(SPX_PLUGIN_LVRB), nrt, net, has(SPX_PLUGIN_CAPACITY), has(SPX_PLUGIN_LROC),
                     has(SPX_PLUGIN_PEAKS), has(SPX_PLUGIN_SYSCHED), has(SPX_PLUGIN_COSCHED), has(SPX_PLUGIN_NODEMETA), has(SPX_PLUGIN_PODSTATE),
                     nrt || net || e->ext_mask};
}

// Every SPX_ERR_ARG / SPX_ERR_STATE answer of an evaluation, from host state alone: a call refused here has allocated nothing,
// launched nothing and written no engine field.  The order is the order in which a call with several faults names them.
int eval_check(const spx_engine* e, const EvalPlugins& f, int64_t row_begin, int64_t row_end) {
  const uint32_t known = (1u << SPX_PLUGIN_ALLOCATABLE) | (1u << SPX_PLUGIN_TLP) | (1u << SPX_PLUGIN_LVRB) | (1u << SPX_PLUGIN_NRT) |
                         (1u << SPX_PLUGIN_NETOVERHEAD) | (1u << SPX_PLUGIN_CAPACITY) | (1u << SPX_PLUGIN_LROC) | (1u << SPX_PLUGIN_PEAKS) |
                         (1u << SPX_PLUGIN_SYSCHED) | (1u << SPX_PLUGIN_COSCHED) | (1u << SPX_PLUGIN_NODEMETA) | (1u << SPX_PLUGIN_PODSTATE);
  if (f.mask == 0 || (f.mask & ~known)) return fail(e, SPX_ERR_ARG, "plugin mask has unsupported bits");
  if (f.lroc && !(e->tri_nodes && e->lroc_nodes && e->lroc_pods)) return fail(e, SPX_ERR_STATE, "LowRiskOverCommitment node/pod tables not uploaded");
  if (f.peaks && !(e->peaks_nodes && e->peaks_pods)) return fail(e, SPX_ERR_STATE, "Peaks node/pod tables not uploaded");
  if (f.sysched && !(e->sy_nodes && e->sy_pods)) return fail(e, SPX_ERR_STATE, "SySched node/pod tables not uploaded");
  if (f.sysched && e->sy_node_words != e->sy_pod_words) return fail(e, SPX_ERR_STATE, "SySched: the node and pod tables differ in n_words");
  if (f.sysched && e->row_indirect) return fail(e, SPX_ERR_STATE, "SySched is not part of the sequential commit loop");
  if (f.nodemeta && !e->nm_nodes) return fail(e, SPX_ERR_STATE, "NodeMetadata node column not uploaded");
  if (f.podstate && !e->ps_nodes) return fail(e, SPX_ERR_STATE, "PodState node column not uploaded");
  if (f.nodemeta && e->row_indirect) return fail(e, SPX_ERR_STATE, "NodeMetadata is not part of the sequential commit loop");
  if (f.podstate && e->row_indirect) return fail(e, SPX_ERR_STATE, "PodState is not part of the sequential commit loop");
  if (f.cosched && !e->cosched) return fail(e, SPX_ERR_STATE, "Coscheduling tables not uploaded");
  if (f.cosched && e->row_indirect) return fail(e, SPX_ERR_STATE, "Coscheduling is not part of the sequential commit loop");
  if (f.quota && !e->quota) return fail(e, SPX_ERR_STATE, "CapacityScheduling quota tables not uploaded");
  if (e->n_nodes <= 0 && f.mask != (1u << SPX_PLUGIN_CAPACITY)) return fail(e, SPX_ERR_STATE, "no node table uploaded");
  if ((f.tlp || f.lvrb) && !(e->tri_nodes && e->tri_pods)) return fail(e, SPX_ERR_STATE, "trimaran node/pod tables not uploaded");
  if (e->n_pods <= 0) {
    if (f.tlp || f.lvrb) return fail(e, SPX_ERR_STATE, "no pod table uploaded");
    return fail(e, SPX_ERR_STATE, "n_pods unknown: upload a pod table first");
  }
  if (row_begin < 0 || row_end > e->n_pods || row_begin > row_end) return fail(e, SPX_ERR_ARG, "row range out of bounds");
  int rc;
  if (f.nrt && e->nrt_wide && !(e->nrtw_slots && e->nrtw_nodes && e->nrtw_pods)) return fail(e, SPX_ERR_STATE, "NRT wide slot/node/pod tables not uploaded");
  if (f.nrt && !e->nrt_wide && !(e->nrt_slots && e->nrt_nodes && e->nrt_pods)) return fail(e, SPX_ERR_STATE, "NRT slot/node/pod tables not uploaded");
  if (f.nrt && !e->nrt_wide && !e->nrt_long_ok)
    return fail(e, SPX_ERR_STATE, "NRT: the pod batch has pods with more than 8 containers: call spx_upload_nrt_long_pods after spx_upload_nrt_pods");
  if (f.nrt && !e->nrt_wide && (rc = nrt_tall_ready(e))) return rc;
  if (f.alloc && (rc = alloc_check(e))) return rc;
  if (f.net && !(e->net_nodes && e->net_topo && e->net_pods)) return fail(e, SPX_ERR_STATE, "NetworkOverhead node/topology/pod tables not uploaded");
  // the reference accumulates a node's cost in int64 (networkoverhead.go:605-633); the narrow sweeps add in int32 and keep the Filter
  // verdict in the sign bit, which is exact as long as (largest cost entry) x (most pairs of any workload) stays below 2^31; from
  // there on the 64-bit sweep runs (kernels_network_wide.hip), up to the 2^63 at which the reference's own sum could wrap
  if (f.net && (rc = net_bound_check(e, 0, ""))) return rc;
  // tables the caller bound: large enough, and (all of them share row_stride when engine-owned) with the engine's row stride
  for (int p = 0; p < 5; ++p)
    if ((f.mask & (1u << p)) && (rc = score_table_fits(e, p))) return rc;
  if (f.lroc && ((rc = score_table_fits(e, SPX_PLUGIN_LROC)) || (rc = score_table_stride(e, SPX_PLUGIN_LROC)))) return rc;
  if (f.peaks && ((rc = score_table_fits(e, SPX_PLUGIN_PEAKS)) || (rc = score_table_stride(e, SPX_PLUGIN_PEAKS)))) return rc;
  if (f.nrt && (rc = status_table_fits(e, SPX_PLUGIN_NRT))) return rc;
  if (f.net && (rc = status_table_fits(e, SPX_PLUGIN_NETOVERHEAD))) return rc;
  if (f.sysched && ((rc = score_table_fits(e, SPX_PLUGIN_SYSCHED)) || (rc = score_table_stride(e, SPX_PLUGIN_SYSCHED)))) return rc;
  if (f.nodemeta && ((rc = score_table_fits(e, SPX_PLUGIN_NODEMETA)) || (rc = score_table_stride(e, SPX_PLUGIN_NODEMETA)))) return rc;
  if (f.podstate && ((rc = score_table_fits(e, SPX_PLUGIN_PODSTATE)) || (rc = score_table_stride(e, SPX_PLUGIN_PODSTATE)))) return rc;
  for (int p = 0; p < 3; ++p)
    if ((f.mask & (1u << p)) && (rc = score_table_stride(e, p))) return rc;
  if (f.nrt && (rc = score_table_stride(e, SPX_PLUGIN_NRT))) return rc;
  if (f.nrt && e->nrt_wide && e->row_indirect)
    return fail(e, SPX_ERR_STATE, "NRT: the sequential commit loop does not take a wide snapshot (more than 8 resource slots)");
  if (f.net && (rc = score_table_stride(e, SPX_PLUGIN_NETOVERHEAD))) return rc;
  if (f.lroc && e->lroc_loop_form >= 0 && row_end - row_begin != 1)
    return fail(e, SPX_ERR_STATE, "internal: the commit loop evaluates LowRiskOverCommitment one row at a time");
  if (f.peaks && e->peaks_loop_row && row_end - row_begin != 1) return fail(e, SPX_ERR_STATE, "internal: the commit loop evaluates Peaks one row at a time");
  return SPX_OK;
}

// ---- preparation: what has to exist before ev0
int prepare_tables(spx_engine* e, const EvalPlugins& f) {
  int rc;
  if (f.alloc && (rc = prepare_alloc(e))) return rc;
  if (f.net && (rc = net_prepare(e, 0, ""))) return rc;
  for (int p = 0; p < SPX_NUM_PLUGINS; ++p)
    if ((f.mask & (1u << p)) && plugin_has_score(p) && (rc = ensure_score_table(e, p))) return rc;
  if (f.nrt && (rc = ensure_status_table(e, SPX_PLUGIN_NRT))) return rc;
  if (f.net && (rc = ensure_status_table(e, SPX_PLUGIN_NETOVERHEAD))) return rc;
  return SPX_OK;
}

int prepare_lroc(spx_engine* e) { return ensure(e, e->d_lroc_tab, static_cast<size_t>(e->row_stride) * spx::kLrocTabCols * sizeof(double)); }

int prepare_peaks(spx_engine* e) {
  int rc;
  if ((rc = ensure(e, e->d_pk_min, static_cast<size_t>(e->n_pods) * 8)) || (rc = ensure(e, e->d_pk_max, static_cast<size_t>(e->n_pods) * 8)) ||
      (rc = ensure(e, e->d_pk_rowc, static_cast<size_t>(e->n_pods) * 16)) || (rc = ensure(e, e->d_pk_tab, static_cast<size_t>(e->row_stride) * 96)))
    return rc;
  return SPX_OK;
}

// SySched's raw table: as many distinct sets per chunk as the scratch budget holds (and a launch's grid takes)
int prepare_sysched(spx_engine* e, int64_t* per_chunk) {
  const size_t row_bytes = static_cast<size_t>(e->row_stride) * sizeof(int32_t);
  *per_chunk = std::min<int64_t>(std::max<int64_t>(1, static_cast<int64_t>(spx::kSyschedRawBudget / row_bytes)), spx::kSyschedMaxChunkSets);
  int rc;
  if ((rc = ensure(e, e->d_sy_raw, static_cast<size_t>(std::min<int64_t>(*per_chunk, e->sy_n_sets)) * row_bytes)) ||
      (rc = ensure(e, e->d_sy_max, static_cast<size_t>(e->sy_n_sets) * sizeof(int32_t))))
    return rc;
  return SPX_OK;
}

// the trimaran launch (Allocatable's unmasked broadcast, TLP, LVRB) and what becomes of Allocatable's table in this evaluation
struct TrimaranStep {
  spx::TrimaranArgs a{};
  bool alloc_keepable = false;  // the unmasked broadcast goes into an engine-owned table, by a host-side row range
  bool alloc_kept_now = false;  // ... and these rows already hold it (SPX_OPT_ALLOC_TABLE_KEEP): the sweep leaves Allocatable's stores out
};

// TargetLoadPacking's float32 node constants and ambiguity table, for spx_eval's sweep and spx_decide's fused one
int tlp_scratch(spx_engine* e, spx::TrimaranArgs& a) {
  int rc;
  if ((rc = ensure(e, e->d_tlp_fast, static_cast<size_t>(spx::round_up(e->row_stride, 1024)) * 4 * sizeof(float)))) return rc;
  a.tlp_fast = static_cast<float*>(e->d_tlp_fast.p);
  if (!e->d_tlp_amb.p) e->tlp_amb_built = false;
  if ((rc = ensure(e, e->d_tlp_amb, static_cast<size_t>(spx::kTlpAmbSize) * 4))) return rc;
  a.tlp_amb = static_cast<uint32_t*>(e->d_tlp_amb.p);
  a.tlp_amb_size = spx::kTlpAmbSize;
  a.tlp_amb_built = &e->tlp_amb_built;
  a.tlp_amb_geom = e->tlp_amb_geom;
  return SPX_OK;
}

int prepare_trimaran(spx_engine* e, const EvalPlugins& f, const EvalCall& call, int64_t row_begin, int64_t row_end, TrimaranStep* t) {
  spx::TrimaranArgs& a = t->a;
  fill_trimaran(e, a);
  a.row_begin = row_begin;
  a.row_end = row_end;
  a.out_alloc = (f.alloc && !f.masked) ? static_cast<uint8_t*>(e->score[SPX_PLUGIN_ALLOCATABLE].p) : nullptr;
  // the unmasked table is the broadcast of d_alloc_norm, whatever the pod batch: rows that already hold the broadcast of the row in
  // place are not written again (SPX_OPT_ALLOC_TABLE_KEEP) — the sweeps run their instantiations without Allocatable's stores.
  // Only in an engine-owned table (a bound one is the caller's memory), and not for the commit loop's device-side row.
  const DevBuf& alloc_table = e->score[SPX_PLUGIN_ALLOCATABLE];
  t->alloc_keepable = a.out_alloc && !alloc_table.external && !e->row_indirect;
  if (t->alloc_keepable && e->option[SPX_OPT_ALLOC_TABLE_KEEP] && row_end > row_begin) {
    const spx_engine::AllocKept& k = e->alloc_kept;
    t->alloc_kept_now = k.buf == alloc_table.p && k.stride == e->score_stride[SPX_PLUGIN_ALLOCATABLE] && k.epoch == e->alloc_epoch && k.end > k.begin &&
                        row_begin >= k.begin && row_end <= k.end;
    if (t->alloc_kept_now) a.out_alloc = nullptr;
  }
  if (f.alloc && f.masked && !call.skip_alloc_masked) alloc_table_dirty(e);  // a masked normalisation is about to write these rows (launch_net or launch_alloc_masked)
  a.out_tlp = f.tlp ? static_cast<uint8_t*>(e->score[SPX_PLUGIN_TLP].p) : nullptr;
  a.out_lvrb = f.lvrb ? static_cast<uint8_t*>(e->score[SPX_PLUGIN_LVRB].p) : nullptr;
  int rc;
  if (f.lvrb) {
    if ((rc = ensure(e, e->d_lv_exact, static_cast<size_t>(e->n_nodes) * 8 * sizeof(double)))) return rc;
    a.lv_exact = static_cast<double*>(e->d_lv_exact.p);
    if (!e->d_lv_exact.p || !e->d_lv_fast.p || !e->d_lv_amb.p) e->lv_amb_built = false;
    if ((rc = ensure(e, e->d_lv_fast, static_cast<size_t>(spx::round_up(e->row_stride, 512)) * 8 * sizeof(float)))) return rc;
    a.lv_fast = static_cast<float*>(e->d_lv_fast.p);
    if ((rc = ensure(e, e->d_lv_amb, spx::lvrb_amb_bytes()))) return rc;
    a.lv_amb = static_cast<uint32_t*>(e->d_lv_amb.p);
    a.lv_amb_built = &e->lv_amb_built;
    a.lv_amb_geom = e->lv_amb_geom;
  }
  if (f.tlp) {
    if ((rc = tlp_scratch(e, a))) return rc;
    // pod classes: a whole-batch evaluation whose order describes the column in place (every writer of d_tlp_pod clears the flag
    // before it writes and rebuilds the order after), when enough of its rows are copies to pay for the scattered row order
    e->tlp_last_form = 0;
    a.tlp_form = &e->tlp_last_form;
    const int64_t cls_opt = e->option[SPX_OPT_TLP_POD_CLASSES];
    if (cls_opt && e->tlp_order_valid && row_begin == 0 && row_end == e->n_pods && !e->row_indirect && row_end >= 256) {
      const int64_t copied = e->n_pods - e->tlp_rows_evaluated;
      if (cls_opt == 2 ? copied > 0 : copied * 100 >= spx::kTlpClassMinCopyPct * e->n_pods) a.tlp_order = static_cast<const int32_t*>(e->d_tlp_order.p);
    }
  }
  return SPX_OK;
}

// ---- the launches between ev0 and ev1, in this order
int launch_quota_rows(spx_engine* e, int64_t row_begin, int64_t row_end) {
  int rc;
  if ((rc = ensure(e, e->d_q_status, static_cast<size_t>(e->n_pods)))) return rc;
  spx::QuotaArgs qa{};
  qa.row_begin = row_begin;
  qa.row_end = row_end;
  qa.row_ptr = e->row_indirect;
  qa.n_namespaces = e->q_n_namespaces;
  qa.pod_ns = static_cast<const int32_t*>(e->d_q_pod_ns.p);
  qa.pod_priority = static_cast<const int32_t*>(e->d_q_pod_prio.p);
  qa.pod_req = static_cast<const int64_t*>(e->d_q_pod_req.p);
  qa.pod_req_present = static_cast<const uint8_t*>(e->d_q_pod_reqp.p);
  qa.has_quota = static_cast<const uint8_t*>(e->d_q_has.p);
  qa.used = static_cast<const int64_t*>(e->d_q_used.p);
  qa.max = static_cast<const int64_t*>(e->d_q_max.p);
  qa.max_present = static_cast<const uint8_t*>(e->d_q_maxp.p);
  std::memcpy(qa.agg_used, e->q_agg_used, sizeof qa.agg_used);
  std::memcpy(qa.agg_min, e->q_agg_min, sizeof qa.agg_min);
  qa.agg_used_present = e->q_agg_used_present;
  qa.agg_min_present = e->q_agg_min_present;
  qa.agg_used_dyn = e->q_agg_dyn;
  qa.other_nominated = static_cast<const int64_t*>(e->d_q_other.p);
  qa.other_nominated_present = static_cast<const uint8_t*>(e->d_q_otherp.p);
  qa.nom_ptr = static_cast<const int32_t*>(e->d_q_nom_ptr.p);
  qa.nom_priority = static_cast<const int32_t*>(e->d_q_nom_prio.p);
  qa.nom_pending_index = static_cast<const int64_t*>(e->d_q_nom_idx.p);
  qa.nom_req = static_cast<const int64_t*>(e->d_q_nom_req.p);
  qa.nom_req_present = static_cast<const uint8_t*>(e->d_q_nom_reqp.p);
  qa.out_status = static_cast<uint8_t*>(e->d_q_status.p);
  spx::launch_quota(qa, e->stream);
  SPX_HIP(e, hipGetLastError());
  return SPX_OK;
}

// the PodGroup gate: per snapshot the scan and the groups' verdicts (until the next upload), per call the rows' status bytes
int launch_cosched_rows(spx_engine* e, int64_t row_begin, int64_t row_end) {
  spx::CoschedArgs ga{};
  fill_cosched(e, ga);
  ga.row_begin = row_begin;
  ga.row_end = row_end;
  if (!e->cs_gate_valid) {
    spx::launch_cosched_gate(ga, e->stream);
    e->cs_gate_valid = true;
    e->cs_last_walk = e->cs_n_walk;
    e->cs_row_begin = e->cs_row_end = 0;
  }
  spx::launch_cosched_status(ga, e->stream);
  SPX_HIP(e, hipGetLastError());
  if (row_end > row_begin) {
    if (e->cs_row_end > e->cs_row_begin && row_begin <= e->cs_row_end && row_end >= e->cs_row_begin)
      e->cs_row_begin = std::min(e->cs_row_begin, row_begin), e->cs_row_end = std::max(e->cs_row_end, row_end);
    else
      e->cs_row_begin = row_begin, e->cs_row_end = row_end;
  }
  return SPX_OK;
}

// What the dense NRT sweep of one evaluation launches: the arguments, whether one representative per pod class is swept and copied
// to its class, and what d_nrt_fz holds once the fused launch has run (gen 0: matches no later sweep)
struct NrtDensePlan {
  spx::NrtArgs na{};
  bool classes = false;
  spx_engine::FzKey fz_key;
};

// LeastAllocated's Score launch in packed float32 (only the split launch of a row range acts on it: launch_nrt_fast)
int nrt_plan_packed_score(spx_engine* e, spx::NrtArgs& na) {
  NrtPacked pk;
  if (!(na.fast && !(na.opts & spx::kOptNrtGeneric) && !e->row_indirect && nrt_packed_score(e, &pk))) return SPX_OK;
  if (pk.tab_slot >= 0) {
    const size_t bytes = (static_cast<size_t>(pk.tab_kmax) + 1) * pk.tab_words * 4;
    if (!e->d_nrt_pk_tab.p || e->d_nrt_pk_tab.bytes < bytes) e->nrt_pk_tab_built = false;
    if (int rc = ensure(e, e->d_nrt_pk_tab, bytes)) return rc;
  }
  na.pk_mode = 1, na.pk_tab_slot = pk.tab_slot;
  na.pk_tab = static_cast<uint32_t*>(e->d_nrt_pk_tab.p);
  na.pk_tab_words = pk.tab_words, na.pk_tab_kmax = pk.tab_kmax, na.pk_tab_inv_unit = pk.tab_inv_unit;
  na.pk_tab_built = &e->nrt_pk_tab_built;
  return SPX_OK;
}

// LeastNUMANodes, batch launch: per evaluated row and node scope a list of the nodes whose cell needs the complete subset
// search (k_nrt_ln_redo) — room for 3/8 of the nodes per list by default (config #3 lists 13 % of the cells, no row more than 40 %); a
// list that overflows sends the launch back to the complete sweep
void nrt_plan_ln_lists(spx_engine* e, spx::NrtArgs& na, int64_t rows) {
  // The lists are scratch: held to 1 GiB (config #3: 0.42 GB) by shortening them — a shorter list overflows sooner, and an
  // allocation that fails leaves the launch without lists; either way the complete sweep writes the same table, slower
  uint32_t per_row = static_cast<uint32_t>(spx::round_up(std::max<int64_t>(64, e->n_nodes * e->option[SPX_OPT_NRT_LN_LIST_PERMILLE] / 1000), 64));
  constexpr size_t kListWords = (size_t{1} << 30) / sizeof(uint32_t);
  if (rows > 0) {
    const size_t room = (kListWords - 2) / (2 * static_cast<size_t>(rows));  // 1 + per_row words per list
    if (room < 1 + static_cast<size_t>(per_row)) per_row = room > 64 ? static_cast<uint32_t>((room - 1) / 64 * 64) : 0;
  }
  const size_t words = 2 + 2 * static_cast<size_t>(rows) * (1 + static_cast<size_t>(per_row));
  if (rows <= 0 || per_row < 64) return;
  std::string kept;
  {
    std::lock_guard<std::mutex> g(e->err_mu);
    kept = e->err;
  }
  if (ensure(e, e->d_nrt_redo, words * sizeof(uint32_t)) == SPX_OK &&
      ensure(e, e->d_nrt_lnrec, static_cast<size_t>(e->n_nodes) * (SPX_NRT_MAX_ZONES * (e->nrt_n_res <= 4 ? 4 : 8) * 2 + 16) * sizeof(uint32_t)) == SPX_OK) {
    na.redo_list = static_cast<uint32_t*>(e->d_nrt_redo.p);
    na.ln_rec = static_cast<uint32_t*>(e->d_nrt_lnrec.p);
    na.ln_rows = rows;
    na.ln_per_row = per_row;
  } else {
    (void)hipGetLastError();  // the failed allocation's sticky error
    std::lock_guard<std::mutex> g(e->err_mu);
    e->err = kept;
  }
}

// the walk's block start reads the windows' sorted quantities: (re)built when the zone tables changed
int nrt_plan_window_sort(spx_engine* e, spx::NrtArgs& na) {
  int rc;
  size_t rank_bytes = 0;
  const size_t sort_bytes = spx::nrt_window_sort_bytes(e->n_nodes, &rank_bytes);
  if (!e->d_nrt_wsort.p || e->d_nrt_wsort.bytes < sort_bytes || !e->d_nrt_wrank.p || e->d_nrt_wrank.bytes < rank_bytes) e->nrt_wsort_built = false;
  if ((rc = ensure(e, e->d_nrt_wsort, sort_bytes)) || (rc = ensure(e, e->d_nrt_wrank, rank_bytes))) return rc;
  if (!e->nrt_wsort_built) {
    spx::launch_nrt_window_sort(na, static_cast<double*>(e->d_nrt_wsort.p), static_cast<uint16_t*>(e->d_nrt_wrank.p), e->stream);
    e->nrt_wsort_built = true;
  }
  na.wsort = static_cast<const double*>(e->d_nrt_wsort.p);
  na.wrank = static_cast<const uint16_t*>(e->d_nrt_wrank.p);
  return SPX_OK;
}

// decides the form of the dense sweep over [row_begin, row_end) and readies its scratch and derived tables
int nrt_dense_plan(spx_engine* e, int64_t row_begin, int64_t row_end, NrtDensePlan* plan) {
  int rc;
  if (e->nrt_params.strategy == SPX_NRT_LEAST_NUMA_NODES && (rc = build_ln_tab(e))) return rc;
  if (e->nrt_params.strategy == SPX_NRT_BALANCED_ALLOCATION) {
    // room for 1/32 of the cells (config #3 marks 0.7 %); what does not fit is recomputed where it is found.  Inside the
    // sequential commit loop (row_indirect: one row per launch, graph capture) the list allocated for the first pod is kept.
    const uint64_t want = std::max<uint64_t>(4096, static_cast<uint64_t>(row_end - row_begin) * static_cast<uint64_t>(e->row_stride) / 32);
    const uint32_t cap = static_cast<uint32_t>(std::min<uint64_t>(want, 1u << 28));
    if (cap > e->nrt_redo_cap) {
      if ((rc = ensure(e, e->d_nrt_redo, (2 + 2 * static_cast<size_t>(cap)) * sizeof(uint32_t)))) return rc;
      e->nrt_redo_cap = cap;
    }
  }
  if ((rc = ensure_nrt_creq(e))) return rc;
  spx::NrtArgs& na = plan->na;
  fill_nrt(e, na);
  na.row_begin = row_begin;
  na.row_end = row_end;
  na.out_status = static_cast<uint8_t*>(e->status[SPX_PLUGIN_NRT].p);
  na.out_score = static_cast<uint8_t*>(e->score[SPX_PLUGIN_NRT].p);
  const bool batch = na.fast && !(na.opts & spx::kOptNrtGeneric) && !e->row_indirect;  // the float64 formulation, rows given by the host
  const bool whole = row_begin == 0 && row_end == e->n_pods;
  // one representative per pod equivalence class when the whole batch is evaluated with the float64 formulation and enough
  // rows are copies (a partial range may cut a class off from its representative)
  const bool classes = e->option[SPX_OPT_NRT_POD_CLASSES] && batch && whole && e->nrt_n_dups > 0 && e->nrt_n_dups * 32 >= e->n_pods &&
                       !(na.strategy == SPX_NRT_LEAST_NUMA_NODES && !na.ln_tab);
  plan->classes = classes;
  if ((rc = nrt_plan_packed_score(e, na))) return rc;
  // the fused Filter + Score launch (kernels_nrt_fused.hip): a whole-batch LeastAllocated sweep in the packed Score's preconditions with unit
  // weights; it walks the rank stream of the class representatives or, without classes, of every row
  // (BalancedAllocation, round 6b: the walk carries its float32 Score too — no packed-Score preconditions, its own list of cells for float64)
  const bool fz_balanced = na.strategy == SPX_NRT_BALANCED_ALLOCATION && batch;
  bool fused = e->option[SPX_OPT_NRT_FUSED] && e->option[SPX_OPT_NRT_RANK_FILTER] && (na.pk_mode || fz_balanced) && !(na.opts & spx::kOptNrtSingleLaunch) && whole;
  fused = fused && e->option[SPX_OPT_NRT_RANK_NARROW];  // (its only count layout)
  for (int i = 0; fused && !fz_balanced && i < e->nrt_n_res; ++i) fused = e->nrt_slot_weight[i] == 0 || e->nrt_slot_weight[i] == 1;
  if (classes || fused) {
    if ((rc = nrt_rank_stream(e, classes ? 1 : 2))) return rc;
  }
  const bool stream = e->nrt_rk_max_dwords && e->nrt_rk_kind == (classes ? 1 : 2) && e->option[SPX_OPT_NRT_RANK_FILTER];
  if (classes) {
    na.row_list = static_cast<const int32_t*>(e->d_nrt_uniq.p);
    na.n_list = e->nrt_n_uniq;
  }
  fused = fused && stream && e->nrt_rk_all_narrow;
  if (stream && (classes || fused)) {  // the Filter in rank space (its own launch, or inside the fused one)
    na.rk_stream = static_cast<const uint32_t*>(e->d_nrt_rk.p);
    na.rk_off = static_cast<const uint32_t*>(e->d_nrt_rk_off.p);
    na.rk_max_dwords = e->nrt_rk_max_dwords;
    na.rk_first = static_cast<const uint32_t*>(e->d_nrt_rk_first.p);
    na.rk_chunks = e->nrt_rk_chunks;
    na.rk_all_narrow = e->nrt_rk_all_narrow && e->option[SPX_OPT_NRT_FUSED];
    if (!classes) na.n_list = e->n_pods;
    if (fused) {
      if ((rc = ensure(e, e->d_nrt_fz, spx::nrt_fused_item_words(e->nrt_n_res, na.n_list) * sizeof(uint32_t)))) return rc;
      na.fz_items = static_cast<uint32_t*>(e->d_nrt_fz.p);
      plan->fz_key = spx_engine::FzKey{e->nrt_items_gen, classes ? 1 : 2, na.pk_tab_slot, e->d_nrt_fz.p};
      na.fz_pack = !(plan->fz_key == e->nrt_fz_key);
    }
  }
  if (na.strategy == SPX_NRT_LEAST_NUMA_NODES && batch) nrt_plan_ln_lists(e, na, classes ? e->nrt_n_uniq : row_end - row_begin);
  if (na.rk_stream && na.rk_all_narrow && e->nrt_n_res <= 4 && (rc = nrt_plan_window_sort(e, na))) return rc;
  return SPX_OK;
}

// the dense sweep as planned, its copies to the pod classes, then the long rows and the tall nodes' columns
int nrt_dense_launch(spx_engine* e, const NrtDensePlan& plan, int64_t row_begin, int64_t row_end) {
  const spx::NrtArgs& na = plan.na;
  const bool ran_fused = spx::launch_nrt(na, e->stream);
  // the fused launch may decline (BalancedAllocation's cpu slot not exact in float32, a chunk block too large for LDS): then the
  // pack did not run either, and the key must not claim d_nrt_fz holds this pod generation's items
  if (na.fz_items) e->nrt_fz_key = ran_fused ? plan.fz_key : spx_engine::FzKey{};
  e->last_nrt_filter = ran_fused ? 3 : (na.rk_stream ? 2 : 1);
  if (plan.classes)
    spx::launch_rows_expand(static_cast<const int32_t*>(e->d_nrt_dups.p), static_cast<const int32_t*>(e->d_nrt_dups.p) + 2 * e->nrt_n_dups, e->nrt_n_tasks, na.out_status, na.out_score,
                            e->row_stride, e->stream);
  SPX_HIP(e, hipGetLastError());
  int rc;
  // the long rows overwrite what the sweep above wrote from their pod-level request, before NetworkOverhead and Allocatable's
  // masked normalisation read the NRT status table (a long row is a class of its own: no copy of it was made above)
  if ((rc = launch_nrt_long_rows(e, na, row_begin, row_end))) return rc;
  // then the tall nodes' columns of every row of the range (class copies and long rows included), still ahead of those readers
  return launch_nrt_tall_rows(e, na, row_begin, row_end);
}

int launch_nrt_rows(spx_engine* e, int64_t row_begin, int64_t row_end) {
  int rc;
  if (e->nrt_wide) {  // the wide tables: one sparse launch over the row range (kernels_nrt_wide.hip)
    if ((rc = launch_nrt_wide_rows(e, row_begin, row_end, nullptr))) return rc;
    e->last_nrt_filter = 4;
    e->nrt_long_last = 0;
    e->nrt_tall_last = 0;
    return SPX_OK;
  }
  NrtDensePlan plan;
  if ((rc = nrt_dense_plan(e, row_begin, row_end, &plan))) return rc;
  return nrt_dense_launch(e, plan, row_begin, row_end);
}

// NetworkOverhead; *alloc_by_net: Allocatable's masked table was written by this sweep (SPX_OPT_NET_ALLOC_FUSED)
int launch_net_rows(spx_engine* e, const EvalPlugins& f, const EvalCall& call, int64_t row_begin, int64_t row_end, bool* alloc_by_net) {
  spx::NetArgs g{};
  fill_net(e, g);
  g.row_begin = row_begin;
  g.row_end = row_end;
  // upstream scores only nodes that passed every Filter plugin
  const uint8_t* st[3];
  feasibility_status(e, f.mask, st);
  g.other_status[0] = st[0], g.other_status[1] = st[2];
  g.out_status = static_cast<uint8_t*>(e->status[SPX_PLUGIN_NETOVERHEAD].p);
  g.out_score = static_cast<uint8_t*>(e->score[SPX_PLUGIN_NETOVERHEAD].p);
  // Allocatable's masked NormalizeScore rides on the network kernel's walks when both are evaluated over a row range (same feasible
  // set; k_alloc_masked would read the status tables again): launch_net says whether it did
  if (f.alloc && f.masked && !call.skip_alloc_masked && e->alloc_compact && !e->row_indirect && row_end - row_begin > 1 && e->option[SPX_OPT_NET_ALLOC_FUSED]) {
    g.alloc_rel = static_cast<const uint32_t*>(e->d_alloc_rel.p);
    g.out_alloc = static_cast<uint8_t*>(e->score[SPX_PLUGIN_ALLOCATABLE].p);
  }
  *alloc_by_net = spx::launch_net(g, e->stream);
  SPX_HIP(e, hipGetLastError());
  return SPX_OK;
}

int launch_trimaran_rows(spx_engine* e, const EvalPlugins& f, const EvalCall& call, const TrimaranStep& t, int64_t row_begin, int64_t row_end) {
  spx::launch_trimaran(t.a, e->stream);
  SPX_HIP(e, hipGetLastError());
  e->last_alloc_table = !f.alloc ? 0 : f.masked ? (call.skip_alloc_masked ? 0 : 1) : (t.alloc_kept_now ? 2 : 1);
  if (t.alloc_keepable && t.a.out_alloc && row_end > row_begin) {
    // the launch that broadcasts the row into [row_begin, row_end) is on the stream: these rows join the record when they touch
    // rows written to the same buffer from the same row (eval_info's rule), and replace it otherwise
    const DevBuf& alloc_table = e->score[SPX_PLUGIN_ALLOCATABLE];
    spx_engine::AllocKept& k = e->alloc_kept;
    const bool same = k.buf == alloc_table.p && k.stride == e->score_stride[SPX_PLUGIN_ALLOCATABLE] && k.epoch == e->alloc_epoch && k.end > k.begin;
    if (same && row_begin <= k.end && row_end >= k.begin) {
      k.begin = std::min(k.begin, row_begin);
      k.end = std::max(k.end, row_end);
    } else {
      k = spx_engine::AllocKept{row_begin, row_end, alloc_table.p, e->score_stride[SPX_PLUGIN_ALLOCATABLE], e->alloc_epoch};
    }
  }
  return SPX_OK;
}

int launch_lroc_rows(spx_engine* e, int64_t row_begin, int64_t row_end) {
  spx::LrocArgs la{};
  fill_lroc(e, la);
  la.row_begin = row_begin;
  la.row_end = row_end;
  la.out_score = static_cast<uint8_t*>(e->score[SPX_PLUGIN_LROC].p);
  if (!e->lroc_tab_ready) {  // per-node riskLoad: once per (node tables, params)
    spx::launch_lroc_prepare(la, e->stream);
    SPX_HIP(e, hipGetLastError());
    e->lroc_tab_ready = true;
  }
  // inside the sequential commit loop: one row, a whole workgroup on it, in the form chosen for the batch (kernels_commit_scorers.hip)
  if (e->lroc_loop_form >= 0) {
    if (e->lroc_loop_form != spx::kLrocFormF32) la.pod_f32 = nullptr;
    spx::launch_commit_lroc_row(la, e->row_indirect, e->lroc_loop_form, e->stream);
  } else {
    e->lroc_last_form = -1;
    spx::launch_lroc(la, e->stream);
  }
  SPX_HIP(e, hipGetLastError());
  return SPX_OK;
}

// after the Filter plugins: NormalizeScore runs over each pod's feasible nodes
int launch_peaks_rows(spx_engine* e, const EvalPlugins& f, int64_t row_begin, int64_t row_end) {
  spx::PeaksArgs ka{};
  fill_peaks(e, ka);
  ka.row_begin = row_begin;
  ka.row_end = row_end;
  feasibility_status(e, f.mask, ka.other_status);
  ka.out_score = static_cast<uint8_t*>(e->score[SPX_PLUGIN_PEAKS].p);
  // one row per distinct cpu request when the whole batch is swept and nothing narrows a pod's node list (NormalizeScore runs
  // over the same nodes for every pod then), provided enough rows are copies
  const bool classes = e->option[SPX_OPT_PEAKS_POD_CLASSES] && !f.masked && row_begin == 0 && row_end == e->n_pods && e->pk_n_dups > 0 &&
                       e->pk_n_dups * 8 >= e->n_pods;
  if (classes) {
    ka.row_list = static_cast<const int32_t*>(e->d_pk_uniq.p);
    ka.n_list = e->pk_n_uniq;
  }
  if (e->pk_negative || e->peaks_loop_row) ka.opts &= ~spx::kOptPeaksEstimate;  // (the float64 passes take whatever the table holds; one row needs no lists)
  if (ka.opts & spx::kOptPeaksEstimate) {  // the undecided cells' list: sized by the rows this sweep walks
    int rc;
    size_t seg_bytes = 0, cnt_bytes = 0;
    ka.est_pods = spx::peaks_est_plan(ka.opts, e->row_stride, classes ? ka.n_list : row_end - row_begin, &seg_bytes, &cnt_bytes);
    if ((rc = ensure(e, e->d_pk_seg, seg_bytes)) || (rc = ensure(e, e->d_pk_segn, cnt_bytes))) return rc;
    ka.seg = e->d_pk_seg.p;
    ka.seg_n = static_cast<int32_t*>(e->d_pk_segn.p);
  }
  // inside the sequential commit loop with Filter plugins: the pod's row against its CURRENT status rows, one workgroup, no estimate scratch
  if (e->peaks_loop_row)
    spx::launch_commit_peaks_row(ka, e->row_indirect, e->stream);
  else
    spx::launch_peaks(ka, e->stream);
  if (classes)
    spx::launch_rows_expand(static_cast<const int32_t*>(e->d_pk_dups.p), static_cast<const int32_t*>(e->d_pk_dups.p) + 2 * e->pk_n_dups, e->pk_n_tasks, ka.out_score, nullptr,
                            e->row_stride, e->stream);
  SPX_HIP(e, hipGetLastError());
  return SPX_OK;
}

// after the Filter plugins, as Peaks: NormalizeScore runs over each pod's feasible nodes
int launch_sysched_rows(spx_engine* e, const EvalPlugins& f, int64_t per_chunk, int64_t row_begin, int64_t row_end) {
  spx::SyschedArgs ya{};
  fill_sysched(e, ya);
  feasibility_status(e, f.mask, ya.other_status);
  ya.row_begin = row_begin;
  ya.row_end = row_end;
  ya.out_score = static_cast<uint8_t*>(e->score[SPX_PLUGIN_SYSCHED].p);
  // nothing narrows a pod's node list and the whole batch is swept: every distinct set's row is normalised once and copied
  const bool classes = !f.masked && row_begin == 0 && row_end == e->n_pods;
  // a single row needs its own set's raw row only
  int32_t s_lo = 0, s_hi = e->sy_n_sets;
  if (row_end - row_begin == 1) s_lo = e->h_sy_pod_set[static_cast<size_t>(row_begin)], s_hi = s_lo + 1;
  SPX_HIP(e, hipMemsetAsync(e->d_sy_max.p, 0, static_cast<size_t>(e->sy_n_sets) * sizeof(int32_t), e->stream));
  int chunks = 0;
  for (int64_t s0 = s_lo; s0 < s_hi; s0 += per_chunk, ++chunks) {
    ya.set_begin = static_cast<int32_t>(s0);
    ya.set_end = static_cast<int32_t>(std::min<int64_t>(s0 + per_chunk, s_hi));
    spx::launch_sysched_raw(ya, e->stream);
    if (classes) spx::launch_sysched_norm(ya, e->stream);
    else spx::launch_sysched_rows(ya, e->h_sy_first[static_cast<size_t>(ya.set_end)] - e->h_sy_first[static_cast<size_t>(ya.set_begin)], e->stream);
  }
  if (classes && e->sy_n_dups > 0)
    spx::launch_rows_expand(static_cast<const int32_t*>(e->d_sy_dups.p), static_cast<const int32_t*>(e->d_sy_dups.p) + 2 * e->sy_n_dups, e->sy_n_tasks, ya.out_score, nullptr,
                            e->row_stride, e->stream);
  SPX_HIP(e, hipGetLastError());
  e->sy_last_chunks = chunks;
  return SPX_OK;
}

// Allocatable's NormalizeScore over each pod's feasible nodes, when no other sweep of the evaluation has written it
int launch_alloc_masked_rows(spx_engine* e, const EvalPlugins& f, int64_t row_begin, int64_t row_end) {
  spx::ProfileArgs pa{};
  pa.n_nodes = e->n_nodes;
  pa.row_stride = e->row_stride;
  pa.row_begin = row_begin;
  pa.row_end = row_end;
  pa.row_ptr = e->row_indirect;
  feasibility_status(e, f.mask, pa.status);
  pa.alloc_raw = static_cast<const int64_t*>(e->d_alloc_raw.p);
  pa.alloc_rel = static_cast<const uint32_t*>(e->d_alloc_rel.p);
  pa.out_alloc = static_cast<uint8_t*>(e->score[SPX_PLUGIN_ALLOCATABLE].p);
  pa.block_per_row = static_cast<int32_t>(e->option[SPX_OPT_ROW_WORKGROUP]);
  spx::launch_alloc_masked(pa, e->stream);
  SPX_HIP(e, hipGetLastError());
  return SPX_OK;
}

// NodeMetadata's or PodState's table, once the status tables of the evaluation are final: the pod-independent row broadcast when
// nothing narrows a pod's node list, NormalizeScore over each pod's feasible nodes otherwise (kernels_node_columns.hip)
int launch_node_columns(spx_engine* e, const EvalPlugins& f, int plugin, int64_t row_begin, int64_t row_end) {
  spx::NodeColArgs ca{};
  const bool meta = plugin == SPX_PLUGIN_NODEMETA;
  ca.kind = meta ? spx::kNodeColMeta : spx::kNodeColPodState;
  ca.n_nodes = e->n_nodes;
  ca.row_stride = e->row_stride;
  ca.row_begin = row_begin;
  ca.row_end = row_end;
  ca.raw = static_cast<const int64_t*>(meta ? e->d_nm_raw.p : e->d_ps_raw.p);
  feasibility_status(e, f.mask, ca.status);
  ca.norm_row = static_cast<uint8_t*>(e->d_ncol_row.p);
  ca.out_score = static_cast<uint8_t*>(e->score[plugin].p);
  ca.block_per_row = static_cast<int32_t>(e->option[SPX_OPT_ROW_WORKGROUP]);
  spx::launch_node_column(ca, e->stream);
  SPX_HIP(e, hipGetLastError());
  return SPX_OK;
}

// what the engine remembers of an evaluation whose launches are all on the stream
void eval_record(spx_engine* e, const EvalPlugins& f, const EvalCall& call, int64_t row_begin, int64_t row_end) {
  e->timed = true;
  e->best_valid = false;
  e->evaluated |= f.mask;
  const bool alloc_skipped = f.alloc && f.masked && call.skip_alloc_masked;  // spx_decide: the table is not written — nothing to fetch
  if (alloc_skipped) {
    e->evaluated &= ~(1u << SPX_PLUGIN_ALLOCATABLE);
    e->eval_info[SPX_PLUGIN_ALLOCATABLE] = spx_engine::EvalInfo{};
  }
  if (row_end <= row_begin) return;
  const uint32_t filters = f.mask & kFilterPlugins;
  for (int p = 0; p < SPX_NUM_PLUGINS; ++p) {
    if (!((f.mask >> p) & 1u) || (alloc_skipped && p == SPX_PLUGIN_ALLOCATABLE) || p == SPX_PLUGIN_COSCHED) continue;  // (the gate keeps its own rows: cs_row_*)
    spx_engine::EvalInfo& i = e->eval_info[p];
    const bool same_ctx = i.filters == filters && i.ext_gen == e->ext_gen && i.end > i.begin;
    if (same_ctx && row_begin <= i.end && row_end >= i.begin) {  // overlapping or adjacent: the evaluated rows grow
      i.begin = std::min(i.begin, row_begin);
      i.end = std::max(i.end, row_end);
    } else {
      i.begin = row_begin, i.end = row_end, i.filters = filters, i.ext_gen = e->ext_gen;
    }
  }
}

int eval_rows(spx_engine* e, uint32_t plugin_mask, int64_t row_begin, int64_t row_end, const EvalCall& call) {
  SPX_HIP(e, hipSetDevice(e->device));
  const EvalPlugins f = eval_plugins(e, plugin_mask);
  int rc;
  if ((rc = eval_check(e, f, row_begin, row_end))) return rc;
  if ((rc = prepare_tables(e, f))) return rc;
  if (f.lroc && (rc = prepare_lroc(e))) return rc;
  if (f.peaks && (rc = prepare_peaks(e))) return rc;
  int64_t sy_per_chunk = 0;
  if (f.sysched && (rc = prepare_sysched(e, &sy_per_chunk))) return rc;
  if ((f.nodemeta || f.podstate) && (rc = ensure(e, e->d_ncol_row, static_cast<size_t>(e->row_stride)))) return rc;
  TrimaranStep tri;
  if ((rc = prepare_trimaran(e, f, call, row_begin, row_end, &tri))) return rc;
  if (!call.hold_ev0) SPX_HIP(e, hipEventRecord(e->ev0, e->stream));
  bool alloc_by_net = false;
  if (f.quota && (rc = launch_quota_rows(e, row_begin, row_end))) return rc;
  if (f.cosched && (rc = launch_cosched_rows(e, row_begin, row_end))) return rc;
  if (f.nrt && (rc = launch_nrt_rows(e, row_begin, row_end))) return rc;
  if (f.net && (rc = launch_net_rows(e, f, call, row_begin, row_end, &alloc_by_net))) return rc;
  if ((rc = launch_trimaran_rows(e, f, call, tri, row_begin, row_end))) return rc;
  if (f.lroc && (rc = launch_lroc_rows(e, row_begin, row_end))) return rc;
  if (f.peaks && (rc = launch_peaks_rows(e, f, row_begin, row_end))) return rc;
  if (f.sysched && row_end > row_begin && (rc = launch_sysched_rows(e, f, sy_per_chunk, row_begin, row_end))) return rc;
  if (f.alloc && f.masked && !call.skip_alloc_masked && !alloc_by_net && (rc = launch_alloc_masked_rows(e, f, row_begin, row_end))) return rc;
  if (f.nodemeta && (rc = launch_node_columns(e, f, SPX_PLUGIN_NODEMETA, row_begin, row_end))) return rc;
  if (f.podstate && (rc = launch_node_columns(e, f, SPX_PLUGIN_PODSTATE, row_begin, row_end))) return rc;
  SPX_HIP(e, hipEventRecord(e->ev1, e->stream));
  eval_record(e, f, call, row_begin, row_end);
  return SPX_OK;
}

}  // namespace

extern "C" {

int spx_eval(spx_engine* e, uint32_t plugin_mask, int64_t row_begin, int64_t row_end) {
  if (!e) return SPX_ERR_ARG;
  return eval_rows(e, plugin_mask, row_begin, row_end, EvalCall{});
}

int spx_sync(spx_engine* e) {
  if (!e) return SPX_ERR_ARG;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

int spx_nrt_filter_path(const spx_engine* e) { return e ? e->last_nrt_filter : 0; }

int spx_alloc_table_path(const spx_engine* e) { return e ? e->last_alloc_table : 0; }

int spx_tlp_pod_classes(const spx_engine* e, int64_t* rows_evaluated, int64_t* rows_copied) {
  if (!e) return SPX_ERR_ARG;
  if (!e->tri_pods || !e->tlp_order_valid) return fail(e, SPX_ERR_STATE, "TargetLoadPacking: no row order (no pod batch uploaded, or more than 2^31 - 1 rows)");
  if (rows_evaluated) *rows_evaluated = e->tlp_rows_evaluated;
  if (rows_copied) *rows_copied = e->n_pods - e->tlp_rows_evaluated;
  return SPX_OK;
}

int spx_tlp_form(const spx_engine* e) { return e ? e->tlp_last_form : 0; }

int spx_tlp_fetch_order(spx_engine* e, int32_t* rows) {
  if (!e || !rows) return SPX_ERR_ARG;
  if (!e->tri_pods || !e->tlp_order_valid) return fail(e, SPX_ERR_STATE, "TargetLoadPacking: no row order (no pod batch uploaded, or more than 2^31 - 1 rows)");
  const size_t n = static_cast<size_t>(e->n_pods);
  SPX_HIP(e, hipMemcpyAsync(rows, e->d_tlp_order.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

int spx_nrt_wide(const spx_engine* e) { return e && e->nrt_wide ? 1 : 0; }

int spx_nrt_long_rows(const spx_engine* e, int64_t* n_out) {
  if (!e || !n_out) return SPX_ERR_ARG;
  *n_out = e->nrt_long_last;
  return SPX_OK;
}

int spx_nrt_tall_count(const spx_engine* e, int64_t* n_out) {
  if (!e || !n_out) return SPX_ERR_ARG;
  *n_out = e->nrt_tall_last;
  return SPX_OK;
}

int spx_nrt_packed_score_slots(const spx_engine* e) {
  if (!e) return SPX_ERR_ARG;
  NrtPacked pk;
  if (!nrt_packed_score(e, &pk)) return 0;
  return static_cast<int>(0x1000000u | pk.small_slots | (static_cast<uint32_t>(pk.tab_slot + 1) << 16));
}

int spx_commit_path(const spx_engine* e) { return e ? e->last_commit_path : SPX_ERR_ARG; }

int spx_kernel_path(const spx_engine* e, int plugin) {
  if (!e) return SPX_ERR_ARG;
  if (plugin == SPX_PLUGIN_NRT)
    return (e->nrt_fast_slots && e->nrt_fast_nodes && e->nrt_fast_pods && !forced_reference(e, SPX_PLUGIN_NRT) &&
            (e->nrt_params.strategy != SPX_NRT_LEAST_NUMA_NODES || e->nrt_ln_ok)) ? 1 : 0;
  if (plugin == SPX_PLUGIN_NETOVERHEAD) {
    if (e->net_topo && net_wide(e, 0)) return 2;  // the 64-bit sweep, in either of its forms
    return (e->net_nodes && e->net_class16 && e->net_n_classes > 0 && !forced_reference(e, SPX_PLUGIN_NETOVERHEAD)) ? 1 : 0;
  }
  if (plugin == SPX_PLUGIN_LROC) {  // after a sequential commit: the form the loop chose for the batch
    if (e->lroc_last_form >= 0) return e->lroc_last_form == spx::kLrocFormF32 ? 1 : 0;
    return lroc_f32_ok(e) ? 1 : 0;
  }
  if (plugin == SPX_PLUGIN_SYSCHED) return e->sy_last_chunks;
  if (plugin == SPX_PLUGIN_COSCHED) return e->cs_last_walk;
  if (plugin == SPX_PLUGIN_TLP) return (e->tlp.target_utilization >= 1 && e->tlp.target_utilization <= 99 && !(launch_opts(e) & spx::kOptTrimaranExact)) ? 1 : 0;
  return 0;
}

int spx_last_eval_ms(spx_engine* e, float* ms) {
  if (!e || !ms) return SPX_ERR_ARG;
  if (!e->timed) return fail(e, SPX_ERR_STATE, "no spx_eval has run");
  SPX_HIP(e, hipEventSynchronize(e->ev1));
  SPX_HIP(e, hipEventElapsedTime(ms, e->ev0, e->ev1));
  return SPX_OK;
}

namespace {
// A reader thread's own pinned staging buffer and stream (thread-local, per device): a row lands in pinned memory with an async
// copy on the reader's stream and is copied out from there — no pageable-memory path through the runtime's shared staging
// buffers, no engine stream, no engine state.  The calling thread's current device is set first (it is arbitrary on a reader
// thread; with spx_multi the engines live on different devices).
struct ReaderSlot {
  int device = -1;
  hipStream_t stream = nullptr;
  void* pinned = nullptr;
  size_t bytes = 0;
  ~ReaderSlot() {
    if (device < 0) return;
    if (hipSetDevice(device) != hipSuccess) return;
    if (pinned) (void)hipHostFree(pinned);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
thread_local ReaderSlot tl_reader[8];  // by device id modulo 8

int reader_copy(spx_engine* e, void* out, const void* src, size_t bytes) {
  SPX_HIP(e, hipSetDevice(e->device));
  ReaderSlot& r = tl_reader[static_cast<unsigned>(e->device) & 7u];
  if (r.device != e->device) {
    if (r.device >= 0) {  // slot taken by another device id (more than 8 devices): the plain copy
      SPX_HIP(e, hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
      return SPX_OK;
    }
    SPX_HIP(e, hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking));
    r.device = e->device;
  }
  if (r.bytes < bytes) {
    if (r.pinned) SPX_HIP(e, hipHostFree(r.pinned));
    r.pinned = nullptr, r.bytes = 0;
    const size_t want = (bytes + 65535) & ~static_cast<size_t>(65535);
    SPX_HIP(e, hipHostMalloc(&r.pinned, want, hipHostMallocDefault));
    r.bytes = want;
  }
  SPX_HIP(e, hipMemcpyAsync(r.pinned, src, bytes, hipMemcpyDeviceToHost, r.stream));
  SPX_HIP(e, hipStreamSynchronize(r.stream));
  std::memcpy(out, r.pinned, bytes);
  return SPX_OK;
}
}  // namespace

int spx_fetch_scores(spx_engine* e, int plugin, int64_t pod_row, uint8_t* out) {
  if (!e || !out) return SPX_ERR_ARG;
  if (plugin < 0 || plugin >= SPX_NUM_PLUGINS || plugin == SPX_PLUGIN_COSCHED || !(e->evaluated & (1u << plugin)))
    return fail(e, SPX_ERR_STATE, "plugin has not been evaluated");
  if (pod_row < 0 || pod_row >= e->n_pods) return fail(e, SPX_ERR_ARG, "pod_row out of range");
  if (int rc = rows_evaluated(e, plugin, pod_row, pod_row + 1)) return rc;
  // one row, D2H, from any number of reader threads after spx_sync() (no engine state is touched: reader_copy)
  const uint8_t* src = static_cast<const uint8_t*>(e->score[plugin].p) + pod_row * e->score_stride[plugin];
  return reader_copy(e, out, src, static_cast<size_t>(e->n_nodes));
}

int spx_fetch_status(spx_engine* e, int plugin, int64_t pod_row, uint8_t* out) {
  if (!e || !out) return SPX_ERR_ARG;
  if (plugin < 0 || plugin >= SPX_NUM_PLUGINS || !e->status[plugin].p || !(e->evaluated & (1u << plugin)))
    return fail(e, SPX_ERR_STATE, "plugin has no evaluated Filter table");
  if (pod_row < 0 || pod_row >= e->n_pods) return fail(e, SPX_ERR_ARG, "pod_row out of range");
  if (int rc = rows_evaluated(e, plugin, pod_row, pod_row + 1)) return rc;
  const uint8_t* src = static_cast<const uint8_t*>(e->status[plugin].p) + pod_row * e->row_stride;
  return reader_copy(e, out, src, static_cast<size_t>(e->n_nodes));
}

int spx_fetch_raw(spx_engine* e, int plugin, int which, int64_t pod_row, int64_t* out) {
  if (!e || !out) return SPX_ERR_ARG;
  // a raw row is computed on demand (a single-row launch on the engine stream into one scratch row): concurrent readers are
  // serialised here — correct from any thread, but not a fan-out path; the uint8 tables are
  std::lock_guard<std::mutex> raw_guard(e->raw_mu);
  SPX_HIP(e, hipSetDevice(e->device));
  if (e->n_nodes <= 0) return fail(e, SPX_ERR_STATE, "no node table uploaded");
  int rc;
  const size_t bytes = static_cast<size_t>(e->n_nodes) * sizeof(int64_t);
  int64_t* raw = nullptr;  // the scratch row the plugin's launch fills
  // every plugin but Allocatable, after its state check: the row exists and so does the scratch row
  auto scratch_row = [&]() -> int {
    if (pod_row < 0 || pod_row >= e->n_pods) return fail(e, SPX_ERR_ARG, "pod_row out of range");
    const int r = ensure(e, e->d_raw_row, bytes);
    raw = static_cast<int64_t*>(e->d_raw_row.p);
    return r;
  };
  if (plugin == SPX_PLUGIN_ALLOCATABLE) {  // the same row for every pod: no launch
    if ((rc = prepare_alloc(e))) return rc;
    raw = static_cast<int64_t*>(e->d_alloc_raw.p);
  } else if (plugin == SPX_PLUGIN_NRT && e->nrt_wide) {
    if ((rc = scratch_row()) || (rc = launch_nrt_wide_rows(e, pod_row, pod_row + 1, raw))) return rc;
  } else if (plugin == SPX_PLUGIN_NRT) {  // TopologyMatch has no NormalizeScore (score.go:104-106)
    if (!(e->nrt_slots && e->nrt_nodes && e->nrt_pods)) return fail(e, SPX_ERR_STATE, "NRT slot/node/pod tables not uploaded");
    if ((rc = scratch_row()) || (rc = nrt_tall_ready(e))) return rc;
    if (e->nrt_params.strategy == SPX_NRT_LEAST_NUMA_NODES && (rc = build_ln_tab(e))) return rc;
    if ((rc = ensure_nrt_creq(e))) return rc;
    spx::NrtArgs na{};
    fill_nrt(e, na);
    na.row_begin = pod_row;
    na.row_end = pod_row + 1;
    na.out_raw = raw;
    spx::launch_nrt(na, e->stream);
    const int64_t swept = e->nrt_long_last;  // (spx_nrt_long_rows reports spx_eval's sweeps, not this row)
    rc = launch_nrt_long_rows(e, na, pod_row, pod_row + 1);
    e->nrt_long_last = swept;
    if (rc) return rc;
    const int64_t swept_tall = e->nrt_tall_last;
    rc = launch_nrt_tall_rows(e, na, pod_row, pod_row + 1);
    e->nrt_tall_last = swept_tall;
    if (rc) return rc;
  } else if (plugin == SPX_PLUGIN_NETOVERHEAD) {  // raw accumulated cost / satisfied / violated (PreFilterState maps)
    if (!(e->net_nodes && e->net_topo && e->net_pods)) return fail(e, SPX_ERR_STATE, "NetworkOverhead tables not uploaded");
    if ((rc = scratch_row())) return rc;
    if (which < SPX_NET_RAW_COST || which > SPX_NET_RAW_VIOLATED) return fail(e, SPX_ERR_ARG, "which: 0 cost, 1 satisfied, 2 violated");
    if ((rc = net_prepare(e, 0, ""))) return rc;
    spx::NetArgs g{};
    fill_net(e, g);
    g.row_begin = pod_row;
    g.row_end = pod_row + 1;
    g.out_raw = raw;
    g.raw_which = which;
    spx::launch_net(g, e->stream);
  } else if (plugin == SPX_PLUGIN_NODEMETA || plugin == SPX_PLUGIN_PODSTATE) {  // the uploaded column, the same for every pod: no launch
    const bool meta = plugin == SPX_PLUGIN_NODEMETA;
    if (!(meta ? e->nm_nodes : e->ps_nodes)) return fail(e, SPX_ERR_STATE, meta ? "NodeMetadata node column not uploaded" : "PodState node column not uploaded");
    if (e->n_pods > 0 && (pod_row < 0 || pod_row >= e->n_pods)) return fail(e, SPX_ERR_ARG, "pod_row out of range");
    raw = static_cast<int64_t*>(meta ? e->d_nm_raw.p : e->d_ps_raw.p);
  } else if (plugin == SPX_PLUGIN_PEAKS) {  // Peaks.Score before NormalizeScore: the power jump x 1e15
    if (!(e->peaks_nodes && e->peaks_pods)) return fail(e, SPX_ERR_STATE, "Peaks node/pod tables not uploaded");
    if ((rc = scratch_row())) return rc;
    spx::PeaksArgs ka{};
    fill_peaks(e, ka);
    ka.row_begin = pod_row;
    ka.row_end = pod_row + 1;
    ka.out_raw = raw;
    spx::launch_peaks(ka, e->stream);
  } else if (plugin == SPX_PLUGIN_SYSCHED) {  // SySched.Score before NormalizeScore; math.MaxInt64 for a pod with the empty set
    if (!(e->sy_nodes && e->sy_pods)) return fail(e, SPX_ERR_STATE, "SySched node/pod tables not uploaded");
    if (e->sy_node_words != e->sy_pod_words) return fail(e, SPX_ERR_STATE, "SySched: the node and pod tables differ in n_words");
    if ((rc = scratch_row())) return rc;
    spx::SyschedArgs ya{};
    fill_sysched(e, ya);
    ya.set_begin = e->h_sy_pod_set[static_cast<size_t>(pod_row)];
    ya.set_end = ya.set_begin + 1;
    ya.out_raw64 = raw;
    spx::launch_sysched_raw(ya, e->stream);
  } else {
    if (plugin != SPX_PLUGIN_TLP && plugin != SPX_PLUGIN_LVRB) return fail(e, SPX_ERR_ARG, "raw rows: unsupported plugin");
    if (!(e->tri_nodes && e->tri_pods)) return fail(e, SPX_ERR_STATE, "trimaran node/pod tables not uploaded");
    if ((rc = scratch_row())) return rc;
    spx::TrimaranArgs a{};
    fill_trimaran(e, a);
    spx::launch_trimaran_raw(a, plugin, pod_row, raw, e->stream);
  }
  SPX_HIP(e, hipGetLastError());
  SPX_HIP(e, hipMemcpyAsync(out, raw, bytes, hipMemcpyDeviceToHost, e->stream));
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

namespace {
// rows [row_begin,row_end) of a uint8 table into a caller buffer with its own row stride: one strided D2H
int fetch_rows(spx_engine* e, const uint8_t* table, int64_t stride, int64_t row_begin, int64_t row_end, uint8_t* out, int64_t out_stride) {
  if (row_begin < 0 || row_end > e->n_pods || row_begin > row_end) return fail(e, SPX_ERR_ARG, "row range out of bounds");
  if (out_stride < e->n_nodes) return fail(e, SPX_ERR_ARG, "out_stride is smaller than n_nodes");
  if (row_begin == row_end) return SPX_OK;
  SPX_HIP(e, hipSetDevice(e->device));  // reader threads: the current device is per thread
  SPX_HIP(e, hipMemcpy2D(out, static_cast<size_t>(out_stride), table + row_begin * stride, static_cast<size_t>(stride),
                         static_cast<size_t>(e->n_nodes), static_cast<size_t>(row_end - row_begin), hipMemcpyDeviceToHost));
  return SPX_OK;
}
}  // namespace

int spx_fetch_score_rows(spx_engine* e, int plugin, int64_t row_begin, int64_t row_end, uint8_t* out, int64_t out_stride) {
  if (!e || !out) return SPX_ERR_ARG;
  if (plugin < 0 || plugin >= SPX_NUM_PLUGINS || !e->score[plugin].p || !(e->evaluated & (1u << plugin)))
    return fail(e, SPX_ERR_STATE, "plugin has not been evaluated");
  if (row_end > row_begin)
    if (int rc = rows_evaluated(e, plugin, row_begin, row_end)) return rc;
  return fetch_rows(e, static_cast<const uint8_t*>(e->score[plugin].p), e->score_stride[plugin], row_begin, row_end, out, out_stride);
}

int spx_fetch_status_rows(spx_engine* e, int plugin, int64_t row_begin, int64_t row_end, uint8_t* out, int64_t out_stride) {
  if (!e || !out) return SPX_ERR_ARG;
  if (plugin < 0 || plugin >= SPX_NUM_PLUGINS || !e->status[plugin].p || !(e->evaluated & (1u << plugin)))
    return fail(e, SPX_ERR_STATE, "plugin has no evaluated Filter table");
  if (row_end > row_begin)
    if (int rc = rows_evaluated(e, plugin, row_begin, row_end)) return rc;
  return fetch_rows(e, static_cast<const uint8_t*>(e->status[plugin].p), e->row_stride, row_begin, row_end, out, out_stride);
}

int spx_fetch_stats(spx_engine* e, int64_t* reevaluated_cells, int reset) {
  if (!e || !reevaluated_cells) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  std::vector<unsigned long long> h(spx::kStatBytes / sizeof(unsigned long long));
  SPX_HIP(e, hipMemcpyAsync(h.data(), e->d_stats.p, spx::kStatBytes, hipMemcpyDeviceToHost, e->stream));
  if (reset) SPX_HIP(e, hipMemsetAsync(e->d_stats.p, 0, spx::kStatBytes, e->stream));
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  for (int p = 0; p < SPX_NUM_PLUGINS; ++p) {  // the kernels spread their counts over kStatSlots lines per plugin
    unsigned long long sum = 0;
    for (int k = 0; k < spx::kStatSlots; ++k) sum += h[static_cast<size_t>(p * spx::kStatSlots + k) * spx::kStatStride];
    reevaluated_cells[p] = static_cast<int64_t>(sum);
  }
  return SPX_OK;
}

int spx_score_table(spx_engine* e, int plugin, void** dptr, int64_t* row_stride, int64_t* n_rows) {
  if (!e || plugin < 0 || plugin >= SPX_NUM_PLUGINS || plugin == SPX_PLUGIN_COSCHED) return SPX_ERR_ARG;
  if (e->n_nodes <= 0 || e->n_pods <= 0) return fail(e, SPX_ERR_STATE, "shape unknown: upload node and pod tables first");
  int rc = ensure_score_table(e, plugin);
  if (rc) return rc;
  if (dptr) *dptr = e->score[plugin].p;
  if (row_stride) *row_stride = e->score_stride[plugin];
  if (n_rows) *n_rows = e->score_rows[plugin];
  return SPX_OK;
}

int spx_bind_score_table(spx_engine* e, int plugin, void* dptr, int64_t row_stride, int64_t n_rows) {
  if (!e || plugin < 0 || plugin >= SPX_NUM_PLUGINS || plugin == SPX_PLUGIN_COSCHED) return SPX_ERR_ARG;
  DevBuf& b = e->score[plugin];
  if (plugin == SPX_PLUGIN_ALLOCATABLE) alloc_table_dirty(e);  // another buffer from here on (a bound one is never kept: the caller owns it)
  if (!dptr) {  // unbind
    if (b.external) b = DevBuf{};
    e->score_rows[plugin] = e->score_stride[plugin] = 0;
    return SPX_OK;
  }
  if (row_stride % spx::kRowAlign != 0 || (reinterpret_cast<uintptr_t>(dptr) % spx::kRowAlign) != 0)
    return fail(e, SPX_ERR_ARG, "bound table must be 16-byte aligned with a 16-byte multiple row stride");
  if (b.p && !b.external) SPX_HIP(e, hipFree(b.p));
  b.p = dptr;
  b.bytes = static_cast<size_t>(row_stride) * static_cast<size_t>(n_rows);
  b.external = true;
  e->score_rows[plugin] = n_rows;
  e->score_stride[plugin] = row_stride;
  return SPX_OK;
}

int spx_bind_status_table(spx_engine* e, int plugin, void* dptr, int64_t row_stride, int64_t n_rows) {
  if (!e || (plugin != SPX_PLUGIN_NRT && plugin != SPX_PLUGIN_NETOVERHEAD)) return SPX_ERR_ARG;
  DevBuf& b = e->status[plugin];
  if (!dptr) {  // unbind
    if (b.external) b = DevBuf{};
    return SPX_OK;
  }
  if (e->row_stride <= 0) return fail(e, SPX_ERR_STATE, "shape unknown: upload the node table first");
  if (row_stride != e->row_stride || (reinterpret_cast<uintptr_t>(dptr) % spx::kRowAlign) != 0)
    return fail(e, SPX_ERR_ARG, "bound status table must be 16-byte aligned and use the engine row stride (spx_score_table reports it)");
  if (b.p && !b.external) SPX_HIP(e, hipFree(b.p));
  b.p = dptr;
  b.bytes = static_cast<size_t>(row_stride) * static_cast<size_t>(n_rows);
  b.external = true;
  return SPX_OK;
}

}  // extern "C"

namespace spx {
EngineView engine_view(spx_engine* e) {
  EngineView v{};
  v.device = e->device;
  v.stream = e->stream;
  v.n_nodes = e->n_nodes;
  v.n_pods = e->n_pods;
  v.row_stride = e->row_stride;
  v.best = e->d_best.p;
  v.best_valid = e->best_valid;
  v.evaluated = e->evaluated;
  v.ev0 = e->ev0;
  v.ev1 = e->ev1;
  v.timed = e->timed;
  return v;
}
}  // namespace spx

extern "C" {
// spx_decide for a profile with Filter plugins (NRT / NetworkOverhead / a caller mask): the sweeps of `eval_mask` write their
// status and score tables as in spx_eval; Allocatable's feasibility-aware normalisation is folded into the argmax kernel
// (k_decide_masked) over the scoring plugins of `score_mask` — its table is not written, and ALLOCATABLE is left "not evaluated"
// for the fetch functions.  eval_mask differs from score_mask in the sequential commit loop (LVRB's rows are swept once, up
// front).  *done = false: the form does not apply (no Filter in play, wide Allocatable range, weights) — nothing was launched.
int decide_masked(spx_engine* e, uint32_t eval_mask, uint32_t score_mask, int64_t row_begin, int64_t row_end, bool* done) {
  *done = false;
  const uint32_t A = 1u << SPX_PLUGIN_ALLOCATABLE;
  const bool masked = (score_mask & ((1u << SPX_PLUGIN_NRT) | (1u << SPX_PLUGIN_NETOVERHEAD))) || e->ext_mask;
  if (!(score_mask & A) || !(eval_mask & A) || !masked || e->option[SPX_OPT_DECIDE_UNFUSED] || e->n_nodes <= 0 || e->n_pods <= 0 || row_begin < 0 ||
      row_end > e->n_pods || row_begin >= row_end)
    return SPX_OK;
  int rc;
  if ((rc = prepare_alloc(e))) return rc;
  spx::ProfileArgs pa{};
  pa.n_nodes = e->n_nodes;
  pa.row_stride = e->row_stride;
  pa.row_begin = row_begin;
  pa.row_end = row_end;
  pa.row_ptr = e->row_indirect;
  pa.alloc_rel = static_cast<const uint32_t*>(e->d_alloc_rel.p);
  for (int k = 0; k < SPX_NUM_PLUGINS; ++k) {
    const bool has_score = plugin_has_score(k);
    // the tables the sweep below will have written by the time the kernel runs (engine-owned or bound: same row stride)
    if ((score_mask & (1u << k)) && has_score && k != SPX_PLUGIN_ALLOCATABLE) pa.score[k] = reinterpret_cast<const uint8_t*>(uintptr_t{1});
    pa.weight[k] = e->plugin_weight[k];
  }
  if (!e->alloc_compact || !spx::decide_masked_ok(pa)) return SPX_OK;
  BestRows best;
  if ((rc = ensure_best(e, &best))) return rc;
  SPX_HIP(e, hipEventRecord(e->ev0, e->stream));
  EvalCall call;
  call.hold_ev0 = call.skip_alloc_masked = true;
  if ((rc = eval_rows(e, eval_mask, row_begin, row_end, call))) return rc;
  for (int k = 0; k < SPX_NUM_PLUGINS; ++k)
    if (pa.score[k]) {
      if (!(e->evaluated & (1u << k)) || e->score_stride[k] != e->row_stride)
        return fail(e, SPX_ERR_STATE, "spx_decide: a scoring plugin of the mask has no evaluated table with the engine row stride");
      pa.score[k] = static_cast<const uint8_t*>(e->score[k].p);
    }
  feasibility_status(e, score_mask, pa.status);
  pa.prefilter = (score_mask & (1u << SPX_PLUGIN_CAPACITY)) ? static_cast<const uint8_t*>(e->d_q_status.p) : nullptr;
  pa.best_score = best.score, pa.best_node = best.node, pa.best_ties = best.ties, pa.best_feasible = best.feasible;
  pa.block_per_row = static_cast<int32_t>(e->option[SPX_OPT_ROW_WORKGROUP]);
  spx::launch_decide_masked(pa, e->stream);
  SPX_HIP(e, hipGetLastError());
  SPX_HIP(e, hipEventRecord(e->ev1, e->stream));
  e->timed = true;
  e->best_valid = true;
  *done = true;
  return SPX_OK;
}
}  // extern "C" (decide_masked: hidden, shared with spx_commit.hip)

extern "C" {

int spx_eval_best(spx_engine* e, uint32_t plugin_mask, int64_t row_begin, int64_t row_end) {
  if (!e) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  if ((plugin_mask & ~e->evaluated) != 0) return fail(e, SPX_ERR_STATE, "spx_eval_best: plugin in the mask has not been evaluated");
  if (e->n_nodes <= 0 || e->n_pods <= 0) return fail(e, SPX_ERR_STATE, "shape unknown");
  if (row_begin < 0 || row_end > e->n_pods || row_begin > row_end) return fail(e, SPX_ERR_ARG, "row range out of bounds");
  int rc;
  // every table in the sum must cover the rows, and the normalising plugins must have been evaluated under exactly the Filter
  // set this argmax uses (their NormalizeScore ran over the nodes that passed those Filters, as upstream's RunScorePlugins does)
  for (int p = 0; p < SPX_NUM_PLUGINS && row_end > row_begin; ++p) {
    if (!((plugin_mask >> p) & 1u) || p == SPX_PLUGIN_COSCHED) continue;  // (the gate's rows are checked below)
    if ((rc = rows_evaluated(e, p, row_begin, row_end))) return rc;
    const spx_engine::EvalInfo& i = e->eval_info[p];
    const bool ctx_matters = ((kNormalizingPlugins >> p) & 1u) != 0;
    uint32_t want = plugin_mask & kFilterPlugins;
    if (p == SPX_PLUGIN_NETOVERHEAD) want &= ~(1u << SPX_PLUGIN_NETOVERHEAD), want |= i.filters & (1u << SPX_PLUGIN_NETOVERHEAD);  // its own Filter is implied
    if (ctx_matters && (i.filters != want || i.ext_gen != e->ext_gen))
      return fail(e, SPX_ERR_STATE, "spx_eval_best: a normalising plugin (Allocatable / NetworkOverhead / Peaks / SySched / NodeMetadata / PodState) was evaluated under a different Filter set "
                                    "or feasibility mask than this argmax uses; evaluate the whole profile in one spx_eval");
  }
  const bool gate = plugin_mask & (1u << SPX_PLUGIN_COSCHED);
  if (gate && row_end > row_begin && (!e->cs_gate_valid || row_begin < e->cs_row_begin || row_end > e->cs_row_end))
    return fail(e, SPX_ERR_STATE, "spx_eval_best: Coscheduling's gate has not been evaluated for these rows since its last upload");
  if (gate && e->row_indirect) return fail(e, SPX_ERR_STATE, "Coscheduling is not part of the sequential commit loop");
  BestRows best;
  if ((rc = ensure_best(e, &best))) return rc;
  spx::ProfileArgs pa{};
  pa.n_nodes = e->n_nodes;
  pa.row_stride = e->row_stride;
  pa.row_begin = row_begin;
  pa.row_end = row_end;
  pa.row_ptr = e->row_indirect;
  feasibility_status(e, plugin_mask, pa.status);
  pa.prefilter = (plugin_mask & (1u << SPX_PLUGIN_CAPACITY)) ? static_cast<const uint8_t*>(e->d_q_status.p) : nullptr;
  for (int k = 0; k < SPX_NUM_PLUGINS; ++k) {
    const bool has_score = plugin_has_score(k);
    if ((plugin_mask & (1u << k)) && has_score) {
      if (e->score_stride[k] != e->row_stride) return fail(e, SPX_ERR_STATE, "score table stride differs from the engine row stride");
      pa.score[k] = static_cast<const uint8_t*>(e->score[k].p);
    }
    pa.weight[k] = e->plugin_weight[k];
  }
  pa.best_score = best.score, pa.best_node = best.node, pa.best_ties = best.ties, pa.best_feasible = best.feasible;
  spx::launch_best(pa, e->stream);
  if (gate) spx::launch_cosched_unschedulable(static_cast<const uint8_t*>(e->d_cs_status.p), row_begin, row_end, pa.best_score, pa.best_node, pa.best_ties, pa.best_feasible, e->stream);
  SPX_HIP(e, hipGetLastError());
  e->best_valid = true;
  return SPX_OK;
}

}  // extern "C"

namespace {
int decide_profile(spx_engine* e, uint32_t plugin_mask, int64_t row_begin, int64_t row_end);
}

extern "C" int spx_decide(spx_engine* e, uint32_t plugin_mask, int64_t row_begin, int64_t row_end) {
  if (!e) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  const uint32_t C = 1u << SPX_PLUGIN_COSCHED;
  if (!(plugin_mask & C)) return decide_profile(e, plugin_mask, row_begin, row_end);
  // Coscheduling's gate is a PreFilter: it is evaluated on its own, the rest of the profile decides as it would without it, and the
  // rows of the pods it turned away are overwritten (the argmax kernels are the ones of a profile without the bit)
  if ((plugin_mask & ~C) == 0) return fail(e, SPX_ERR_ARG, "spx_decide: Coscheduling alone scores nothing");
  int rc;
  if ((rc = spx_eval(e, C, row_begin, row_end))) return rc;
  if ((rc = decide_profile(e, plugin_mask & ~C, row_begin, row_end))) return rc;
  const BestRows b = best_rows(e);
  spx::launch_cosched_unschedulable(static_cast<const uint8_t*>(e->d_cs_status.p), row_begin, row_end, b.score, b.node, b.ties, b.feasible, e->stream);
  SPX_HIP(e, hipGetLastError());
  return SPX_OK;
}

namespace {
int decide_profile(spx_engine* e, uint32_t plugin_mask, int64_t row_begin, int64_t row_end) {
  const uint32_t A = 1u << SPX_PLUGIN_ALLOCATABLE, T = 1u << SPX_PLUGIN_TLP;
  // Score-only plugins whose tables the fused sweep can fold in: no Filter, and their bytes are final once evaluated
  // (Peaks normalises inside its own sweep)
  const int kExtra[3] = {SPX_PLUGIN_LVRB, SPX_PLUGIN_LROC, SPX_PLUGIN_PEAKS};
  uint32_t extra_mask = 0;
  int64_t w_sum = 0;
  bool w_ok = true;
  for (int p = 0; p < SPX_NUM_PLUGINS; ++p)
    if (plugin_mask & (1u << p)) w_sum += e->plugin_weight[p], w_ok &= e->plugin_weight[p] >= 0;
  for (int x = 0; x < 3; ++x) extra_mask |= plugin_mask & (1u << kExtra[x]);
  const int64_t wa = e->plugin_weight[SPX_PLUGIN_ALLOCATABLE], wt = e->plugin_weight[SPX_PLUGIN_TLP];
  const bool fusable = (plugin_mask & T) && !(plugin_mask & ~(A | T | extra_mask)) && !e->ext_mask && e->tri_nodes && e->tri_pods &&
                       e->tlp.target_utilization >= 1 && e->tlp.target_utilization <= 99 && !(launch_opts(e) & spx::kOptTrimaranExact) &&
                       !e->option[SPX_OPT_DECIDE_UNFUSED] && w_ok && w_sum <= 8000;  // (every weighted total in 21 bits: the sweep's 32-bit key)
  int rc;
  if (!fusable) {  // a profile with Filter plugins: see decide_masked
    bool done = false;
    if ((rc = decide_masked(e, plugin_mask, plugin_mask, row_begin, row_end, &done)) || done) return rc;
  }
  if (!fusable) {
    if ((rc = spx_eval(e, plugin_mask, row_begin, row_end))) return rc;
    return spx_eval_best(e, plugin_mask, row_begin, row_end);
  }
  if (e->n_nodes <= 0 || e->n_pods <= 0) return fail(e, SPX_ERR_STATE, "shape unknown");
  if (row_begin < 0 || row_end > e->n_pods || row_begin > row_end) return fail(e, SPX_ERR_ARG, "row range out of bounds");
  const bool use_alloc = plugin_mask & A;
  if (use_alloc && (rc = prepare_alloc(e))) return rc;
  BestRows best;
  if ((rc = ensure_best(e, &best))) return rc;
  if ((rc = ensure(e, e->d_decide, spx::decide_scratch_bytes(e->row_stride, row_end - row_begin)))) return rc;
  spx::DecideLaunch d{};
  fill_trimaran(e, d.t);
  d.t.row_begin = row_begin;
  d.t.row_end = row_end;
  if ((rc = tlp_scratch(e, d.t))) return rc;
  d.use_alloc = use_alloc;
  d.w_alloc = static_cast<int32_t>(use_alloc ? wa : 0);
  d.w_tlp = static_cast<int32_t>(wt);
  d.scratch = e->d_decide.p;
  d.best_score = best.score, d.best_node = best.node, d.best_ties = best.ties, d.best_feasible = best.feasible;
  SPX_HIP(e, hipEventRecord(e->ev0, e->stream));
  if (extra_mask) {
    EvalCall call;
    call.hold_ev0 = true;
    if ((rc = eval_rows(e, extra_mask, row_begin, row_end, call))) return rc;
    for (int x = 0; x < 3; ++x)
      if (extra_mask & (1u << kExtra[x])) {
        d.w_extra[d.n_extra] = static_cast<int32_t>(e->plugin_weight[kExtra[x]]);
        d.extra[d.n_extra++] = static_cast<const uint8_t*>(e->score[kExtra[x]].p);
      }
  }
  spx::launch_decide_trimaran(d, e->stream);
  SPX_HIP(e, hipGetLastError());
  SPX_HIP(e, hipEventRecord(e->ev1, e->stream));
  e->timed = true;
  e->best_valid = true;
  return SPX_OK;
}
}  // namespace

extern "C" {

int spx_fetch_best(spx_engine* e, int64_t row_begin, int64_t row_end, int32_t* node_idx, int64_t* weighted_score, int32_t* n_ties,
                   int32_t* n_feasible) {
  if (!e || !node_idx || !weighted_score) return SPX_ERR_ARG;
  if (!e->best_valid) return fail(e, SPX_ERR_STATE, "spx_eval_best has not run since the last spx_eval");
  if (row_begin < 0 || row_end > e->n_pods || row_begin > row_end) return fail(e, SPX_ERR_ARG, "row range out of bounds");
  const size_t n = static_cast<size_t>(row_end - row_begin);
  const size_t P = static_cast<size_t>(e->n_pods);
  // one D2H of the whole decision block into pinned memory, then scatter into the caller's arrays
  if (e->h_best_bytes < P * 20) {
    if (e->h_best) SPX_HIP(e, hipHostFree(e->h_best));
    e->h_best = nullptr;
    e->h_best_bytes = 0;
    SPX_HIP(e, hipHostMalloc(&e->h_best, P * 20, hipHostMallocDefault));
    e->h_best_bytes = P * 20;
  }
  SPX_HIP(e, hipMemcpyAsync(e->h_best, e->d_best.p, P * 20, hipMemcpyDeviceToHost, e->stream));
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  const int64_t* hs = static_cast<const int64_t*>(e->h_best);
  const int32_t* hn = reinterpret_cast<const int32_t*>(hs + P);
  std::memcpy(weighted_score, hs + row_begin, n * 8);
  std::memcpy(node_idx, hn + row_begin, n * 4);
  if (n_ties) std::memcpy(n_ties, hn + P + row_begin, n * 4);
  if (n_feasible) std::memcpy(n_feasible, hn + 2 * P + row_begin, n * 4);
  return SPX_OK;
}

}  // extern "C"

