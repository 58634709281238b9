// spx_eval_args.hip — what the evaluation (spx_engine.hip) and the one-pod-at-a-time loops (spx_commit.hip) both do before a launch:
// the engine's options and tables as the kernels' argument structs (launch_opts, fill_*), Allocatable's normalised row
// (alloc_check, prepare_alloc) and NetworkOverhead's cost bound and widening (net_cost_bound, net_bound_check, net_prepare).
// Declared in spx_engine.h; no kernel and no entry point lives here.
#include "spx_engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace spx_eng {

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

}  // namespace spx_eng
