// spx_loads.hip — the one-call loaders: spx_load_* / spx_load_profile turn object tables into SoA columns (the host flatteners) and hand
// them to the spx_upload_* functions of spx_uploads.hip.  Engine state and what crosses the units: spx_engine.h.
#include "spx_engine.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <thread>

extern "C" {

// ---------------------------------------------------------------- object tables -> SoA -> device in one call
// What a cgo (or any FFI) caller wants: it holds object tables (marshalled itself, or decoded by spx_ingest_*) and should not have to
// size and own two dozen intermediate arrays per plugin.  Each function runs the host flatteners with the engine's current plugin
// parameters and uploads the result, exactly the sequence of scheduler-plugins_amd/engine.py's load_*_objects.
int spx_load_trimaran(spx_engine* e, const spx_node_objects* nodes, const spx_resource_classes* rc, const spx_pod_objects* pods, const spx_metrics_objects* metrics,
                      const spx_assigned_objects* assigned) {
  if (!e || !nodes || !pods || !metrics) return SPX_ERR_ARG;
  const size_t N = static_cast<size_t>(nodes->n_nodes), P = static_cast<size_t>(pods->n_pods), R = e->alloc_res.size();
  spx_allocatable_params ap{e->alloc_mode, static_cast<int32_t>(R), e->alloc_res.data(), e->alloc_weight.data()};
  std::vector<int64_t> alloc(R * N);
  if (spx_flatten_alloc_nodes(nodes, rc, &ap, alloc.data()) != SPX_OK) return fail(e, SPX_ERR_ARG, "spx_flatten_alloc_nodes failed");
  spx_alloc_nodes_soa an{nodes->n_nodes, static_cast<int32_t>(R), alloc.data()};
  int rc_;
  if ((rc_ = spx_upload_alloc_nodes(e, &an))) return rc_;
  std::vector<int64_t> cap(N), missing(N), acpu(N), amem(N), tpod(P), rcpu(P), rmem(P);
  std::vector<double> util(N), cavg(N), cstd(N), mavg(N), mstd(N);
  std::vector<uint8_t> valid(N), flags(N);
  if (spx_flatten_trimaran_nodes(nodes, metrics, assigned, &e->tlp, cap.data(), util.data(), missing.data(), valid.data(), acpu.data(), amem.data(), cavg.data(),
                                 cstd.data(), mavg.data(), mstd.data(), flags.data()) != SPX_OK)
    return fail(e, SPX_ERR_ARG, "spx_flatten_trimaran_nodes failed");
  spx_trimaran_nodes_soa tn{nodes->n_nodes, cap.data(), util.data(), missing.data(), valid.data(), acpu.data(), amem.data(), cavg.data(), cstd.data(), mavg.data(),
                            mstd.data(), flags.data()};
  if ((rc_ = spx_upload_trimaran_nodes(e, &tn))) return rc_;
  if (spx_flatten_trimaran_pods(pods, &e->tlp, tpod.data(), rcpu.data(), rmem.data()) != SPX_OK) return fail(e, SPX_ERR_ARG, "spx_flatten_trimaran_pods failed");
  spx_trimaran_pods_soa tp{pods->n_pods, tpod.data(), rcpu.data(), rmem.data()};
  return spx_upload_trimaran_pods(e, &tp);
}

// A new pending batch for the trimaran plugins (and Allocatable): the three pod columns are flattened by all host threads straight
// into the engine's pinned staging buffer and leave with asynchronous DMAs at link speed — through pageable memory (flatten into
// the caller's arrays, then spx_upload_trimaran_pods) the runtime copies each column a second time into its own staging first:
// 1.04 ms for 100 000 pods against the sweep's 0.42.
int spx_load_trimaran_pods(spx_engine* e, const spx_pod_objects* pods) {
  if (!e || !pods) return SPX_ERR_ARG;
  SPX_HIP(e, hipSetDevice(e->device));
  int rc = set_pods(e, pods->n_pods);
  if (rc) return rc;
  const size_t p = static_cast<size_t>(pods->n_pods), col = (p * 8 + 255) & ~static_cast<size_t>(255), bytes = 3 * col;
  SPX_HIP(e, hipStreamSynchronize(e->stream));  // an earlier upload may still be reading the staging buffer
  if ((rc = ensure_pinned(e, e->h_stage, e->h_stage_bytes, bytes, 65536))) return rc;
  char* h = static_cast<char*>(e->h_stage);
  int64_t* tpod = reinterpret_cast<int64_t*>(h);
  int64_t* rcpu = reinterpret_cast<int64_t*>(h + col);
  int64_t* rmem = reinterpret_cast<int64_t*>(h + 2 * col);
  if (spx_flatten_trimaran_pods(pods, &e->tlp, tpod, rcpu, rmem) != SPX_OK) return fail(e, SPX_ERR_ARG, "spx_flatten_trimaran_pods failed");
  e->tlp_order_valid = false;  // (as spx_upload_trimaran_pods)
  if ((rc = upload(e, e->d_tlp_pod, tpod, p * 8))) return rc;
  if ((rc = upload(e, e->d_lv_rcpu, rcpu, p * 8))) return rc;
  if ((rc = upload(e, e->d_lv_rmem, rmem, p * 8))) return rc;
  e->tri_pods = true;
  if ((rc = tlp_build_order(e))) return rc;
  SPX_HIP(e, hipStreamSynchronize(e->stream));
  return SPX_OK;
}

// SySched: both tables from the object image (interned names, distinct sets, residents)
int spx_load_sysched(spx_engine* e, const spx_sysched_objects* o) {
  if (!e || !o) return SPX_ERR_ARG;
  int32_t W = 0;
  int64_t n_stale = 0;
  if (spx_flatten_sysched_nodes(o, 0, &W, &n_stale, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != SPX_OK)
    return fail(e, SPX_ERR_ARG, "spx_flatten_sysched_nodes failed (more than SPX_SYSCHED_MAX_NAMES names, or an id out of range)");
  const size_t N = static_cast<size_t>(o->n_nodes), P = static_cast<size_t>(o->n_pods), S = static_cast<size_t>(o->n_sets);
  std::vector<uint64_t> host(N * static_cast<size_t>(W) + 1), sets(S * static_cast<size_t>(W) + 1);
  std::vector<uint8_t> present(N + 1);
  std::vector<int32_t> k(N + 1), a(N + 1), sptr(N + 1), sbit(static_cast<size_t>(n_stale) + 1), scnt(static_cast<size_t>(n_stale) + 1), pod_set(P + 1);
  if (spx_flatten_sysched_nodes(o, n_stale, &W, &n_stale, host.data(), present.data(), k.data(), a.data(), sptr.data(), sbit.data(), scnt.data()) != SPX_OK)
    return fail(e, SPX_ERR_ARG, "spx_flatten_sysched_nodes failed");
  if (spx_flatten_sysched_pods(o, sets.data(), pod_set.data()) != SPX_OK) return fail(e, SPX_ERR_ARG, "spx_flatten_sysched_pods failed");
  const spx_sysched_nodes_soa ns{o->n_nodes, W, host.data(), present.data(), k.data(), a.data(), sptr.data(), sbit.data(), scnt.data()};
  int rc_;
  if ((rc_ = spx_upload_sysched_nodes(e, &ns))) return rc_;
  const spx_sysched_pods_soa ps{o->n_pods, W, o->n_sets, sets.data(), pod_set.data()};
  return spx_upload_sysched_pods(e, &ps);
}

}  // extern "C"

namespace {
// why a node flattener refused the snapshot, when its zone counts are the reason: the node and its count by name
int fail_nrt_nodes(spx_engine* e, const spx_nrt_objects* nrt, bool wide, const char* plain) {
  int64_t node = -1;
  int32_t nz = 0;
  const int rc = spx_nrt_first_tall_node(nrt, &node, &nz);
  char buf[240];
  if (rc != SPX_OK && node >= 0) {
    std::snprintf(buf, sizeof buf, "NRT: node %lld lists %d NUMA zones of type Node (or one with id 64); this build takes up to %d zones with ids 0..63",
                  static_cast<long long>(node), nz, SPX_NRT_TALL_MAX_ZONES);
    return fail(e, SPX_ERR_ARG, buf);
  }
  if (wide && node >= 0) {
    std::snprintf(buf, sizeof buf, "NRT: node %lld lists %d NUMA zones; a wide snapshot (more than 8 resource slots, or SPX_OPT_NRT_WIDE) takes up to %d per node",
                  static_cast<long long>(node), nz, SPX_NRT_MAX_ZONES);
    return fail(e, SPX_ERR_ARG, buf);
  }
  return fail(e, SPX_ERR_ARG, plain);
}

// the side table of the node table's tall nodes (more than 8 zones), flattened and uploaded after spx_upload_nrt_nodes marked them
int load_nrt_tall(spx_engine* e, const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_nrt_slots& slots) {
  int64_t n_tall = 0;
  int32_t zs = 0;
  if (spx_flatten_nrt_tall_nodes(nodes, nrt, &slots, 0, 0, &n_tall, &zs, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != SPX_OK)
    return fail_nrt_nodes(e, nrt, false, "spx_flatten_nrt_tall_nodes failed");
  const size_t T = static_cast<size_t>(n_tall), S = static_cast<size_t>(zs), R = static_cast<size_t>(slots.n_res > 0 ? slots.n_res : 1);
  std::vector<int32_t> idx(T), mx(T), cost(T * S * S);
  std::vector<uint8_t> fl(T), np(T), nz(T), zid(T * S), zp(T * S);
  std::vector<int64_t> av(T * S * R);
  std::vector<float> mavg(T * S);
  if (spx_flatten_nrt_tall_nodes(nodes, nrt, &slots, n_tall, zs, &n_tall, &zs, idx.data(), fl.data(), mx.data(), np.data(), nz.data(), zid.data(), zp.data(), av.data(),
                                 cost.data(), mavg.data()) != SPX_OK)
    return fail(e, SPX_ERR_ARG, "spx_flatten_nrt_tall_nodes failed");
  const spx_nrt_tall_nodes tt{n_tall, slots.n_res, zs, idx.data(), fl.data(), mx.data(), np.data(), nz.data(), zid.data(), zp.data(), av.data(), cost.data(), mavg.data()};
  return spx_upload_nrt_tall_nodes(e, &tt);
}

// spx_load_nrt's wide route: slot numbering done, the node and pod halves flattened and uploaded side by side as in the dense route
int load_nrt_wide(spx_engine* e, const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_resource_classes* rc, const spx_pod_objects* pods,
                  const spx_nrt_params* params, const spx_nrt_slots& slots) {
  int rc_;
  if ((rc_ = spx_set_nrt_params(e, params)) || (rc_ = spx_upload_nrt_slots_wide(e, &slots))) return rc_;
  if ((rc_ = set_nodes(e, nodes->n_nodes)) || (rc_ = set_pods(e, pods->n_pods))) return rc_;
  const size_t N = static_cast<size_t>(nodes->n_nodes), P = static_cast<size_t>(pods->n_pods), R = static_cast<size_t>(slots.n_res > 0 ? slots.n_res : 1),
               Z = SPX_NRT_MAX_ZONES, C = static_cast<size_t>(pods->ctr_ptr[pods->n_pods] - pods->ctr_ptr[0]);
  int rc_pods = SPX_OK;
  std::thread pod_half([&] {
    int64_t n_req = 0, n_ent = 0;
    if (spx_flatten_nrt_pods_wide(pods, rc, &slots, 0, 0, &n_req, &n_ent, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  nullptr) != SPX_OK) {
      rc_pods = fail(e, SPX_ERR_ARG, "spx_flatten_nrt_pods_wide failed");
      return;
    }
    std::vector<uint8_t> qos(P), nn(P), rslot(static_cast<size_t>(n_req)), ckind(C), eslot(static_cast<size_t>(n_ent));
    std::vector<int32_t> rptr(P + 1), cptr(P + 1), eptr(C + 1);
    std::vector<int64_t> rqty(static_cast<size_t>(n_req)), eqty(static_cast<size_t>(n_ent));
    if (spx_flatten_nrt_pods_wide(pods, rc, &slots, n_req, n_ent, &n_req, &n_ent, qos.data(), nn.data(), rptr.data(), rslot.data(), rqty.data(), cptr.data(),
                                  ckind.data(), eptr.data(), eslot.data(), eqty.data()) != SPX_OK) {
      rc_pods = fail(e, SPX_ERR_ARG, "spx_flatten_nrt_pods_wide failed");
      return;
    }
    const spx_nrt_pods_wide ps{pods->n_pods, slots.n_res, qos.data(), nn.data(), rptr.data(), rslot.data(), rqty.data(), cptr.data(), ckind.data(),
                               eptr.data(), eslot.data(), eqty.data()};
    rc_pods = spx_upload_nrt_pods_wide(e, &ps);
  });
  int rc_nodes = SPX_OK;
  {
    std::vector<uint8_t> nflags(N), nz(N), zid(N * Z);
    std::vector<uint32_t> zp(N * Z), np(N);
    std::vector<int32_t> max_numa(N), zcost(N * Z * Z);
    std::vector<int64_t> zavail(N * Z * R);
    std::vector<float> minavg(N * Z);
    if (spx_flatten_nrt_nodes_wide(nodes, nrt, &slots, nflags.data(), max_numa.data(), nz.data(), zid.data(), zp.data(), zavail.data(), zcost.data(),
                                   minavg.data(), np.data()) != SPX_OK) {
      rc_nodes = fail_nrt_nodes(e, nrt, true, "spx_flatten_nrt_nodes_wide failed");
    } else {
      const spx_nrt_nodes_wide ns{nodes->n_nodes, slots.n_res, nflags.data(), max_numa.data(), nz.data(), zid.data(), zp.data(), zavail.data(), zcost.data(),
                                  minavg.data(), np.data()};
      rc_nodes = spx_upload_nrt_nodes_wide(e, &ns);
    }
  }
  pod_half.join();
  return rc_nodes ? rc_nodes : rc_pods;
}
}  // namespace

extern "C" {

int spx_load_nrt(spx_engine* e, const spx_node_objects* nodes, const spx_nrt_objects* nrt, const spx_resource_classes* rc, const spx_pod_objects* pods,
                 const spx_nrt_params* params) {
  if (!e || !nodes || !nrt || !pods || !params) return SPX_ERR_ARG;
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  for (double& x : e->load_nrt_ms) x = 0.0;
  auto t0 = clk::now();
  // the slot numbering once, wide enough for either form: up to 8 slots it is spx_flatten_nrt_slots' own
  int32_t n_res = 0, slot_res[SPX_NRT_MAX_RES_WIDE] = {0};
  uint8_t slot_flags[SPX_NRT_MAX_RES_WIDE] = {0};
  int64_t slot_weight[SPX_NRT_MAX_RES_WIDE] = {0};
  if (spx_flatten_nrt_slots_wide(pods, nrt, rc, params, SPX_NRT_MAX_RES_WIDE, &n_res, slot_res, slot_flags, slot_weight) != SPX_OK) {
    if (n_res <= SPX_NRT_MAX_RES_WIDE) return fail(e, SPX_ERR_ARG, "spx_flatten_nrt_slots failed");
    char buf[160];
    std::snprintf(buf, sizeof buf, "NRT: the snapshot names %d distinct resources; this build takes up to %d", n_res, SPX_NRT_MAX_RES_WIDE);
    return fail(e, SPX_ERR_ARG, buf);
  }
  const spx_nrt_slots slots{n_res, slot_res, slot_flags, slot_weight};
  e->load_nrt_ms[0] = since(t0);  // 0: spx_flatten_nrt_slots
  if (n_res > SPX_NRT_MAX_RES || e->option[SPX_OPT_NRT_WIDE]) return load_nrt_wide(e, nodes, nrt, rc, pods, params, slots);
  t0 = clk::now();
  int rc_;
  if ((rc_ = spx_set_nrt_params(e, params)) || (rc_ = spx_upload_nrt_slots(e, &slots))) return rc_;
  // (both halves below check the batch / node count against what the engine holds: settled here, before they run side by side)
  if ((rc_ = set_nodes(e, nodes->n_nodes)) || (rc_ = set_pods(e, pods->n_pods))) return rc_;
  e->load_nrt_ms[3] = since(t0);  // 3: params + slot table
  const size_t N = static_cast<size_t>(nodes->n_nodes), P = static_cast<size_t>(pods->n_pods), R = static_cast<size_t>(n_res > 0 ? n_res : 1), Z = SPX_NRT_MAX_ZONES,
               Cn = SPX_NRT_MAX_CTRS;
  // Round 6: the node half (flatten 1.8 ms + upload 2.7 ms at 20 000 nodes) and the pod half (0.4 + 2.7 ms at 8 192 pods) touch disjoint
  // engine state — node tables / the blob staging, pod tables / the record stream's staging — and one stream; they run on two host
  // threads (each with its own worker pool, parallel.hpp).  Stages 1 / 4 and 2 / 5 therefore overlap in time.
  int rc_pods = SPX_OK;
  std::thread pod_half([&] {
    const auto t1 = clk::now();
    std::vector<uint8_t> qos(P), nn(P), nctr(P), ckind(P * Cn), cpres(P * Cn), ppres(P);
    std::vector<int64_t> creq(P * Cn * R), preq(P * R);
    if (spx_flatten_nrt_pods(pods, rc, &slots, qos.data(), nn.data(), nctr.data(), ckind.data(), cpres.data(), creq.data(), ppres.data(), preq.data()) != SPX_OK) {
      rc_pods = fail(e, SPX_ERR_ARG, "spx_flatten_nrt_pods failed");
      return;
    }
    e->load_nrt_ms[2] = since(t1);  // 2: pod columns allocated + spx_flatten_nrt_pods
    const auto t2 = clk::now();
    const spx_nrt_pods_soa ps{pods->n_pods, n_res, qos.data(), nn.data(), nctr.data(), ckind.data(), cpres.data(), creq.data(), ppres.data(), preq.data()};
    rc_pods = spx_upload_nrt_pods(e, &ps);
    if (rc_pods == SPX_OK && !e->nrt_long_ok) {  // pods with more than 8 containers: their CSR table
      int64_t n_long = 0, n_lc = 0;
      spx_flatten_nrt_long_pods(pods, rc, &slots, 0, 0, &n_long, &n_lc, nullptr, nullptr, nullptr, nullptr, nullptr);
      const size_t Ls = static_cast<size_t>(n_long), Cs = static_cast<size_t>(n_lc);
      std::vector<int32_t> lrow(Ls), lptr(Ls + 1);
      std::vector<uint8_t> lkind(Cs), lpres(Cs);
      std::vector<int64_t> lreq(Cs * R);
      if (spx_flatten_nrt_long_pods(pods, rc, &slots, n_long, n_lc, &n_long, &n_lc, lrow.data(), lptr.data(), lkind.data(), lpres.data(), lreq.data()) != SPX_OK) {
        rc_pods = fail(e, SPX_ERR_ARG, "spx_flatten_nrt_long_pods failed");
        return;
      }
      const spx_nrt_long_pods lt{n_long, n_res, lrow.data(), lptr.data(), lkind.data(), lpres.data(), lreq.data()};
      rc_pods = spx_upload_nrt_long_pods(e, &lt);
    }
    e->load_nrt_ms[5] = since(t2);  // 5: spx_upload_nrt_pods (item stream, pod classes, rank stream)
  });
  int rc_nodes = SPX_OK;
  {
    const auto t1 = clk::now();
    std::vector<uint8_t> nflags(N), nz(N), zid(N * Z), zp(N * Z), np(N);
    std::vector<int32_t> max_numa(N), zcost(N * Z * Z);
    std::vector<int64_t> zavail(N * Z * R);
    std::vector<float> minavg(N * Z);
    if (spx_flatten_nrt_nodes(nodes, nrt, &slots, nflags.data(), max_numa.data(), nz.data(), zid.data(), zp.data(), zavail.data(), zcost.data(), minavg.data(), np.data()) !=
        SPX_OK) {
      rc_nodes = fail_nrt_nodes(e, nrt, false, "spx_flatten_nrt_nodes failed");
    } else {
      e->load_nrt_ms[1] = since(t1);  // 1: node columns allocated + spx_flatten_nrt_nodes
      const auto t2 = clk::now();
      const spx_nrt_nodes_soa ns{nodes->n_nodes, n_res, nflags.data(), max_numa.data(), nz.data(), zid.data(), zp.data(), zavail.data(), zcost.data(), minavg.data(), np.data()};
      rc_nodes = spx_upload_nrt_nodes(e, &ns);
      if (rc_nodes == SPX_OK && !e->nrt_tall_ok) rc_nodes = load_nrt_tall(e, nodes, nrt, slots);  // nodes with more than 8 zones: their side table
      e->load_nrt_ms[4] = since(t2);  // 4: spx_upload_nrt_nodes (precondition checks, window-local node order, one blob, derived columns on the device)
    }
  }
  pod_half.join();
  return rc_nodes ? rc_nodes : rc_pods;
}

// The four loaders of a full profile side by side: they fill disjoint tables of the engine (trimaran + Allocatable columns, NRT tables,
// NetworkOverhead tables, quota tables), share one stream, and each takes a worker pool of its own.  Members left NULL skip their loader.
int spx_load_profile(spx_engine* e, const spx_profile_objects* o) {
  if (!e || !o || !o->nodes || !o->pods) return SPX_ERR_ARG;
  if (o->nrt && !o->nrt_params) return fail(e, SPX_ERR_ARG, "spx_load_profile: nrt without nrt_params");
  int rc_;
  if ((rc_ = set_nodes(e, o->nodes->n_nodes)) || (rc_ = set_pods(e, o->pods->n_pods))) return rc_;
  int rcs[4] = {SPX_OK, SPX_OK, SPX_OK, SPX_OK};
  std::string msgs[4];  // a failing loader's message, taken on the thread it failed on (fail() records it in that thread's tl_err)
  const auto run = [&](int i, const auto& load) {
    tl_err_engine = nullptr;
    rcs[i] = load();
    if (rcs[i] && tl_err_engine == e) msgs[i] = tl_err;
  };
  std::vector<std::thread> th;
  if (o->nrt) th.emplace_back([&] { run(1, [&] { return spx_load_nrt(e, o->nodes, o->nrt, o->rc, o->pods, o->nrt_params); }); });  // the longest first
  if (o->appgroups && o->nettopo) th.emplace_back([&] { run(2, [&] { return spx_load_network(e, o->nodes, o->pods, o->appgroups, o->nettopo); }); });
  if (o->quota) th.emplace_back([&] { run(3, [&] { return spx_load_quota(e, o->pods, o->rc, o->quota); }); });
  if (o->metrics) run(0, [&] { return spx_load_trimaran(e, o->nodes, o->rc, o->pods, o->metrics, o->assigned); });
  for (std::thread& t : th) t.join();
  // the caller's spx_last_error must name the failure returned here, not an older one of this thread on this engine
  for (int i = 0; i < 4; ++i)
    if (rcs[i]) return fail(e, rcs[i], msgs[i].empty() ? std::string("spx_load_profile: a loader failed") : msgs[i]);
  return SPX_OK;
}

int spx_last_load_nrt_ms(const spx_engine* e, double* ms6) {
  if (!e || !ms6) return SPX_ERR_ARG;
  std::memcpy(ms6, e->load_nrt_ms, sizeof e->load_nrt_ms);
  return SPX_OK;
}

int spx_load_network(spx_engine* e, const spx_node_objects* nodes, const spx_pod_objects* pods, const spx_appgroup_objects* appgroups, const spx_nettopo_objects* nettopo) {
  if (!e || !nodes || !pods || !appgroups || !nettopo) return SPX_ERR_ARG;
  const size_t P = static_cast<size_t>(pods->n_pods);
  const size_t rg = static_cast<size_t>(nettopo->n_regions), zc = static_cast<size_t>(nettopo->n_zones);
  // the cost matrices are flattened in the CRD's own int64; a snapshot whose entries all fit int32 is narrowed and takes the 32-bit
  // tables as before, any other one the wide tables (spx_upload_net_topo_wide)
  std::vector<int64_t> rcost64(rg * rg ? rg * rg : 1, -1), zcost64(zc * zc ? zc * zc : 1, -1);
  if (spx_flatten_net_topo_wide(nettopo, rcost64.data(), zcost64.data()) != SPX_OK) return fail(e, SPX_ERR_ARG, "spx_flatten_net_topo_wide failed");
  const auto fits = [](const std::vector<int64_t>& v) { return std::all_of(v.begin(), v.end(), [](int64_t c) { return c <= INT32_MAX; }); };
  const bool narrow = fits(rcost64) && fits(zcost64);
  std::vector<int32_t> rcost, zcost;
  if (narrow) rcost.assign(rcost64.begin(), rcost64.end()), zcost.assign(zcost64.begin(), zcost64.end());
  int32_t n_keys = 0;
  int64_t n_pairs = 0, n_eff = 0;
  if (spx_flatten_net_keys(pods, appgroups, &n_keys, &n_pairs, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != SPX_OK)
    return fail(e, SPX_ERR_ARG, "spx_flatten_net_keys failed");
  std::vector<int32_t> pod_key(P), topo(P), pair_ptr(static_cast<size_t>(n_keys) + 1), pair_node(n_pairs > 0 ? static_cast<size_t>(n_pairs) : 1);
  std::vector<uint8_t> eq(n_keys > 0 ? static_cast<size_t>(n_keys) : 1);
  std::vector<int64_t> pair_max(n_pairs > 0 ? static_cast<size_t>(n_pairs) : 1);
  if (spx_flatten_net_keys(pods, appgroups, &n_keys, &n_pairs, pod_key.data(), topo.data(), eq.data(), pair_ptr.data(), pair_node.data(), pair_max.data()) != SPX_OK)
    return fail(e, SPX_ERR_ARG, "spx_flatten_net_keys failed");
  if (spx_flatten_net_commit(pods, appgroups, &n_eff, nullptr, nullptr, nullptr) != SPX_OK) return fail(e, SPX_ERR_ARG, "spx_flatten_net_commit failed");
  std::vector<int32_t> eff_ptr(P + 1), eff_key(n_eff > 0 ? static_cast<size_t>(n_eff) : 1);
  std::vector<int64_t> eff_cost(n_eff > 0 ? static_cast<size_t>(n_eff) : 1);
  if (spx_flatten_net_commit(pods, appgroups, &n_eff, eff_ptr.data(), eff_key.data(), eff_cost.data()) != SPX_OK) return fail(e, SPX_ERR_ARG, "spx_flatten_net_commit failed");
  int rc_;
  const spx_net_nodes_soa nn{nodes->n_nodes, nodes->region, nodes->zone};
  if ((rc_ = spx_upload_net_nodes(e, &nn))) return rc_;
  if (narrow) {
    const spx_net_topo_soa nt{nettopo->n_regions, nettopo->n_zones, rcost.data(), zcost.data()};
    if ((rc_ = spx_upload_net_topo(e, &nt))) return rc_;
  } else {
    const spx_net_topo_wide nt{nettopo->n_regions, nettopo->n_zones, rcost64.data(), zcost64.data()};
    if ((rc_ = spx_upload_net_topo_wide(e, &nt))) return rc_;
  }
  const spx_net_pods_soa np{pods->n_pods, n_keys, pod_key.data(), eq.data(), pair_ptr.data(), pair_node.data(), pair_max.data(), topo.data()};
  if ((rc_ = spx_upload_net_pods(e, &np))) return rc_;
  const spx_net_commit_soa nc{pods->n_pods, eff_ptr.data(), eff_key.data(), eff_cost.data()};
  return spx_upload_net_commit(e, &nc);
}

int spx_load_quota(spx_engine* e, const spx_pod_objects* pods, const spx_resource_classes* rc, const spx_quota_objects* quota) {
  if (!e || !pods || !quota) return SPX_ERR_ARG;
  constexpr size_t S = SPX_QUOTA_SLOTS;
  const size_t P = static_cast<size_t>(pods->n_pods), NS = static_cast<size_t>(quota->n_namespaces), NN = quota->n_nominated > 0 ? static_cast<size_t>(quota->n_nominated) : 1;
  std::vector<int32_t> pod_ns(P), pod_prio(P), nom_ptr(NS + 1), nom_prio(NN);
  std::vector<int64_t> pod_req(P * S), agg_used(S), agg_min(S), other((NS ? NS : 1) * S), nom_pending(NN), nom_req(NN * S);
  std::vector<uint8_t> pod_reqp(P), other_p(NS ? NS : 1), nom_reqp(NN);
  uint8_t agg_used_p = 0, agg_min_p = 0;
  if (spx_flatten_quota(pods, rc, quota, pod_ns.data(), pod_prio.data(), pod_req.data(), pod_reqp.data(), agg_used.data(), &agg_used_p, agg_min.data(), &agg_min_p, other.data(),
                        other_p.data(), nom_ptr.data(), nom_prio.data(), nom_pending.data(), nom_req.data(), nom_reqp.data()) != SPX_OK)
    return fail(e, SPX_ERR_ARG, "spx_flatten_quota failed");
  spx_quota_soa q{};
  q.n_pods = pods->n_pods, q.n_namespaces = quota->n_namespaces;
  q.pod_ns = pod_ns.data(), q.pod_priority = pod_prio.data(), q.pod_req = pod_req.data(), q.pod_req_present = pod_reqp.data();
  q.has_quota = quota->has_quota, q.used = quota->used, q.used_present = quota->used_present, q.max = quota->max, q.max_present = quota->max_present;
  q.agg_used = agg_used.data(), q.agg_used_present = &agg_used_p, q.agg_min = agg_min.data(), q.agg_min_present = &agg_min_p;
  q.other_nominated = other.data(), q.other_nominated_present = other_p.data();
  q.nom_ptr = nom_ptr.data(), q.nom_priority = nom_prio.data(), q.nom_pending_index = nom_pending.data(), q.nom_req = nom_req.data(), q.nom_req_present = nom_reqp.data();
  q.min = quota->min, q.min_present = quota->min_present;
  return spx_upload_quota(e, &q);
}

}  // extern "C"
