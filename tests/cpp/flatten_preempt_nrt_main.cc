// flatten_preempt_nrt_main.cc — the host flattener of the preemption tables' NRT side table on a seeded snapshot, as a program of its own:
// built with the host sources it calls under -fsanitize=address,undefined (tests/test_flatten_preempt_nrt_sanitized.py), it exits 0
// when every call answered as expected and the sanitizers found nothing.
//
// The snapshot: N nodes of 1..8 zones reporting cpu, memory and one extended resource, 0..40 pods per node of one or two containers
// with random placements (valid ids, ids the node lacks, none, unknown), pending pods of 1..8 containers.  Checked: the flattener and
// the check function accept it, every array is written within its stated size (the arrays are exactly that size, so ASan sees one
// byte more), rel_cap one short is refused with the count, and the additivity claim against spx_nrt_post_eviction for the whole list of
// every node.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "spx.h"

namespace {

struct Pods {
  std::vector<int32_t> ctr_ptr{0}, req_ptr{0}, req_res, lim_ptr{0}, lim_res, ovh_ptr{0}, priority, appgroup, selector, ns;
  std::vector<uint8_t> ctr_kind;
  std::vector<int64_t> req_qty, lim_qty, queue_ts;
  void container(uint8_t kind, const std::vector<std::pair<int32_t, int64_t>>& req, bool limits) {
    ctr_kind.push_back(kind);
    for (auto& r : req) {
      req_res.push_back(r.first), req_qty.push_back(r.second);
      if (limits) lim_res.push_back(r.first), lim_qty.push_back(r.second);
    }
    req_ptr.push_back(static_cast<int32_t>(req_res.size()));
    lim_ptr.push_back(static_cast<int32_t>(lim_res.size()));
  }
  void end_pod() {
    ctr_ptr.push_back(static_cast<int32_t>(ctr_kind.size()));
    ovh_ptr.push_back(0), priority.push_back(0), queue_ts.push_back(0), appgroup.push_back(-1), selector.push_back(-1), ns.push_back(0);
  }
  spx_pod_objects view() const {
    static const int32_t none32 = 0;
    static const int64_t none64 = 0;
    spx_pod_objects p{};
    p.n_pods = static_cast<int64_t>(ctr_ptr.size()) - 1;
    p.ctr_ptr = ctr_ptr.data(), p.ctr_kind = ctr_kind.data(), p.req_ptr = req_ptr.data(), p.lim_ptr = lim_ptr.data(), p.ovh_ptr = ovh_ptr.data();
    p.req_res = req_res.empty() ? &none32 : req_res.data(), p.req_qty = req_qty.empty() ? &none64 : req_qty.data();
    p.lim_res = lim_res.empty() ? &none32 : lim_res.data(), p.lim_qty = lim_qty.empty() ? &none64 : lim_qty.data();
    p.ovh_res = &none32, p.ovh_qty = &none64;
    p.priority = priority.data(), p.queue_ts = queue_ts.data(), p.appgroup = appgroup.data(), p.selector = selector.data(), p.ns = ns.data();
    return p;
  }
};

#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      return 1;                                                          \
    }                                                                    \
  } while (0)

}  // namespace

int main() {
  constexpr int64_t N = 97, P = 33;
  constexpr int32_t kExt = SPX_RES_FIRST_DYNAMIC;
  constexpr int64_t GiB = int64_t{1} << 30;
  std::mt19937_64 rng(20240611);
  auto pick = [&](int n) { return static_cast<int>(rng() % static_cast<uint64_t>(n)); };

  // nodes and their NRTs
  std::vector<int64_t> cpu(N, 64000), mem(N, 256 * GiB), eph(N, 0), podcap(N, 110);
  std::vector<int32_t> scalar_ptr(N + 1), scalar_res(N, kExt), region(N, -1), zone(N, -1);
  std::vector<int64_t> scalar_qty(N, 8);
  for (int64_t n = 0; n <= N; ++n) scalar_ptr[n] = static_cast<int32_t>(n);
  spx_node_objects nodes{N, cpu.data(), mem.data(), eph.data(), podcap.data(), scalar_ptr.data(), scalar_res.data(), scalar_qty.data(), cpu.data(), region.data(), zone.data()};
  std::vector<uint8_t> has_nrt(N), fresh(N), zone_is_node, placement_present(N);
  std::vector<int8_t> legacy(N), attr(N, -1);
  std::vector<int32_t> attr_max(N, -1), zone_ptr{0}, zone_id, zres_ptr{0}, zres_res, none_ptr(N + 1, 0), placement_containers(N);
  std::vector<int64_t> zres_avail, zres_alloc;
  std::vector<std::vector<int>> ids(N);
  for (int64_t n = 0; n < N; ++n) {
    has_nrt[n] = pick(10) != 0, fresh[n] = pick(12) != 0, legacy[n] = static_cast<int8_t>((3 << 1) | pick(2));
    placement_present[n] = pick(8) != 0, placement_containers[n] = placement_present[n] ? pick(6) : 0;
    const int nz = has_nrt[n] ? 1 + static_cast<int>(n % 8) : 0;
    for (int z = 0; z < nz; ++z) {
      ids[n].push_back(2 * z + 1);
      zone_is_node.push_back(1), zone_id.push_back(2 * z + 1);
      for (int32_t res : {static_cast<int32_t>(SPX_RES_CPU), static_cast<int32_t>(SPX_RES_MEMORY), kExt}) {
        if (res == kExt && pick(3) == 0) continue;
        const int64_t alloc = res == SPX_RES_CPU ? 8000 : res == SPX_RES_MEMORY ? 32 * GiB : 2;
        zres_res.push_back(res), zres_alloc.push_back(alloc), zres_avail.push_back(alloc / (1 + pick(3)));
      }
      zres_ptr.push_back(static_cast<int32_t>(zres_res.size()));
    }
    zone_ptr.push_back(static_cast<int32_t>(zone_id.size()));
  }
  zone_is_node.push_back(0), zone_id.push_back(0), zres_res.push_back(0), zres_avail.push_back(0), zres_alloc.push_back(0);  // (never NULL)
  std::vector<int32_t> zcost_ptr(zone_ptr.back() + 1, 0);
  const int32_t no32 = 0;
  const int64_t no64 = 0;
  spx_nrt_objects nrt{};
  nrt.n_nodes = N, nrt.has_nrt = has_nrt.data(), nrt.fresh = fresh.data(), nrt.legacy_policy = legacy.data(), nrt.attr_scope = attr.data(), nrt.attr_policy = attr.data();
  nrt.attr_max_numa = attr_max.data(), nrt.zone_ptr = zone_ptr.data(), nrt.zone_is_node = zone_is_node.data(), nrt.zone_numa_id = zone_id.data();
  nrt.zres_ptr = zres_ptr.data(), nrt.zres_res = zres_res.data(), nrt.zres_avail = zres_avail.data(), nrt.zcost_ptr = zcost_ptr.data(), nrt.zcost_numa_id = &no32;
  nrt.zcost_value = &no64, nrt.assumed_ptr = none_ptr.data(), nrt.arl_ptr = &no32, nrt.arl_res = &no32, nrt.arl_qty = &no64, nrt.zres_allocatable = zres_alloc.data();

  // the assigned pods, node by node, and where the kubelet put their containers
  Pods assigned;
  std::vector<int64_t> assigned_node;
  std::vector<int32_t> ctr_numa;
  for (int64_t n = 0; n < N; ++n)
    for (int k = pick(41); k > 0; --k) {
      const bool guaranteed = pick(2);
      for (int c = 1 + pick(2); c > 0; --c) {
        std::vector<std::pair<int32_t, int64_t>> req{{SPX_RES_CPU, 500 * (1 + pick(4))}, {SPX_RES_MEMORY, GiB}};
        if (pick(4) == 0) req.push_back({kExt, pick(2)});
        assigned.container(SPX_CTR_APP, req, guaranteed);
        const int how = pick(10);
        ctr_numa.push_back(how < 7 && !ids[n].empty() ? ids[n][pick(static_cast<int>(ids[n].size()))] : how == 7 ? 40 : how == 8 ? -1 : SPX_EVICT_CTR_UNKNOWN);
      }
      assigned.end_pod();
      assigned_node.push_back(n);
    }
  const int64_t A = static_cast<int64_t>(assigned_node.size());
  const spx_pod_objects assigned_view = assigned.view();
  spx_preempt_objects o{};
  o.n_assigned = A, o.assigned = &assigned_view, o.assigned_node = assigned_node.data();
  std::vector<int32_t> pod_src(A);
  for (int64_t j = 0; j < A; ++j) pod_src[j] = static_cast<int32_t>(A - 1 - j);  // (any permutation: the outputs follow it)

  // the pending pods
  Pods pending;
  for (int64_t i = 0; i < P; ++i) {
    const int n_ctr = 1 + static_cast<int>(i % 8);
    for (int c = 0; c < n_ctr; ++c) pending.container(c == 0 && n_ctr > 2 ? SPX_CTR_INIT : SPX_CTR_APP, {{SPX_RES_CPU, 1000}, {SPX_RES_MEMORY, GiB}}, i % 2 == 0);
    pending.end_pod();
  }
  const spx_pod_objects pending_view = pending.view();

  // slots, side table, preemptor records: every output exactly as large as the header says
  int32_t n_res = 0, slot_res[SPX_NRT_MAX_RES];
  uint8_t slot_flags[SPX_NRT_MAX_RES];
  int64_t slot_weight[SPX_NRT_MAX_RES];
  EXPECT(spx_flatten_nrt_slots(&pending_view, &nrt, nullptr, nullptr, &n_res, slot_res, slot_flags, slot_weight) == SPX_OK);
  EXPECT(n_res == 3);
  const spx_nrt_slots slots{n_res, slot_res, slot_flags, slot_weight};
  std::vector<uint8_t> node_flags(N), n_zones(N), zid(N * 8), zpresent(N * 8), node_present(N), contributes(A);
  std::vector<int64_t> avail(N * 8 * n_res), room(N * 8 * n_res);
  std::vector<int32_t> rel_ptr(A + 1);
  int64_t n_rel = -1, bad = -1;
  auto flatten = [&](int64_t cap, uint8_t* rz, uint8_t* rs, int64_t* rq) {
    return spx_flatten_preempt_nrt(&nodes, &nrt, nullptr, &slots, &o, ctr_numa.data(), placement_present.data(), placement_containers.data(), A, pod_src.data(), cap, &n_rel,
                                   &bad, node_flags.data(), n_zones.data(), zid.data(), zpresent.data(), node_present.data(), avail.data(), room.data(), contributes.data(),
                                   rel_ptr.data(), rz, rs, rq);
  };
  EXPECT(flatten(0, nullptr, nullptr, nullptr) == SPX_ERR_ARG && n_rel > 0);  // the count
  const int64_t want_rel = n_rel;
  {
    std::vector<uint8_t> rz(want_rel - 1), rs(want_rel - 1);
    std::vector<int64_t> rq(want_rel - 1);
    EXPECT(flatten(want_rel - 1, rz.data(), rs.data(), rq.data()) == SPX_ERR_ARG && n_rel >= want_rel);  // one short
  }
  std::vector<uint8_t> rz(want_rel), rs(want_rel);
  std::vector<int64_t> rq(want_rel);
  EXPECT(flatten(want_rel, rz.data(), rs.data(), rq.data()) == SPX_OK && n_rel == want_rel && bad == 0);
  std::vector<uint8_t> qos(P), nn(P), nctr(P), kind(P * 8), cpresent(P * 8), ppresent(P);
  std::vector<int64_t> creq(P * 8 * n_res), preq(P * n_res);
  EXPECT(spx_flatten_nrt_pods(&pending_view, nullptr, &slots, qos.data(), nn.data(), nctr.data(), kind.data(), cpresent.data(), creq.data(), ppresent.data(), preq.data()) == SPX_OK);
  const spx_nrt_pods_soa pods{P, n_res, qos.data(), nn.data(), nctr.data(), kind.data(), cpresent.data(), creq.data(), ppresent.data(), preq.data()};
  spx_preempt_nrt_soa t{N, &slots, node_flags.data(), n_zones.data(), zid.data(), zpresent.data(), node_present.data(), avail.data(), room.data(), A, contributes.data(),
                        rel_ptr.data(), rz.data(), rs.data(), rq.data(), &pods};
  int32_t what = -1;
  EXPECT(spx_flatten_preempt_nrt_check(&t, &what, &bad) == SPX_OK && what == 0);
  room[5 * 8 * n_res] = -1;
  n_zones[5] = n_zones[5] ? n_zones[5] : 1;
  EXPECT(spx_flatten_preempt_nrt_check(&t, &what, &bad) == SPX_ERR_ARG && what == 1 && bad == 5);
  room[5 * 8 * n_res] = 0;

  // additivity: every pod of a node evicted at once, against the eviction simulation
  std::vector<uint8_t> vq(A);
  int checked = 0;
  for (int64_t n = 0; n < N; ++n) {
    // the node's pods as a victim table of their own (object order), with their containers' placements
    Pods v;
    std::vector<int32_t> vnuma;
    std::vector<int64_t> members;
    for (int64_t j = 0; j < A; ++j) {
      if (assigned_node[j] != n) continue;
      members.push_back(j);
      bool limits = assigned.lim_ptr[assigned.ctr_ptr[j] + 1] > assigned.lim_ptr[assigned.ctr_ptr[j]];
      for (int32_t c = assigned.ctr_ptr[j]; c < assigned.ctr_ptr[j + 1]; ++c) {
        std::vector<std::pair<int32_t, int64_t>> req;
        for (int32_t k = assigned.req_ptr[c]; k < assigned.req_ptr[c + 1]; ++k) req.push_back({assigned.req_res[k], assigned.req_qty[k]});
        v.container(SPX_CTR_APP, req, limits);
        vnuma.push_back(ctr_numa[c]);
      }
      v.end_pod();
    }
    if (members.empty()) continue;
    vnuma.push_back(0);
    const spx_pod_objects vv = v.view();
    for (size_t k = 0; k < members.size(); ++k) vq[k] = assigned.lim_ptr[assigned.ctr_ptr[members[k]] + 1] > assigned.lim_ptr[assigned.ctr_ptr[members[k]]] ? SPX_QOS_GUARANTEED : SPX_QOS_BURSTABLE;
    const int32_t e0 = zres_ptr[zone_ptr[n]], e1 = zres_ptr[zone_ptr[n + 1]];
    std::vector<int64_t> out(e1 - e0 + 1);
    int32_t code = -1;
    EXPECT(spx_nrt_post_eviction(&nrt, nullptr, n, &vv, vq.data(), vnuma.data(), placement_present[n], placement_containers[n], out.data(), &code) == SPX_OK);
    if (code != SPX_EVICT_OK && code != SPX_EVICT_EXCEEDS_ALLOCATABLE && code != SPX_EVICT_NOTHING_TO_ADD) continue;
    // the same from the table: the pods of node n are the table positions j with assigned_node[pod_src[j]] == n
    std::vector<int64_t> sum(8 * n_res, 0);
    int contributing = 0;
    for (int64_t j = 0; j < A; ++j) {
      if (assigned_node[pod_src[j]] != n) continue;
      contributing += contributes[j];
      for (int32_t k = rel_ptr[j]; k < rel_ptr[j + 1]; ++k) sum[rz[k] * n_res + rs[k]] += rq[k];
    }
    bool over = false;
    for (int e = 0; e < 8 * n_res; ++e) over |= sum[e] > room[n * 8 * n_res + e];
    const int32_t mine = contributing == 0 ? SPX_EVICT_NOTHING_TO_ADD : over ? SPX_EVICT_EXCEEDS_ALLOCATABLE : SPX_EVICT_OK;
    EXPECT(mine == code);
    if (code == SPX_EVICT_OK)
      for (int32_t z = zone_ptr[n]; z < zone_ptr[n + 1]; ++z)
        for (int32_t e = zres_ptr[z]; e < zres_ptr[z + 1]; ++e) {
          int s = 0;
          while (slot_res[s] != zres_res[e]) ++s;
          const int64_t at = (n * 8 + (z - zone_ptr[n])) * n_res + s;
          EXPECT(out[e - e0] == avail[at] + sum[(z - zone_ptr[n]) * n_res + s]);
        }
    ++checked;
  }
  EXPECT(checked > 20);
  std::printf("flatten_preempt_nrt: %lld assigned pods, %lld releases, %d nodes checked against the eviction simulation\n", static_cast<long long>(A),
              static_cast<long long>(want_rel), checked);
  return 0;
}
