"""Seeded synthetic cluster snapshots as object tables (numpy, vectorised, any scale).

Value distributions follow SURVEY.md §8d: node sizes mirror the reference benchmarks' 64-core
nodes (pkg/trimaran/targetloadpacking/targetloadpacking_test.go:452-456), pods are shaped like
the reference's test pods (1-3 app containers, optional init container, QoS mix).  The same
arrays feed the CPU oracle and, through the host flatteners, the GPU — that is the parity setup.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from ._abi import Header, Table

SEED = 20260921
GiB = 1 << 30
MiB = 1 << 20


def _csr_from_mask(mask: np.ndarray):
    """mask [n, slots] -> (ptr [n+1], flat selector) keeping row-major slot order."""
    counts = mask.sum(axis=1)
    ptr = np.zeros(mask.shape[0] + 1, dtype=np.int32)
    np.cumsum(counts, out=ptr[1:])
    return ptr, mask.reshape(-1)


def _csr_append(ptr: np.ndarray, cols, mask: np.ndarray, add):
    """a CSR structure with entries appended to each row: row r keeps its entries, then gains add[j][r, k] for every k with mask[r, k]
    (in k order).  cols / add: parallel value arrays.  Returns (new ptr, new value arrays)."""
    n = len(ptr) - 1
    old_cnt, new_cnt = np.diff(ptr).astype(np.int64), mask.sum(axis=1).astype(np.int64)
    nptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(old_cnt + new_cnt, out=nptr[1:])
    row_old = np.repeat(np.arange(n), old_cnt)
    pos_old = nptr[:-1][row_old] + (np.arange(len(row_old)) - ptr[:-1][row_old])
    row_new = np.repeat(np.arange(n), new_cnt)
    new_start = np.concatenate([[0], np.cumsum(new_cnt)[:-1]]).astype(np.int64)
    pos_new = nptr[:-1][row_new] + old_cnt[row_new] + (np.arange(len(row_new)) - new_start[row_new])
    sel = mask.reshape(-1)
    out = []
    for c, a in zip(cols, add):
        v = np.zeros(int(nptr[-1]), dtype=c.dtype)
        v[pos_old] = c
        v[pos_new] = a.reshape(-1)[sel]
        out.append(v)
    return nptr, out


RES_EXTRA0 = 12  # first id of nrt_snapshot(extra_res=...)'s resources


def extra_resource_is_hugepage(k: int) -> bool:
    """extra resource k (id RES_EXTRA0 + k): every third one a hugepage size, the others extended (SR-IOV / RDMA style) device pools"""
    return k % 3 == 1


def _widen_nrt(hdr: Header, nodes_scalar, nrt: Table, pods: Table, extra_res: int, seed: int, req_frac: float):
    """nrt_snapshot's extra resources, from their own random stream: reported by a random subset of node allocatables and zones,
    requested (request == limit, zero quantities included) by the first app container of a share req_frac of the pods"""
    rng = np.random.default_rng(seed + 207)
    ptr, res, qty = nodes_scalar
    N, K = len(ptr) - 1, extra_res
    ids = np.arange(RES_EXTRA0, RES_EXTRA0 + K, dtype=np.int32)
    hp = np.array([extra_resource_is_hugepage(k) for k in range(K)])
    node_has = rng.random((N, K)) < 0.8
    node_qty = np.where(hp[None, :], 64 * GiB, 8).astype(np.int64) * np.ones((N, 1), np.int64)
    sptr, (sres, sqty) = _csr_append(ptr, [res, qty], node_has, [np.tile(ids, (N, 1)), node_qty])
    # zones: a node that lists the resource reports it in most of its zones
    zone_ptr = nrt.array("zone_ptr")
    nzt = int(zone_ptr[-1])
    node_of = np.repeat(np.arange(N), np.diff(zone_ptr))
    z_has = (node_has & (rng.random((N, K)) < 0.75))[node_of] & (rng.random((nzt, K)) < 0.85)
    z_qty = np.where(hp[None, :], rng.integers(0, 9, (nzt, K)) * GiB, rng.integers(0, 5, (nzt, K))).astype(np.int64)
    zptr, (zres, zavail) = _csr_append(nrt.array("zres_ptr"), [nrt.array("zres_res"), nrt.array("zres_avail")], z_has, [np.tile(ids, (nzt, 1)), z_qty])
    fields = ("has_nrt", "fresh", "legacy_policy", "attr_scope", "attr_policy", "attr_max_numa", "zone_ptr", "zone_is_node", "zone_numa_id",
              "zcost_ptr", "zcost_numa_id", "zcost_value", "assumed_ptr", "arl_ptr", "arl_res", "arl_qty")
    nrt = Table(hdr, "spx_nrt_objects", n_nodes=N, zres_ptr=zptr, zres_res=zres, zres_avail=zavail, **{f: nrt.array(f) for f in fields})
    # pods: one to three extra resources in the first app container
    P = int(pods.struct.n_pods)
    cptr, kind = pods.array("ctr_ptr"), pods.array("ctr_kind")
    n_ctr = int(cptr[-1])
    first_app = np.full(P, -1, np.int64)
    for i in np.flatnonzero(rng.random(P) < req_frac):
        app = np.flatnonzero(kind[cptr[i]:cptr[i + 1]] == 0)
        if len(app):
            first_app[i] = cptr[i] + app[0]
    pick = np.zeros((P, K), bool)
    n_pick = rng.integers(1, 4, P)
    for i in np.flatnonzero(first_app >= 0):
        pick[i, rng.choice(K, min(K, int(n_pick[i])), replace=False)] = True
    c_has = np.zeros((n_ctr, K), bool)
    c_has[first_app[first_app >= 0]] = pick[first_app >= 0]
    c_qty = np.where(hp[None, :], rng.integers(0, 3, (n_ctr, K)) * GiB, rng.integers(0, 3, (n_ctr, K))).astype(np.int64)
    rptr, (rres, rqty) = _csr_append(pods.array("req_ptr"), [pods.array("req_res"), pods.array("req_qty")], c_has, [np.tile(ids, (n_ctr, 1)), c_qty])
    lptr, (lres, lqty) = _csr_append(pods.array("lim_ptr"), [pods.array("lim_res"), pods.array("lim_qty")], c_has, [np.tile(ids, (n_ctr, 1)), c_qty])
    pfields = ("ctr_ptr", "ctr_kind", "ovh_ptr", "ovh_res", "ovh_qty", "priority", "queue_ts", "appgroup", "selector", "ns")
    pods = Table(hdr, "spx_pod_objects", n_pods=P, req_ptr=rptr, req_res=rres, req_qty=rqty, lim_ptr=lptr, lim_res=lres, lim_qty=lqty,
                 **{f: pods.array(f) for f in pfields})
    return (sptr, sres, sqty), nrt, pods


def widen_snapshot(hdr: Header, snap: Dict[str, Table], extra_res: int, seed: int = SEED, req_frac: float = 0.15) -> Dict[str, Table]:
    """a snapshot (nrt_snapshot / full_snapshot keys) with nrt_snapshot(extra_res=...)'s extra resources added to its nodes, NRT objects,
    pods and resource classes; the other tables are shared"""
    nodes = snap["nodes"]
    scalar = (nodes.array("scalar_ptr"), nodes.array("scalar_res"), nodes.array("scalar_qty"))
    scalar, nrt, pods = _widen_nrt(hdr, scalar, snap["nrt"], snap["pods"], extra_res, seed, req_frac)
    nf = ("alloc_cpu_milli", "alloc_mem", "alloc_eph", "alloc_pods", "cap_cpu_milli", "region", "zone")
    out = dict(snap)
    out["nodes"] = Table(hdr, "spx_node_objects", n_nodes=int(nodes.struct.n_nodes), scalar_ptr=scalar[0], scalar_res=scalar[1],
                         scalar_qty=scalar[2], **{f: nodes.array(f) for f in nf})
    out["nrt"], out["pods"] = nrt, pods
    out["rc"] = nrt_resource_classes(hdr, False, extra_res)
    return out


def synth_pods(hdr: Header, n_pods: int, seed: int = SEED, device_res: int = -1, n_appgroups: int = 0,
               n_namespaces: int = 100, hugepage_res: int = -1, qos_p=(0.5, 0.4, 0.1), device2_res: int = -1, hugepage2_res: int = -1) -> Table:
    """`qos_p`: shares of Guaranteed / Burstable / BestEffort pods (50 / 40 / 10 %; experiments vary it).
    `device2_res` / `hugepage2_res`: a second extended resource and a second hugepage size (the six-slot NRT workload); their
    random streams are separate, so every other column is the same with or without them."""
    rng = np.random.default_rng(seed + 1)
    n_app = rng.integers(1, 4, n_pods)
    has_init = rng.random(n_pods) < 0.2
    n_ctr = n_app + has_init
    ctr_ptr = np.zeros(n_pods + 1, dtype=np.int32)
    np.cumsum(n_ctr, out=ctr_ptr[1:])
    total = int(ctr_ptr[-1])
    pod_of = np.repeat(np.arange(n_pods), n_ctr)
    pos = np.arange(total) - ctr_ptr[pod_of]
    kind = np.where(has_init[pod_of] & (pos == 0), 1, 0).astype(np.uint8)
    # 10% of init containers are sidecars
    kind = np.where((kind == 1) & (rng.random(total) < 0.1), 2, kind).astype(np.uint8)

    qos = rng.choice(3, n_pods, p=list(qos_p))  # 0 Guaranteed, 1 Burstable, 2 BestEffort
    q = qos[pod_of]
    cpu = np.exp(rng.uniform(np.log(100), np.log(8000), total)).astype(np.int64)
    whole = rng.random(total) < 0.3
    cpu = np.where(whole, np.maximum(1, (cpu + 500) // 1000) * 1000, cpu)
    mem = (np.exp(rng.uniform(np.log(64), np.log(32 * 1024), total)).astype(np.int64)) * MiB
    dev = (rng.random(n_pods) < 0.1)[pod_of] & (device_res >= 0) & (kind == 0) & (pos == has_init[pod_of])
    dev_n = rng.integers(1, 3, total)

    # requests: slots (cpu, memory, device, hugepages)
    rng_hp = np.random.default_rng(seed + 101)  # separate stream: keeps the other columns identical with/without hugepages
    hp = (rng_hp.random(total) < 0.15) & (hugepage_res >= 0) & (q != 2)
    hp_q = rng_hp.integers(0, 65, total).astype(np.int64) * (2 << 20)  # includes explicit zero-quantity requests
    bur_cpu = rng.random(total) < 0.8  # burstable containers may omit one of the two
    bur_mem = rng.random(total) < 0.8
    rng_w = np.random.default_rng(seed + 202)
    dev2 = (rng_w.random(n_pods) < 0.08)[pod_of] & (device2_res >= 0) & (kind == 0) & (pos == has_init[pod_of])
    dev2_n = rng_w.integers(1, 3, total)
    hp2 = (rng_w.random(total) < 0.08) & (hugepage2_res >= 0) & (q != 2)
    hp2_q = rng_w.integers(1, 5, total).astype(np.int64) * GiB
    req_mask = np.stack([(q == 0) | ((q == 1) & bur_cpu), (q == 0) | ((q == 1) & bur_mem), dev, hp, dev2, hp2], axis=1)
    req_res = np.tile(np.array([0, 1, max(device_res, 0), max(hugepage_res, 0), max(device2_res, 0), max(hugepage2_res, 0)], dtype=np.int32), (total, 1))
    req_qty = np.stack([cpu, mem, dev_n, hp_q, dev2_n, hp2_q], axis=1)
    req_ptr, sel = _csr_from_mask(req_mask)
    # limits: Guaranteed == requests; Burstable sometimes a larger cpu limit; devices/hugepages always limit == request
    bur_lim = (q == 1) & bur_cpu & (rng.random(total) < 0.5)
    lim_mask = np.stack([(q == 0) | bur_lim, (q == 0), dev, hp, dev2, hp2], axis=1)
    lim_qty = np.stack([np.where(q == 0, cpu, cpu * 2), mem, dev_n, hp_q, dev2_n, hp2_q], axis=1)
    lim_ptr, lsel = _csr_from_mask(lim_mask)

    ovh = rng.random(n_pods) < 0.05
    ovh_mask = np.stack([ovh, ovh & (rng.random(n_pods) < 0.5)], axis=1)
    ovh_qty = np.stack([rng.integers(50, 500, n_pods), rng.integers(16, 256, n_pods) * MiB], axis=1)
    ovh_res = np.tile(np.array([0, 1], dtype=np.int32), (n_pods, 1))
    ovh_ptr, osel = _csr_from_mask(ovh_mask)

    if n_appgroups > 0:
        appgroup = np.where(rng.random(n_pods) < 0.9, rng.integers(0, n_appgroups, n_pods), -1).astype(np.int32)
        selector = np.where(appgroup >= 0, rng.integers(0, 11, n_pods), -1).astype(np.int32)
    else:
        appgroup = np.full(n_pods, -1, dtype=np.int32)
        selector = np.full(n_pods, -1, dtype=np.int32)
    return Table(
        hdr, "spx_pod_objects", n_pods=n_pods, ctr_ptr=ctr_ptr, ctr_kind=kind,
        req_ptr=req_ptr, req_res=req_res.reshape(-1)[sel], req_qty=req_qty.reshape(-1)[sel],
        lim_ptr=lim_ptr, lim_res=req_res.reshape(-1)[lsel], lim_qty=lim_qty.reshape(-1)[lsel],
        ovh_ptr=ovh_ptr, ovh_res=ovh_res.reshape(-1)[osel], ovh_qty=ovh_qty.reshape(-1)[osel],
        priority=rng.choice(np.array([0, 100, 1000], dtype=np.int32), n_pods),
        queue_ts=np.arange(n_pods, dtype=np.int64) * 1000 + 1_700_000_000_000_000,
        appgroup=appgroup, selector=selector, ns=rng.integers(0, n_namespaces, n_pods).astype(np.int32),
    )



def _gather_csr(ptr: np.ndarray, idx: np.ndarray):
    """rows `idx` of a CSR structure: (new ptr, positions of the gathered entries in the old value arrays)"""
    cnt = (ptr[1:] - ptr[:-1])[idx]
    nptr = np.zeros(len(idx) + 1, dtype=np.int32)
    np.cumsum(cnt, out=nptr[1:])
    pos = np.repeat(ptr[:-1][idx] - nptr[:-1], cnt) + np.arange(int(nptr[-1]))
    return nptr, pos


def take_pods(hdr: Header, pods: Table, idx) -> Table:
    """The pod table made of rows `idx` of `pods`, in that order, repeats allowed: a queue of Deployment replicas is
    take_pods(templates, rng.integers(0, n_templates, n_pods)).  Queue timestamps are renumbered (they are per queue entry)."""
    idx = np.asarray(idx, dtype=np.int64)
    ctr_ptr, cpos = _gather_csr(pods.array("ctr_ptr"), idx)
    req_ptr, rpos = _gather_csr(pods.array("req_ptr"), cpos)
    lim_ptr, lpos = _gather_csr(pods.array("lim_ptr"), cpos)
    ovh_ptr, opos = _gather_csr(pods.array("ovh_ptr"), idx)
    return Table(
        hdr, "spx_pod_objects", n_pods=len(idx), ctr_ptr=ctr_ptr, ctr_kind=pods.array("ctr_kind")[cpos],
        req_ptr=req_ptr, req_res=pods.array("req_res")[rpos], req_qty=pods.array("req_qty")[rpos],
        lim_ptr=lim_ptr, lim_res=pods.array("lim_res")[lpos], lim_qty=pods.array("lim_qty")[lpos],
        ovh_ptr=ovh_ptr, ovh_res=pods.array("ovh_res")[opos], ovh_qty=pods.array("ovh_qty")[opos],
        priority=pods.array("priority")[idx], queue_ts=np.arange(len(idx), dtype=np.int64) * 1000 + 1_700_000_000_000_000,
        appgroup=pods.array("appgroup")[idx], selector=pods.array("selector")[idx], ns=pods.array("ns")[idx],
    )


def lengthen_pods(hdr: Header, pods: Table, frac: float = 0.0, seed: int = SEED, lo: int = 9, hi: int = 40, rows=None) -> Table:
    """The pod table with a share `frac` of its pods (or the pods `rows`) made "long" for NodeResourceTopologyMatch: lo..hi containers
    each (more than the dense NRT table's 8), copies of the pod's own containers taken in turn with every quantity divided by a third of
    the count (so that some still fit a zone); up to three init containers lead, a third of them sidecars.  Requests equal limits
    wherever they did, so each pod keeps its QoS class.  Other pods and columns are unchanged."""
    rng = np.random.default_rng(seed + 303)
    P = int(pods.struct.n_pods)
    if rows is None:
        rows = np.flatnonzero(rng.random(P) < frac)
    chosen = np.zeros(P, bool)
    chosen[np.asarray(rows, dtype=np.int64)] = True
    ptr, kind = pods.array("ctr_ptr"), pods.array("ctr_kind")
    src, kinds, div = [], [], []
    counts = np.zeros(P, np.int64)
    for i in range(P):
        own = np.arange(ptr[i], ptr[i + 1])
        if not chosen[i] or len(own) == 0:
            src.extend(own), kinds.extend(kind[own]), div.extend([1] * len(own))
            counts[i] = len(own)
            continue
        n = int(rng.integers(lo, hi + 1))
        n_init = int(rng.integers(0, 4))
        k = np.zeros(n, np.uint8)
        k[:n_init] = np.where(rng.random(n_init) < 1 / 3, 2, 1)
        src.extend(own[np.arange(n) % len(own)]), kinds.extend(k), div.extend([max(1, n // 3)] * n)
        counts[i] = n
    src, div = np.asarray(src, np.int64), np.asarray(div, np.int64)
    ctr_ptr = np.zeros(P + 1, np.int32)
    np.cumsum(counts, out=ctr_ptr[1:])
    req_ptr, rpos = _gather_csr(pods.array("req_ptr"), src)
    lim_ptr, lpos = _gather_csr(pods.array("lim_ptr"), src)
    rdiv, ldiv = np.repeat(div, np.diff(req_ptr)), np.repeat(div, np.diff(lim_ptr))
    return Table(
        hdr, "spx_pod_objects", n_pods=P, ctr_ptr=ctr_ptr, ctr_kind=np.asarray(kinds, np.uint8),
        req_ptr=req_ptr, req_res=pods.array("req_res")[rpos], req_qty=pods.array("req_qty")[rpos] // rdiv,
        lim_ptr=lim_ptr, lim_res=pods.array("lim_res")[lpos], lim_qty=pods.array("lim_qty")[lpos] // ldiv,
        ovh_ptr=pods.array("ovh_ptr"), ovh_res=pods.array("ovh_res"), ovh_qty=pods.array("ovh_qty"),
        priority=pods.array("priority"), queue_ts=pods.array("queue_ts"), appgroup=pods.array("appgroup"), selector=pods.array("selector"),
        ns=pods.array("ns"),
    )


def synth_nodes(hdr: Header, n_nodes: int, seed: int = SEED, device_res: int = -1, n_regions: int = 8,
                zones_per_region: int = 8) -> Table:
    rng = np.random.default_rng(seed + 2)
    cpu = rng.choice(np.array([8, 16, 32, 64, 96, 128], dtype=np.int64), n_nodes) * 1000
    mem = rng.choice(np.array([32, 64, 128, 256, 346, 512, 1024], dtype=np.int64), n_nodes) * GiB
    reserved = rng.integers(500, 2001, n_nodes)
    has_dev = (rng.random(n_nodes) < 0.5) & (device_res >= 0)
    sc_mask = has_dev.reshape(-1, 1)
    sc_ptr, ssel = _csr_from_mask(sc_mask)
    region = rng.integers(0, n_regions, n_nodes).astype(np.int32)
    zone = (region * zones_per_region + rng.integers(0, zones_per_region, n_nodes)).astype(np.int32)
    unl = rng.random(n_nodes) < 0.01
    region = np.where(unl, -1, region).astype(np.int32)
    zone = np.where(unl, -1, zone).astype(np.int32)
    return Table(
        hdr, "spx_node_objects", n_nodes=n_nodes,
        alloc_cpu_milli=cpu - reserved, alloc_mem=mem - 2 * GiB, alloc_eph=np.full(n_nodes, 500 * GiB, dtype=np.int64),
        alloc_pods=np.full(n_nodes, 110, dtype=np.int64),
        scalar_ptr=sc_ptr, scalar_res=np.full(n_nodes, max(device_res, 0), dtype=np.int32)[ssel],
        scalar_qty=rng.integers(1, 9, n_nodes)[ssel],
        cap_cpu_milli=cpu, region=region, zone=zone,
    )


def synth_metrics(hdr: Header, n_nodes: int, seed: int = SEED, window_end: int = 1_700_000_000,
                  round_frac: float = 0.0) -> Table:
    """Per node up to 6 metric slots in a fixed order that exercises SURVEY appendix B.5:
    [CPU AVG, CPU STD, CPU Latest, Memory AVG, Memory STD, Memory ""].  TLP takes the LAST of
    CPU AVG/Latest, LVRB prefers AVG regardless of order."""
    rng = np.random.default_rng(seed + 3)
    present = rng.random(n_nodes) >= 0.02
    nil = present & (rng.random(n_nodes) < 0.005)
    r = rng.random((n_nodes, 6))
    mask = np.stack([r[:, 0] < 0.9, r[:, 1] < 0.8, r[:, 2] < 0.3, r[:, 3] < 0.85, r[:, 4] < 0.7, r[:, 5] < 0.2], axis=1)
    mask &= (present & ~nil).reshape(-1, 1)
    mtype = np.tile(np.array([0, 0, 0, 1, 1, 1], dtype=np.uint8), (n_nodes, 1))
    mop = np.tile(np.array([0, 1, 2, 0, 1, 3], dtype=np.uint8), (n_nodes, 1))
    val = np.stack([rng.uniform(0, 100, n_nodes), rng.uniform(0, 30, n_nodes), rng.uniform(0, 100, n_nodes),
                    rng.uniform(0, 100, n_nodes), rng.uniform(0, 30, n_nodes), rng.uniform(0, 100, n_nodes)], axis=1)
    # optional slice of round values that land exactly on rounding ties / threshold boundaries (tests);
    # SURVEY.md §8d's distribution itself is continuous: cpu_util% ~ U[0,100)
    rnd = rng.random(n_nodes) < round_frac
    val = np.where(rnd.reshape(-1, 1), np.round(val), val)
    ptr, sel = _csr_from_mask(mask)
    return Table(hdr, "spx_metrics_objects", map_is_nil=0, window_end=window_end,
                 node_present=present.astype(np.uint8), node_metrics_nil=nil.astype(np.uint8), m_ptr=ptr,
                 m_type=mtype.reshape(-1)[sel], m_op=mop.reshape(-1)[sel], m_value=val.reshape(-1)[sel])


def synth_assigned(hdr: Header, n_nodes: int, seed: int = SEED, window_end: int = 1_700_000_000) -> Table:
    """ScheduledPodsCache: 10% of nodes hold 1-3 recently bound pods with timestamps straddling the
    metrics window end (both sides of the 60 s rule, targetloadpacking.go:158-159)."""
    rng = np.random.default_rng(seed + 4)
    cnt = np.where(rng.random(n_nodes) < 0.1, rng.integers(1, 4, n_nodes), 0)
    e_ptr = np.zeros(n_nodes + 1, dtype=np.int32)
    np.cumsum(cnt, out=e_ptr[1:])
    n_e = int(e_ptr[-1])
    ts = window_end + rng.integers(-200, 100, n_e)
    pods = synth_pods(hdr, max(n_e, 1), seed=seed + 77)
    return Table(hdr, "spx_assigned_objects", e_ptr=e_ptr, e_ts_unix=ts.astype(np.int64),
                 e_pod=np.arange(n_e, dtype=np.int32), pods=pods)


def synth_node_pods(hdr: Header, n_nodes: int, seed: int = SEED, max_pods: int = 12) -> Table:
    """framework.NodeInfo.GetPods(): 0..max_pods-1 pods already running per node, drawn like the pending pods (so a
    share of Burstable pods carries cpu limits of twice the request: small nodes end up over-committed on limits, large
    ones do not — both sides of lowriskovercommitment.go:206)."""
    rng = np.random.default_rng(seed + 5)
    cnt = rng.integers(0, max_pods, n_nodes)
    p_ptr = np.zeros(n_nodes + 1, dtype=np.int32)
    np.cumsum(cnt, out=p_ptr[1:])
    n_p = int(p_ptr[-1])
    return Table(hdr, "spx_node_pods_objects", p_ptr=p_ptr, p_pod=np.arange(n_p, dtype=np.int32),
                 pods=synth_pods(hdr, max(n_p, 1), seed=seed + 55))


def synth_power_models(hdr: Header, n_nodes: int, seed: int = SEED) -> Table:
    """PeaksArgs.NodePowerModel: Power = K0 + K1 * e^(K2 * utilisation) with K1, K2 < 0 around the reference's fixture
    (peaks_test.go:80-86); 5% of the nodes have no entry (getPowerModel then yields the zero model, peaks.go:190-196)."""
    rng = np.random.default_rng(seed + 6)
    has = rng.random(n_nodes) >= 0.05
    k0 = np.where(has, rng.uniform(300, 600, n_nodes), 0.0)
    k1 = np.where(has, -rng.uniform(40, 160, n_nodes), 0.0)
    k2 = np.where(has, -rng.uniform(0.02, 0.12, n_nodes), 0.0)
    return Table(hdr, "spx_power_model_objects", k0=k0, k1=k1, k2=k2)


def resource_classes(hdr: Header, flags: Optional[np.ndarray] = None) -> Table:
    if flags is None:
        flags = np.zeros(8, dtype=np.uint8)
        flags[[0, 1, 2, 3, 4]] = 2  # native
    return Table(hdr, "spx_resource_classes", n_res=len(flags), flags=flags)


def trimaran_snapshot(hdr: Header, n_nodes: int, n_pods: int, seed: int = SEED, round_frac: float = 0.0,
                      with_node_pods: bool = False) -> Dict[str, Table]:
    """Object tables for BASELINE.json config #2 (Allocatable + TargetLoadPacking [+ LVRB]); with_node_pods adds the pods
    already running on every node, which LowRiskOverCommitment sums."""
    snap = {
        "nodes": synth_nodes(hdr, n_nodes, seed),
        "pods": synth_pods(hdr, n_pods, seed),
        "metrics": synth_metrics(hdr, n_nodes, seed, round_frac=round_frac),
        "assigned": synth_assigned(hdr, n_nodes, seed),
        "rc": resource_classes(hdr),
    }
    if with_node_pods:
        snap["node_pods"] = synth_node_pods(hdr, n_nodes, seed)
    return snap


# ------------------------------------------------------------------ NodeResourceTopology (config #3)
RES_HUGEPAGES_2MI = 8   # "hugepages-2Mi"
RES_DEVICE = 9          # "example.com/gpu" style extended resource
RES_HUGEPAGES_1GI = 10  # "hugepages-1Gi"      (the six-slot workload: a cluster with two hugepage sizes and two device types)
RES_DEVICE2 = 11        # a second extended resource


def nrt_resource_classes(hdr: Header, wide: bool = False, extra_res: int = 0) -> Table:
    flags = np.zeros(RES_EXTRA0 + extra_res if extra_res else (12 if wide else 10), dtype=np.uint8)
    flags[[0, 1, 2, 3, 4]] = 2              # native
    flags[RES_HUGEPAGES_2MI] = 1 | 2 | 4    # hugepage, native, scalar
    flags[RES_DEVICE] = 4                   # extended: not native, scalar
    if wide:
        flags[RES_HUGEPAGES_1GI] = 1 | 2 | 4
        flags[RES_DEVICE2] = 4
    for k in range(extra_res):
        flags[RES_EXTRA0 + k] = (1 | 2 | 4) if extra_resource_is_hugepage(k) else 4
    return Table(hdr, "spx_resource_classes", n_res=len(flags), flags=flags)


def synth_nrt(hdr: Header, nodes: Table, seed: int = SEED, n_zones: int = 8, vary: bool = True, wide: bool = False,
              tall_frac: float = 0.0, tall_zones=(9, 16), tall_control: bool = False):
    """NRT objects for the given nodes: Z NUMA zones per node with ids == list positions,
    per-zone available = alloc/Z x U[0.1,1] for {cpu, memory, hugepages-2Mi, device}; distances 10 on the
    diagonal and {12,20,32} off it; single-numa-node policy, container scope 70% / pod scope 30%,
    1% of nodes without NRT, 1% stale.  `vary` adds the ragged cases the reference tests cover: fewer zones,
    zones that do not report the device, missing cost entries, non-single-numa policies, assumed pods."""
    rng = np.random.default_rng(seed + 5)
    N = nodes.struct.n_nodes
    cpu = nodes.array("alloc_cpu_milli")
    mem = nodes.array("alloc_mem")
    has = rng.random(N) >= 0.01
    fresh = rng.random(N) >= 0.01
    nz = np.full(N, n_zones)
    if vary:
        nz = np.where(rng.random(N) < 0.15, rng.choice(np.array([1, 2, 4]), N), nz)
    nz = np.where(has, nz, 0)
    zone_ptr = np.zeros(N + 1, dtype=np.int32)
    np.cumsum(nz, out=zone_ptr[1:])
    nzt = int(zone_ptr[-1])
    node_of = np.repeat(np.arange(N), nz)
    zpos = np.arange(nzt) - zone_ptr[node_of]
    frac = rng.uniform(0.1, 1.0, (nzt, 4))
    z_cpu = (cpu[node_of] / nz[node_of] * frac[:, 0]).astype(np.int64)
    whole = rng.random(nzt) < 0.5
    z_cpu = np.where(whole, (z_cpu // 1000) * 1000, z_cpu)
    z_mem = (mem[node_of] / nz[node_of] * frac[:, 1]).astype(np.int64)
    z_hp = (rng.integers(0, 513, nzt) * (2 << 20)).astype(np.int64)
    z_dev = rng.integers(0, 5, nzt).astype(np.int64)
    node_has_dev = rng.random(N) < 0.6
    rep_dev = node_has_dev[node_of] & ((rng.random(nzt) < 0.85) if vary else True)
    rep_hp = (rng.random(N) < 0.8)[node_of]
    mask = np.stack([np.ones(nzt, bool), np.ones(nzt, bool), rep_hp, rep_dev], axis=1)
    res = np.tile(np.array([0, 1, RES_HUGEPAGES_2MI, RES_DEVICE], dtype=np.int32), (nzt, 1))
    qty = np.stack([z_cpu, z_mem, z_hp, z_dev], axis=1)
    if wide:  # two more zone resources, from their own stream (the four above stay as they are)
        rng_w = np.random.default_rng(seed + 205)
        z_hp1g = (rng_w.integers(0, 9, nzt) * GiB).astype(np.int64)
        z_dev2 = rng_w.integers(0, 3, nzt).astype(np.int64)
        rep_hp1g = (rng_w.random(N) < 0.7)[node_of]
        rep_dev2 = (rng_w.random(N) < 0.5)[node_of] & (rng_w.random(nzt) < 0.9)
        mask = np.concatenate([mask, np.stack([rep_hp1g, rep_dev2], axis=1)], axis=1)
        res = np.tile(np.array([0, 1, RES_HUGEPAGES_2MI, RES_DEVICE, RES_HUGEPAGES_1GI, RES_DEVICE2], dtype=np.int32), (nzt, 1))
        qty = np.concatenate([qty, np.stack([z_hp1g, z_dev2], axis=1)], axis=1)
    zres_ptr, sel = _csr_from_mask(mask)
    # costs: full matrix per node, 5% of entries dropped when vary
    cnt = nz[node_of]
    cost_ptr = np.zeros(nzt + 1, dtype=np.int32)
    cmask = np.arange(8)[None, :] < cnt[:, None]
    if vary:
        cmask &= rng.random((nzt, 8)) >= 0.05
    tgt = np.tile(np.arange(8, dtype=np.int32), (nzt, 1))
    off = rng.choice(np.array([12, 20, 32]), (N, 8, 8))
    off = np.minimum(off, off.transpose(0, 2, 1))
    cval = np.where(tgt == zpos[:, None], 10, off[node_of[:, None], np.minimum(zpos, 7)[:, None], tgt])
    np.cumsum(cmask.sum(axis=1), out=cost_ptr[1:])
    csel = cmask.reshape(-1)
    # policies
    pod_scope = rng.random(N) < 0.3
    legacy = np.where(pod_scope, (3 << 1) | 1, (3 << 1) | 0).astype(np.int8)
    attr_scope = np.full(N, -1, dtype=np.int8)
    attr_policy = np.full(N, -1, dtype=np.int8)
    attr_max = np.full(N, -1, dtype=np.int32)
    if vary:
        other = rng.random(N) < 0.06
        legacy = np.where(other, rng.choice(np.array([-1, (1 << 1) | 0, (2 << 1) | 1], dtype=np.int8), N), legacy).astype(np.int8)
        via_attr = rng.random(N) < 0.1   # attributes override the legacy field
        attr_policy = np.where(via_attr, 3, attr_policy).astype(np.int8)
        attr_scope = np.where(via_attr, rng.integers(0, 2, N), attr_scope).astype(np.int8)
        attr_max = np.where(rng.random(N) < 0.1, rng.choice(np.array([4, 8, 16]), N), attr_max).astype(np.int32)
    # assumed pods (OverReserve): 5% of nodes carry 1-2 assumed pods
    acnt = np.where((rng.random(N) < 0.05) & has & vary, rng.integers(1, 3, N), 0)
    assumed_ptr = np.zeros(N + 1, dtype=np.int32)
    np.cumsum(acnt, out=assumed_ptr[1:])
    na = int(assumed_ptr[-1])
    arl_ptr = np.arange(na + 1, dtype=np.int32) * 2
    arl_res = np.tile(np.array([0, 1], dtype=np.int32), na)
    arl_qty = np.stack([rng.integers(500, 4000, na), rng.integers(1, 16, na) * GiB], axis=1).reshape(-1)
    out = Table(
        hdr, "spx_nrt_objects", n_nodes=N, has_nrt=has.astype(np.uint8), fresh=fresh.astype(np.uint8),
        legacy_policy=legacy, attr_scope=attr_scope, attr_policy=attr_policy, attr_max_numa=attr_max,
        zone_ptr=zone_ptr, zone_is_node=np.ones(nzt, dtype=np.uint8), zone_numa_id=zpos.astype(np.int32),
        zres_ptr=zres_ptr, zres_res=res.reshape(-1)[sel], zres_avail=qty.reshape(-1)[sel],
        zcost_ptr=cost_ptr, zcost_numa_id=tgt.reshape(-1)[csel], zcost_value=cval.reshape(-1)[csel].astype(np.int64),
        assumed_ptr=assumed_ptr, arl_ptr=arl_ptr, arl_res=arl_res, arl_qty=arl_qty.astype(np.int64),
    )
    # `tall_frac`: that share of the nodes gets tall_zones[0]..tall_zones[1] zones (heighten_nrt, its own stream); 0 leaves the objects
    # as they always were.  `tall_control`: the same nodes lose their NRT object instead.
    return heighten_nrt(hdr, nodes, out, tall_frac, tall_zones, seed, drop_nrt=tall_control) if tall_frac > 0 else out


def heighten_nrt(hdr: Header, nodes: Table, nrt: Table, frac: float = 0.0, zones=(9, 16), seed: int = SEED, rows=None, drop_nrt: bool = False) -> Table:
    """The NRT objects with a share `frac` of the nodes that have an NRT object (or the nodes `rows`) made "tall" for
    NodeResourceTopologyMatch: zones[0]..zones[1] zones each (more than the dense NRT table's 8) reporting cpu, memory,
    hugepages-2Mi and — on 85 % of the zones — the device, available = alloc / Z x U[0.1, 1]; distances 10 on the diagonal and
    {12, 20, 32} off it with 5 % of the entries missing; on a third of the tall nodes the ids are a permutation of the positions.
    Policies, freshness and assumed pods stay the node's own.  The draws come from their own stream, so the other nodes' objects
    are those of the input.  `drop_nrt`: the chosen nodes lose their NRT object instead (the control a tall snapshot is compared to)."""
    rng = np.random.default_rng(seed + 404)
    N = nrt.struct.n_nodes
    has = nrt.array("has_nrt").astype(bool)
    if rows is None:
        pick = has & (rng.random(N) < frac)
    else:
        pick = np.zeros(N, bool)
        pick[np.asarray(rows, dtype=np.int64)] = True
    tz = np.where(pick, rng.integers(zones[0], zones[1] + 1, N), 0)
    if drop_nrt:
        tz[:] = 0
    zone_ptr = nrt.array("zone_ptr")
    old_cnt = np.where(pick, 0, zone_ptr[1:] - zone_ptr[:-1])
    keep = np.flatnonzero(~pick[np.repeat(np.arange(N), zone_ptr[1:] - zone_ptr[:-1])])  # old zones that stay
    # the tall nodes' zones
    nt = int(tz.sum())
    t_node = np.repeat(np.arange(N), tz)
    t_first = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(tz, out=t_first[1:])
    t_pos = np.arange(nt) - t_first[t_node]
    t_cnt = tz[t_node]
    t_id = t_pos.copy()
    for n in np.flatnonzero(tz > 0):
        if rng.random() < 1 / 3:
            t_id[t_first[n]:t_first[n + 1]] = rng.permutation(int(tz[n]))
    fr = rng.uniform(0.1, 1.0, (nt, 2))
    z_cpu = (nodes.array("alloc_cpu_milli")[t_node] / np.maximum(t_cnt, 1) * fr[:, 0]).astype(np.int64)
    z_cpu = np.where(rng.random(nt) < 0.5, (z_cpu // 1000) * 1000, z_cpu)
    z_mem = (nodes.array("alloc_mem")[t_node] / np.maximum(t_cnt, 1) * fr[:, 1]).astype(np.int64)
    z_hp = (rng.integers(0, 513, nt) * (2 << 20)).astype(np.int64)
    z_dev = rng.integers(0, 5, nt).astype(np.int64)
    t_mask = np.stack([np.ones(nt, bool), np.ones(nt, bool), np.ones(nt, bool), rng.random(nt) < 0.85], axis=1)
    t_rptr, t_rsel = _csr_from_mask(t_mask)
    t_res = np.tile(np.array([0, 1, RES_HUGEPAGES_2MI, RES_DEVICE], dtype=np.int32), (nt, 1)).reshape(-1)[t_rsel]
    t_qty = np.stack([z_cpu, z_mem, z_hp, z_dev], axis=1).reshape(-1)[t_rsel]
    zmax = int(zones[1])
    col = np.arange(zmax)[None, :]
    t_cmask = (col < t_cnt[:, None]) & (rng.random((nt, zmax)) >= 0.05)
    off = rng.choice(np.array([12, 20, 32]), (nt, zmax))
    t_cval = np.where(col == t_pos[:, None], 10, off)
    t_ctgt = np.zeros((nt, zmax), dtype=np.int32)
    for n in np.flatnonzero(tz > 0):  # column c of a zone's costs names the id of the zone at position c
        k = int(tz[n])
        t_ctgt[t_first[n]:t_first[n + 1], :k] = t_id[t_first[n]:t_first[n + 1]][None, :]
    t_cptr, t_csel = _csr_from_mask(t_cmask)
    # merged zone order: node-major, a node's zones in list order
    new_cnt = old_cnt + tz
    new_ptr = np.zeros(N + 1, dtype=np.int32)
    np.cumsum(new_cnt, out=new_ptr[1:])
    n_keep = len(keep)
    key_node = np.concatenate([np.repeat(np.arange(N), old_cnt), t_node])
    order = np.argsort(key_node, kind="stable")  # (a node has kept zones or tall zones, never both: list order survives)
    src_old = order < n_keep

    def merge_zone(old_vals, tall_vals):
        return np.concatenate([old_vals[keep], tall_vals])[order]

    def merge_csr(old_ptr, old_cols, tall_ptr, tall_cols):
        optr, opos = _gather_csr(old_ptr, keep)
        cnt = np.concatenate([optr[1:] - optr[:-1], tall_ptr[1:] - tall_ptr[:-1]])
        both_ptr = np.zeros(len(cnt) + 1, dtype=np.int32)
        np.cumsum(cnt, out=both_ptr[1:])
        nptr, pos = _gather_csr(both_ptr, order)
        return nptr, [np.concatenate([oc[opos], tc])[pos] for oc, tc in zip(old_cols, tall_cols)]

    zres_ptr, (zres_res, zres_avail) = merge_csr(nrt.array("zres_ptr"), [nrt.array("zres_res"), nrt.array("zres_avail")], t_rptr, [t_res, t_qty])
    zcost_ptr, (zcost_id, zcost_val) = merge_csr(nrt.array("zcost_ptr"), [nrt.array("zcost_numa_id"), nrt.array("zcost_value")], t_cptr,
                                                 [t_ctgt.reshape(-1)[t_csel], t_cval.reshape(-1)[t_csel].astype(np.int64)])
    del src_old
    has_new = has & ~pick if drop_nrt else has
    return Table(
        hdr, "spx_nrt_objects", n_nodes=N, has_nrt=has_new.astype(np.uint8), fresh=nrt.array("fresh"),
        legacy_policy=nrt.array("legacy_policy"), attr_scope=nrt.array("attr_scope"), attr_policy=nrt.array("attr_policy"),
        attr_max_numa=nrt.array("attr_max_numa"), zone_ptr=new_ptr, zone_is_node=merge_zone(nrt.array("zone_is_node"), np.ones(nt, np.uint8)),
        zone_numa_id=merge_zone(nrt.array("zone_numa_id"), t_id.astype(np.int32)),
        zres_ptr=zres_ptr, zres_res=zres_res.astype(np.int32), zres_avail=zres_avail.astype(np.int64),
        zcost_ptr=zcost_ptr, zcost_numa_id=zcost_id.astype(np.int32), zcost_value=zcost_val.astype(np.int64),
        assumed_ptr=nrt.array("assumed_ptr"), arl_ptr=nrt.array("arl_ptr"), arl_res=nrt.array("arl_res"), arl_qty=nrt.array("arl_qty"),
    )


def nrt_snapshot(hdr: Header, n_nodes: int, n_pods: int, seed: int = SEED, vary: bool = True, wide: bool = False,
                 long_frac: float = 0.0, long_ctrs=(9, 40), extra_res: int = 0, extra_req_frac: float = 0.15,
                 tall_frac: float = 0.0, tall_zones=(9, 16), tall_control: bool = False) -> Dict[str, Table]:
    """Object tables for BASELINE.json config #3 (NRT Filter+Score, 8 NUMA zones).  `wide`: six resource slots (cpu, memory,
    hugepages-2Mi, hugepages-1Gi, two extended resources) instead of four — the kernels' 8-slot instantiations.  `long_frac`: that
    share of the pods gets long_ctrs[0]..long_ctrs[1] containers (lengthen_pods); 0 leaves the snapshot as it always was.
    `extra_res`: that many more resources (ids RES_EXTRA0.., hugepage sizes and extended device pools) reported by a random subset of
    node allocatables and zones and requested by a share extra_req_frac of the pods (_widen_nrt); 0 leaves the snapshot unchanged.
    `tall_frac`: that share of the nodes lists tall_zones[0]..tall_zones[1] NUMA zones (heighten_nrt; `tall_control`: they have no NRT
    object instead); 0 leaves the snapshot unchanged."""
    nodes = synth_nodes(hdr, n_nodes, seed, device_res=RES_DEVICE)
    # node-level allocatable must list hugepages too (util.ResourceList key check, filter.go:110-116)
    rng = np.random.default_rng(seed + 6)
    N = n_nodes
    has_hp = rng.random(N) < 0.9
    has_dev = rng.random(N) < 0.7
    mask = np.stack([has_hp, has_dev], axis=1)
    res = np.tile(np.array([RES_HUGEPAGES_2MI, RES_DEVICE], dtype=np.int32), (N, 1))
    qty = np.stack([np.full(N, 1 << 30, dtype=np.int64), rng.integers(1, 17, N)], axis=1)
    if wide:
        rng_w = np.random.default_rng(seed + 206)
        mask = np.concatenate([mask, np.stack([rng_w.random(N) < 0.85, rng_w.random(N) < 0.6], axis=1)], axis=1)
        res = np.tile(np.array([RES_HUGEPAGES_2MI, RES_DEVICE, RES_HUGEPAGES_1GI, RES_DEVICE2], dtype=np.int32), (N, 1))
        qty = np.concatenate([qty, np.stack([np.full(N, 64 * GiB, dtype=np.int64), rng_w.integers(1, 9, N)], axis=1)], axis=1)
    ptr, sel = _csr_from_mask(mask)
    pods = synth_pods(hdr, n_pods, seed, device_res=RES_DEVICE, hugepage_res=RES_HUGEPAGES_2MI,
                      device2_res=RES_DEVICE2 if wide else -1, hugepage2_res=RES_HUGEPAGES_1GI if wide else -1)
    if long_frac > 0:
        pods = lengthen_pods(hdr, pods, long_frac, seed, *long_ctrs)
    scalar = (ptr, res.reshape(-1)[sel], qty.reshape(-1)[sel])
    nrt = synth_nrt(hdr, nodes, seed, vary=vary, wide=wide, tall_frac=tall_frac, tall_zones=tall_zones, tall_control=tall_control)
    if extra_res > 0:
        scalar, nrt, pods = _widen_nrt(hdr, scalar, nrt, pods, extra_res, seed, extra_req_frac)
    nodes = Table(hdr, "spx_node_objects", n_nodes=N, alloc_cpu_milli=nodes.array("alloc_cpu_milli"),
                  alloc_mem=nodes.array("alloc_mem"), alloc_eph=nodes.array("alloc_eph"), alloc_pods=nodes.array("alloc_pods"),
                  scalar_ptr=scalar[0], scalar_res=scalar[1], scalar_qty=scalar[2],
                  cap_cpu_milli=nodes.array("cap_cpu_milli"), region=nodes.array("region"), zone=nodes.array("zone"))
    return {
        "nodes": nodes,
        "pods": pods,
        "nrt": nrt,
        "rc": nrt_resource_classes(hdr, wide, extra_res),
    }


# ------------------------------------------------------------------ network-aware (config #4)
def synth_network(hdr: Header, nodes: Table, n_groups: int, seed: int = SEED, n_regions: int = 8, zones_per_region: int = 8,
                  placed_per_group: int = 10):
    """AppGroup + NetworkTopology objects: AppGroups of 11 workloads shaped like onlineboutique
    (networkoverhead_test.go:226-307) with D in [0,7] dependencies each and MaxNetworkCost in {5,10,20,50,100};
    10 already-placed pods per group on random nodes (as the reference benchmarks, :359-370); a 3-tier topology:
    dense zone->zone costs in [1,50] inside a region with 5% of entries missing, region->region in [20,100]."""
    rng = np.random.default_rng(seed + 7)
    N = nodes.struct.n_nodes
    W = 11
    G = n_groups
    n_wl = G * W
    wl_ptr = np.arange(G + 1, dtype=np.int32) * W
    wl_selector = np.tile(np.arange(W, dtype=np.int32), G)
    nd = rng.integers(0, 8, n_wl)
    nd = np.where(rng.random(n_wl) < 0.5, 0, nd)  # most workloads of onlineboutique have no dependencies
    dep_ptr = np.zeros(n_wl + 1, dtype=np.int32)
    np.cumsum(nd, out=dep_ptr[1:])
    n_dep = int(dep_ptr[-1])
    dep_selector = rng.integers(0, W, n_dep).astype(np.int32)
    dep_max = rng.choice(np.array([5, 10, 20, 50, 100], dtype=np.int64), n_dep)
    topo_ptr = wl_ptr.copy()
    topo_selector = wl_selector.copy()  # sorted by selector, as the controller writes it
    topo_index = (np.argsort(rng.random((G, W)), axis=1) + 1).astype(np.int32).reshape(-1)
    S = placed_per_group
    placed_ptr = np.arange(G + 1, dtype=np.int32) * S
    placed_selector = rng.integers(0, W, G * S).astype(np.int32)
    placed_node = rng.integers(0, N, G * S).astype(np.int32)
    ag = Table(hdr, "spx_appgroup_objects", n_groups=G, wl_ptr=wl_ptr, wl_selector=wl_selector, dep_ptr=dep_ptr,
               dep_selector=dep_selector, dep_max_cost=dep_max, topo_ptr=topo_ptr, topo_selector=topo_selector,
               topo_index=topo_index, placed_ptr=placed_ptr, placed_selector=placed_selector, placed_node=placed_node)
    Rg, Zc = n_regions, n_regions * zones_per_region
    rmask = ~np.eye(Rg, dtype=bool)
    rc_ptr, rsel = _csr_from_mask(rmask)
    rdest = np.tile(np.arange(Rg, dtype=np.int32), (Rg, 1))
    rcost = rng.integers(20, 101, (Rg, Rg))
    same_region = (np.arange(Zc)[:, None] // zones_per_region) == (np.arange(Zc)[None, :] // zones_per_region)
    zmask = same_region & ~np.eye(Zc, dtype=bool) & (rng.random((Zc, Zc)) >= 0.05)
    zc_ptr, zsel = _csr_from_mask(zmask)
    zdest = np.tile(np.arange(Zc, dtype=np.int32), (Zc, 1))
    zcost = rng.integers(1, 51, (Zc, Zc))
    nt = Table(hdr, "spx_nettopo_objects", n_regions=Rg, n_zones=Zc, rc_ptr=rc_ptr, rc_dest=rdest.reshape(-1)[rsel],
               rc_cost=rcost.reshape(-1)[rsel].astype(np.int64), zc_ptr=zc_ptr, zc_dest=zdest.reshape(-1)[zsel],
               zc_cost=zcost.reshape(-1)[zsel].astype(np.int64))
    return ag, nt


def network_snapshot(hdr: Header, n_nodes: int, n_pods: int, seed: int = SEED, pods_per_group: int = 100) -> Dict[str, Table]:
    """Object tables for BASELINE.json config #4 (NetworkOverhead + TopologicalSort)."""
    nodes = synth_nodes(hdr, n_nodes, seed)
    n_groups = max(1, n_pods // pods_per_group)
    ag, nt = synth_network(hdr, nodes, n_groups, seed)
    return {"nodes": nodes, "pods": synth_pods(hdr, n_pods, seed, n_appgroups=n_groups), "appgroups": ag, "nettopo": nt,
            "rc": resource_classes(hdr)}


# ------------------------------------------------------------------ CapacityScheduling (config #5's PreFilter gate)
def synth_quota(hdr: Header, pods: Table, seed: int = SEED, n_namespaces: int = 100, n_nominated: int = 300, device_res: int = -1,
                hugepage_res: int = -1, sized_for_batch: bool = False) -> Table:
    """ElasticQuotas for Q namespaces (Q=100): 85% of namespaces carry a quota; Used is drawn
    around Min so that both PreFilter gates fire for a visible share of pods; nominated pods with priorities in
    {0,100,1000}, a few of them being pending pods themselves (the uid exclusion, capacity_scheduling.go:239)."""
    rng = np.random.default_rng(seed + 8)
    NS, S = n_namespaces, 8
    has = rng.random(NS) < 0.85
    mn = np.zeros((NS, S), dtype=np.int64)
    mx = np.zeros((NS, S), dtype=np.int64)
    us = np.zeros((NS, S), dtype=np.int64)
    mn[:, 0] = rng.integers(50, 400, NS) * 1000
    mn[:, 1] = rng.integers(100, 2000, NS) * GiB
    mn[:, 2] = rng.integers(0, 100, NS) * GiB
    mx[:, :3] = (mn[:, :3] * rng.uniform(1.0, 2.0, (NS, 3))).astype(np.int64)
    no_max = rng.random(NS) < 0.1
    mx[no_max, :3] = (1 << 63) - 1
    us[:, :3] = (mn[:, :3] * rng.uniform(0.2, 1.3, (NS, 3))).astype(np.int64)
    if sized_for_batch:
        # Quotas in proportion to what the batch's namespaces ask for (the fixed sizes above suit the frozen sweep's PreFilter
        # hit rate; scheduled one after the other against them, 89 % of a 62.5k-pod batch ends over Max).  Min = 0.7 - 1.4 x the
        # namespace's total request, Max = 1 - 2 x Min, Used = 0 - 0.25 x Min.
        P = pods.struct.n_pods
        cp, qp = pods.array("ctr_ptr"), pods.array("req_ptr")
        ctr_of = np.repeat(np.arange(len(qp) - 1), np.diff(qp))
        pod_of_ctr = np.repeat(np.arange(P), np.diff(cp))
        pod_of_req = pod_of_ctr[ctr_of]
        ns_of_req = pods.array("ns")[pod_of_req]
        rr, qq = pods.array("req_res"), pods.array("req_qty")
        for slot, res in ((0, 0), (1, 1)):
            demand = np.bincount(ns_of_req[rr == res], weights=qq[rr == res].astype(np.float64), minlength=NS)
            mn[:, slot] = (np.maximum(demand, 1.0) * rng.uniform(0.7, 1.4, NS)).astype(np.int64)
        mx[:, :2] = (mn[:, :2] * rng.uniform(1.0, 2.0, (NS, 2))).astype(np.int64)
        mx[no_max, :2] = (1 << 63) - 1
        us[:, :2] = (mn[:, :2] * rng.uniform(0.0, 0.25, (NS, 2))).astype(np.int64)
    present = np.zeros(NS, dtype=np.uint8)
    n_scalar = 0
    scalar_res = np.zeros(4, dtype=np.int32)
    if device_res >= 0:
        n_scalar = 1
        scalar_res[0] = device_res
        mn[:, 4] = rng.integers(0, 64, NS)
        mx[:, 4] = mn[:, 4] + rng.integers(0, 64, NS)
        us[:, 4] = rng.integers(0, 80, NS)
        if sized_for_batch:  # ~10 % of the pods ask for 1-2 devices
            per_ns = max(1, pods.struct.n_pods // NS)
            mn[:, 4] = rng.integers(per_ns // 8, per_ns // 3 + 2, NS)
            mx[:, 4] = mn[:, 4] + rng.integers(0, per_ns // 4 + 2, NS)
            us[:, 4] = rng.integers(0, per_ns // 40 + 2, NS)
        present[:] = 1 << 4
    hp_slot = -1
    if hugepage_res >= 0:  # pods may request hugepages: a scalar resource the quotas do not bound (no key in Min/Max)
        scalar_res[n_scalar] = hugepage_res
        hp_slot = 4 + n_scalar
        n_scalar += 1
    min_present = np.where(rng.random(NS) < 0.9, present, 0).astype(np.uint8)  # some quotas do not list the device in Min
    if sized_for_batch:
        # every quota lists every scalar the batch asks for: a scalar missing from Min counts as Min = 0 in the AGGREGATE gate
        # (cmp2's LowerBoundOfMin, elasticquota.go:193-221 via aggregatedUsedOverMinWith :48-59), so one nominated pod with
        # hugepages anywhere in the cluster turns every quota'd pod away — faithful, and a degenerate queue to time a commit loop on
        min_present = present.copy()
        if hp_slot >= 0:
            mn[:, hp_slot] = 1 << 44
            mx[:, hp_slot] = 1 << 45
            present = (present | (1 << hp_slot)).astype(np.uint8)
            min_present = present.copy()
    P = pods.struct.n_pods
    nom_ns = rng.integers(0, NS, n_nominated).astype(np.int32)
    nom_prio = rng.choice(np.array([0, 100, 1000], dtype=np.int32), n_nominated)
    nom_pods = synth_pods(hdr, max(n_nominated, 1), seed=seed + 99, device_res=device_res, hugepage_res=hugepage_res, n_namespaces=NS)
    pend = np.full(n_nominated, -1, dtype=np.int64)
    k = min(n_nominated // 10, P)
    if k:
        idx = rng.choice(P, k, replace=False)
        pend[:k] = idx
        nom_ns[:k] = pods.array("ns")[idx]  # the same pod lives in the same namespace
    return Table(hdr, "spx_quota_objects", n_namespaces=NS, n_scalar_slots=n_scalar, scalar_res=scalar_res,
                 has_quota=has.astype(np.uint8), min=mn.reshape(-1), min_present=min_present, max=mx.reshape(-1),
                 max_present=present, used=us.reshape(-1), used_present=present, n_nominated=n_nominated, nom_ns=nom_ns,
                 nom_priority=nom_prio, nom_pending_index=pend, nom_pods=nom_pods)


# ------------------------------------------------------------------ full profile (config #5)
def full_snapshot(hdr: Header, n_nodes: int, n_pods: int, seed: int = SEED, pods_per_group: int = 100,
                  n_namespaces: int = 100, quota_sized_for_batch: bool = False) -> Dict[str, Table]:
    """One snapshot carrying every table of the full profile: CapacityScheduling PreFilter + Allocatable + NRT +
    trimaran + network-aware (BASELINE.json config #5)."""
    snap = nrt_snapshot(hdr, n_nodes, n_pods, seed)  # nodes (with hugepages/devices), NRT, rc
    n_groups = max(1, n_pods // pods_per_group)
    snap["pods"] = synth_pods(hdr, n_pods, seed, device_res=RES_DEVICE, hugepage_res=RES_HUGEPAGES_2MI, n_appgroups=n_groups,
                              n_namespaces=n_namespaces)
    snap["metrics"] = synth_metrics(hdr, n_nodes, seed)
    snap["assigned"] = synth_assigned(hdr, n_nodes, seed)
    snap["appgroups"], snap["nettopo"] = synth_network(hdr, snap["nodes"], n_groups, seed)
    snap["quota"] = synth_quota(hdr, snap["pods"], seed, n_namespaces=n_namespaces, device_res=RES_DEVICE,
                                hugepage_res=RES_HUGEPAGES_2MI, sized_for_batch=quota_sized_for_batch)
    return snap


def node_column_snapshot(n_nodes: int, seed: int = SEED, invalid_frac: float = 0.1, max_pods: int = 6) -> Dict[str, np.ndarray]:
    """NodeMetadata's and PodState's raw node columns (spx_node_column_soa.raw) plus a QOSSort queue of n_nodes pods, on a random
    stream of their own (seed + 311), so that every other generator yields what it always did.  "nodemeta": a numeric label in
    [-1000, 1000], math.MinInt64 (no valid metadata) on about invalid_frac of the nodes; "podstate": terminating minus nominated pods,
    each count in [0, max_pods]; "qos": priority / class (1 BestEffort, 2 Burstable, 3 Guaranteed) / queue timestamp columns."""
    rng = np.random.default_rng(seed + 311)
    meta = rng.integers(-1000, 1001, n_nodes).astype(np.int64)
    meta[rng.random(n_nodes) < invalid_frac] = np.iinfo(np.int64).min
    pod_state = (rng.integers(0, max_pods + 1, n_nodes) - rng.integers(0, max_pods + 1, n_nodes)).astype(np.int64)
    qos = dict(priority=rng.integers(-2, 3, n_nodes).astype(np.int32) * 1000, qos=rng.integers(1, 4, n_nodes).astype(np.uint8),
               queue_ts=(1_700_000_000_000_000_000 + rng.integers(0, 50, n_nodes) * 1_000_000).astype(np.int64))
    return {"nodemeta": meta, "podstate": pod_state, "qos": qos}


def sysched_snapshot(hdr: Header, n_nodes: int, n_pods: int, seed: int = SEED, n_profiles: int = 32, stale_frac: float = 0.03,
                     absent_frac: float = 0.03, empty_frac: float = 0.003, n_names: int = 400, core: int = 150, max_residents: int = 12,
                     distinct_pods: bool = False, node_states: Optional[int] = None) -> dict:
    """A SySched snapshot (pkg/sysched): syscall profiles drawn as subsets of an n_names universe around a common core of `core`
    names; 0..max_residents resident pods per node, each with one of the profiles; absent_frac of the nodes without a HostSyscalls
    entry, stale_frac with a resident whose set is no longer inside the cached host set (a SeccompProfile changed after addPod
    cached it); empty_frac of the pods with the empty set (no profile and no default: Score answers math.MaxInt64).
    distinct_pods: every pending pod has a set of its own.  node_states: that many distinct node states, each node taking one of
    them (None: every node its own).

    Returns {"objects": spx_sysched_objects Table, "names": [str], "sets": [frozenset of names] by set id, "pod_set": int32 [P],
    "host": [frozenset or None] per node, "residents": [tuple of set ids] per node}; nodes of one state share their host object."""
    rng = np.random.default_rng(seed)
    names = [f"sys_{i:04d}" for i in range(n_names)]

    def draw(k):
        m = rng.random((k, n_names)) < 0.45
        m[:, :min(core, n_names)] = True
        return m

    prof = draw(n_profiles)
    empty_id = -1
    if distinct_pods:
        member = np.concatenate([prof, draw(n_pods)])
        # (rows are random over >= n_names - core free bits; equal rows would merge two pods into one set: checked)
        assert len(np.unique(np.packbits(member, axis=1), axis=0)) == len(member) or n_names - core < 40
        pod_set = n_profiles + np.arange(n_pods, dtype=np.int32)
    else:
        member = prof
        pod_set = rng.integers(0, n_profiles, n_pods).astype(np.int32)
    if empty_frac > 0:
        member = np.concatenate([member, np.zeros((1, n_names), bool)])
        empty_id = len(member) - 1
        is_empty = rng.random(n_pods) < empty_frac
        if n_pods >= 8:
            is_empty[rng.integers(0, n_pods)] = True
        pod_set = np.where(is_empty, empty_id, pod_set).astype(np.int32)
    n_sets = len(member)

    S = n_nodes if node_states is None else node_states
    k = rng.integers(0, max_residents + 1, S)
    res_ptr_s = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    res_set_s = rng.integers(0, n_profiles, int(res_ptr_s[-1])).astype(np.int32)
    host_s = np.zeros((S, n_names), bool)
    owner = np.repeat(np.arange(S), k)
    np.logical_or.at(host_s, owner, prof[res_set_s])  # the union addPod accumulates (sysched.go:310-333)
    present_s = rng.random(S) >= absent_frac
    # a present node without residents keeps whatever removePod left; give half of them a leftover profile
    leftover = (k == 0) & (rng.random(S) < 0.5)
    host_s[leftover] = prof[rng.integers(0, n_profiles, int(leftover.sum()))]
    stale = (k > 0) & (rng.random(S) < stale_frac)
    for s in np.flatnonzero(stale):  # names some resident holds drop out of the cached set; a few names nobody holds join it
        held = np.flatnonzero(host_s[s, core:]) + core
        if len(held):
            host_s[s, rng.choice(held, size=min(len(held), int(rng.integers(1, 6))), replace=False)] = False
        host_s[s, rng.integers(core, n_names, 2)] = True
    state = np.arange(n_nodes) if node_states is None else rng.integers(0, S, n_nodes)

    def csr_of(mask):
        ptr = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int32)
        return ptr, np.nonzero(mask)[1].astype(np.int32)

    set_ptr, set_name = csr_of(member)
    host_n = host_s[state] & present_s[state][:, None]
    host_ptr, host_name = csr_of(host_n)
    kn = k[state]
    res_ptr = np.concatenate([[0], np.cumsum(kn)]).astype(np.int32)
    take = np.concatenate([np.arange(res_ptr_s[s], res_ptr_s[s + 1]) for s in state]).astype(np.int64) if n_nodes else np.zeros(0, np.int64)
    res_set = res_set_s[take]
    objects = Table(hdr, "spx_sysched_objects", n_names=n_names, n_sets=n_sets, set_ptr=set_ptr, set_name=set_name, n_pods=n_pods, pod_set=pod_set,
                    n_nodes=n_nodes, host_present=present_s[state].astype(np.uint8), host_ptr=host_ptr, host_name=host_name, res_ptr=res_ptr, res_set=res_set)
    sets = [frozenset(names[j] for j in np.flatnonzero(member[i])) for i in range(n_sets)]
    host_objs = [frozenset(names[j] for j in np.flatnonzero(host_s[s])) if present_s[s] else None for s in range(S)]
    res_objs = [tuple(int(x) for x in res_set_s[res_ptr_s[s]:res_ptr_s[s + 1]]) for s in range(S)]
    return {"objects": objects, "names": names, "sets": sets, "pod_set": pod_set, "host": [host_objs[s] for s in state],
            "residents": [res_objs[s] for s in state], "n_stale_states": int(stale.sum()), "empty_set": empty_id}


def preempt_model(n_nodes: int, n_pending: int, seed: int = SEED, pods_per_node: float = 3.0, node_pods=None, n_pdbs: int = 12, quotas: bool = True, scenarios: bool = True) -> dict:
    """A snapshot for the preemption dry run as plain dicts (objects.build_preempt_tables describes the form).  Few distinct priorities,
    start times and sizes, so that cells tie at every level of pickOneNodeForPreemption; node sizes from tiny to large and requests from
    nothing to a whole node, so that a preemptor has anything from one candidate to hundreds; tight and loose quotas, pods outside their
    quota's set, nominated pods (some of them rows of the batch), PDBs with budgets from -1 to 2, absent nodes.  node_pods: the number
    of pods per node (cycled) instead of a draw around pods_per_node.  quotas=False: no namespace has an ElasticQuota.  scenarios: from 64 nodes x 64 pods on, _preempt_scenarios' scenes replace the last nodes and rows."""
    rng = np.random.default_rng(seed)
    n_ns, n_quota = 8, 5 if quotas else 0
    pick = lambda xs, p=None: xs[int(rng.choice(len(xs), p=p))]
    unit = GiB

    def request(big: bool = False):
        v = [0] * 8
        v[0] = pick([0, 500, 1000, 2000, 4000, 16000] if big else [0, 500, 1000, 2000])
        v[1] = pick([0, 1, 2, 4, 8, 32] if big else [0, 1, 2, 4]) * unit
        v[2] = pick([0, 0, 0, 10]) * unit
        p = 0
        g = pick([None, None, 0, 1, 2])
        if g is not None:
            v[4], p = g, p | 1 << 4
        if rng.random() < 0.05:
            v[5], p = 1, p | 1 << 5
        return {"v": v, "p": p}

    def pod(key, ns, prio, start, req, row=-1, terminating=False, pdbs=()):
        fit = list(req["v"])
        fit[3] = 1
        return {"key": key, "ns": ns, "prio": prio, "start": start, "fit": fit, "req": req, "pdbs": sorted(pdbs), "terminating": terminating, "row": row}

    pending = [pod(f"pending-{i}", int(rng.integers(n_ns)), pick([5, 50, 500, 5000]), 0, request(big=True), row=i) for i in range(n_pending)]
    nodes = []
    for n in range(n_nodes):
        alloc = [pick([2000, 4000, 8000, 16000, 64000]), pick([4, 8, 16, 32, 128]) * unit, pick([0, 20, 100]) * unit, pick([2, 4, 8, 110, 300]), pick([0, 2, 4, 8]), pick([0, 0, 1]), 0, 0]
        count = int(node_pods[n % len(node_pods)]) if node_pods is not None else min(int(rng.poisson(pods_per_node)), 256)
        pods = []
        for k in range(count):
            matches = [int(b) for b in rng.choice(n_pdbs, size=min(3, n_pdbs), replace=False) if rng.random() < 0.25] if n_pdbs else []
            pods.append(pod(f"n{n}-p{k}", int(rng.integers(n_ns)), pick([-(1 << 31), 0, 10, 100, 1000], [0.15, 0.25, 0.25, 0.2, 0.15]), pick([1000, 2000, 3000]),
                            request(), terminating=bool(rng.random() < 0.05), pdbs=matches))
        nominated = []
        if rng.random() < 0.1:
            for k in range(int(rng.integers(1, 3))):
                if n_pending and rng.random() < 0.5:
                    src = pending[int(rng.integers(n_pending))]
                    nominated.append(dict(src, key=src["key"]))
                else:
                    nominated.append(pod(f"n{n}-nom{k}", int(rng.integers(n_ns)), pick([5, 50, 500, 5000]), 0, request()))
        nodes.append({"present": bool(rng.random() >= 0.02), "alloc": alloc, "pods": pods, "nominated": nominated})
    eqs = {}
    for ns in range(n_quota):
        used, members = {"v": [0] * 8, "p": 0}, set()
        for node in nodes:
            for p in node["pods"]:
                if p["ns"] == ns and rng.random() < 0.85:
                    members.add(p["key"])
                    used["v"] = [a + b for a, b in zip(used["v"], p["req"]["v"])]
                    used["p"] |= p["req"]["p"]
        if ns == 4:  # a quota without min: newElasticQuotaInfo's zeros, every use is over it
            mn = {"v": [0] * 8, "p": 0}
        else:  # around the use: some quotas lend, some borrow
            f = pick([0.5, 0.9, 1.0, 1.5, 4.0])
            mp = used["p"] if rng.random() < 0.7 else 0
            mn = {"v": [int(u * f) if s < 4 or (mp >> s) & 1 else 0 for s, u in enumerate(used["v"])], "p": mp}  # an absent key holds nothing
        if ns % 2:  # a tight max, scalar keys included
            mx = {"v": [u + pick([0, 1000, 4000]) * (1 if s == 0 else unit if s < 3 else 1) for s, u in enumerate(used["v"])], "p": used["p"]}
            mx["v"] = [0 if s == 3 or (s > 3 and not (mx["p"] >> s) & 1) else v for s, v in enumerate(mx["v"])]
        else:
            mx = {"v": [(1 << 63) - 1] * 3 + [0] * 5, "p": 0}
        eqs[ns] = {"min": mn, "max": mx, "used": used, "pods": members}
    model = {"n_namespaces": n_ns, "quotas": eqs, "pdbs": [pick([-1, 0, 1, 2]) for _ in range(n_pdbs)], "nodes": nodes, "pending": pending}
    if scenarios and n_nodes >= 64 and n_pending >= 64:
        _preempt_scenarios(model, pod, quotas)
    return model


def _preempt_scenarios(model: dict, pod, quotas: bool) -> None:
    """The last 14 nodes and 7 pending rows become seven two-node scenes, one per level of pickOneNodeForPreemption and one for the
    double removal (capacity_scheduling.go:639, :647).  Scene j is closed to everyone else by two scalar slots nothing else uses: its
    preemptor asks for 2^j of slot 6 and 2^(6-j) of slot 7, which only its own nodes offer both of.  Victims are pods of namespace 7
    (no quota), the preemptors have priority 50."""
    lo, scenes = -(1 << 31), []
    victim = lambda name, prio, cpu, start=1000, pdbs=(): pod(name, 7, prio, start, {"v": [cpu, 0, 0, 0, 0, 0, 0, 0], "p": 0}, pdbs=pdbs)
    model["pdbs"].append(0)  # a budget of its own for the first scene: its one match violates it
    scenes.append(([victim("s0-a", 10, 1000, pdbs=[len(model["pdbs"]) - 1])], [victim("s0-b", 10, 1000)]))  # fewest violations
    scenes.append(([victim("s1-a", 10, 1000)], [victim("s1-b", 0, 1000)]))                                   # lowest highest priority
    scenes.append(([victim("s2-a0", 10, 500), victim("s2-a1", 0, 500)], [victim("s2-b", 10, 1000)]))         # smallest sum
    scenes.append(([victim("s3-a0", 10, 500), victim("s3-a1", lo, 500)], [victim("s3-b", 10, 1000)]))        # equal sums, fewest victims
    scenes.append(([victim("s4-a", 10, 1000, start=1000)], [victim("s4-b", 10, 1000, start=2000)]))          # latest start
    scenes.append(([victim("s5-a", 10, 1000)], [victim("s5-b", 10, 1000)]))                                  # the first of a tie of two
    scenes.append(([], []))
    n_nodes, n_pending = len(model["nodes"]), len(model["pending"])
    for j, (a, b) in enumerate(scenes):
        iso = [1 << j, 1 << (6 - j)]
        req = {"v": [1000, 0, 0, 0, 0, 0] + iso, "p": 3 << 6}
        row = n_pending - 7 + j
        model["pending"][row] = pod(f"pending-{row}", 7, 50, 0, req, row=row)
        for k, pods in enumerate((a, b)):
            model["nodes"][n_nodes - 14 + 2 * j + k] = {"present": True, "alloc": [1000, 0, 0, 110, 0, 0] + iso, "pods": pods, "nominated": []}
    if not quotas:
        return
    # the double removal: the preemptor's quota (namespace 5) is over its max with the nominated pod counted, and the node cannot take
    # the victim back.  Min is set so that the aggregate check passes exactly once the victim is gone; cpu puts the quota over its min.
    eqs, row, x, y = model["quotas"], n_pending - 1, model["nodes"][n_nodes - 2], model["nodes"][n_nodes - 1]
    req = dict(model["pending"][row]["req"], v=[1000, 50, 0, 0, 0, 0, 64, 1])
    gap = [sum(q["used"]["v"][s] for q in eqs.values()) - sum(q["min"]["v"][s] for q in eqs.values()) for s in range(8)]
    mn = [max(0, gap[s] + req["v"][s]) for s in range(8)]
    big = max(0, gap[0]) + 1
    v = pod("s6-v", 5, 0, 1000, {"v": [big, 50, 0, 0, 0, 0, 0, 0], "p": 0})
    eqs[5] = {"min": {"v": mn, "p": 0xF0}, "max": {"v": [(1 << 63) - 1, 99, (1 << 63) - 1, 0, 0, 0, 0, 0], "p": 0}, "used": {"v": list(v["req"]["v"]), "p": 0}, "pods": {"s6-v"}}
    model["pending"][row] = pod(f"pending-{row}", 5, 50, 0, req, row=row)
    x["alloc"], x["pods"] = [big + 999, 100, 0, 110, 0, 0, 64, 1], [v]
    y["nominated"] = [pod("s6-nom", 5, 500, 0, {"v": [0, 50, 0, 0, 0, 0, 0, 0], "p": 0})]


PTOL_NOW = 1_700_000_000 * 10**9


def ptol_model(n_nodes: int, n_pending: int, seed: int = SEED, now: int = PTOL_NOW, **kw) -> dict:
    """preempt_model(quotas=False, ...) decorated for PreemptionToleration (objects.build_preempt_toleration_tables describes the form):
    "classes", a "pc" / "scheduled_at" per assigned pod, a "never" per pending pod and "now".  The decoration is drawn from a stream of
    its own, so the undecorated model is preempt_model's to the bit.  Values sit on the edges of ExemptedFromPreemption: minimum
    preemptable priorities around the pending priorities {5, 50, 500, 5000} and one that does not parse, a class of value 2^31-1
    without the annotation (Value + 1 wraps), toleration seconds absent / 0 / -1 / 30 / 9 223 372 037 (whose Duration wraps), and
    scheduled times that put now before, on and after the end of a 30 s toleration.  About 3 % of the pods name a class that does not
    exist, gathered on one node in twenty.  _preempt_scenarios' scenes stay as they are: their pods name no class."""
    from .objects import PTOL_ANNOTATION_MIN, PTOL_ANNOTATION_TOLERATION
    model = preempt_model(n_nodes, n_pending, seed=seed, quotas=False, **kw)
    rng = np.random.default_rng([seed, 0x70746F6C])
    pick = lambda xs, p=None: xs[int(rng.choice(len(xs), p=p))]
    sec = 10**9
    scenes = kw.get("scenarios", True) and n_nodes >= 64 and n_pending >= 64
    classes = {}

    def class_of(value, mn, tol):
        name = f"pc{value}-min-{'none' if mn is None else mn}-tol-{'none' if tol is None else tol}"
        ann = {}
        if mn is not None:
            ann[PTOL_ANNOTATION_MIN] = mn
        if tol is not None:
            ann[PTOL_ANNOTATION_TOLERATION] = tol
        classes.setdefault(name, {"value": value, "annotations": ann})
        return name

    for n, node in enumerate(model["nodes"]):
        scene = scenes and n >= n_nodes - 14
        broken = (not scene) and rng.random() < 0.05
        for p in node["pods"]:
            p["pc"], p["scheduled_at"] = "", None
            if scene:
                continue
            p["scheduled_at"] = pick([None, now - 30 * sec, now - 29 * sec, now - 31 * sec, now + sec])
            u = rng.random()
            if broken and u < 0.6:
                p["pc"] = "no-such-class"
            elif u < 0.3:
                pass  # an empty PriorityClassName
            elif u < 0.35:
                p["pc"] = class_of((1 << 31) - 1, None, pick([None, "-1", "30"]))
            else:
                p["pc"] = class_of(p["prio"], pick([None, "50", "51", "500", "5001", "a"]), pick([None, "0", "-1", "30", "9223372037"]))
    for i, p in enumerate(model["pending"]):
        p["never"] = bool(rng.random() < 0.1) and not (scenes and i >= n_pending - 7)
    model["classes"], model["now"] = classes, now
    return model
