"""Shared by the tests of CapacityScheduling's dry run with NRT's Filter in the refit: preempt_cases' model (quotas on) decorated with
what tests/ptol_nrt_oracle.py reads (ptol_nrt_cases.decorate: containers, zones, placement info; it reads only fields the preemption
model has), the object tables for it, the oracle's answer, and the drivers of the engine.  Computed once per shape and shared; the
cell-by-cell comparison is preempt_cases.assert_dry_run."""
import functools

import numpy as np

import preempt_cases as PC
import preempt_nrt_oracle as CO
import ptol_nrt_cases as NC
import scheduler_plugins_amd as spx
from preempt_cases import assert_dry_run, node_mask  # noqa: F401  (re-exported)
from scheduler_plugins_amd import objects

# ptol_nrt_cases' shapes with the quotas on: rows x nodes at the wave / lane edges, the list lengths at the words of the 256-bit sets,
# 1 / 2 / 8 zones, 1 and 8 slots, 1 and 8 preemptor containers.  LARGEST (the most cells) is the shape the coverage test is about; from
# 64 x 64 on preempt_model's scenes use the last two scalar names, which with EXTRA makes eight slots.
LARGEST = dict(n_nodes=64, n_pending=64, seed=55, zones=(1, 2, 8), max_ctrs=8, extra=True)
SHAPES = {
    "1x1": dict(n_nodes=1, n_pending=1, seed=14, pods_per_node=6.0, zones=(2,), max_ctrs=1),
    "63x65": dict(n_nodes=65, n_pending=63, seed=5, zones=(2, 1), max_ctrs=3),
    "64x64": LARGEST,
    "65x63": dict(n_nodes=63, n_pending=65, seed=3, zones=(8, 2), max_ctrs=2, extra=True),
    "257x3": dict(n_nodes=3, n_pending=257, seed=9, pods_per_node=8.0, zones=(2, 8, 1), max_ctrs=4),
    "lists": dict(n_nodes=14, n_pending=65, seed=6, node_pods=(0, 1, 31, 32, 33, 256, 64), zones=(2, 1, 8), max_ctrs=2),
    "one-slot": dict(n_nodes=20, n_pending=66, seed=12, zones=(2, 1), max_ctrs=2, one_slot=True),
}


@functools.lru_cache(maxsize=None)
def model(zones=(2,), max_ctrs=3, extra=False, one_slot=False, **kw):
    return NC.decorate(PC.model(**kw), kw.get("seed", 0), zones, max_ctrs, extra, one_slot)


def build_tables(m):
    hdr = spx.header()
    t = objects.build_preempt_tables(hdr, m)
    t.update(NC.nrt_tables(hdr, m))
    return t


@functools.lru_cache(maxsize=None)
def tables(**kw):
    return build_tables(model(**kw))


@functools.lru_cache(maxsize=None)
def expected(rows=None, mask_seed=None, mode=True, **kw):
    m = model(**kw)
    rows = tuple(range(len(m["pending"]))) if rows is None else rows
    return CO.dry_run(m, [m["pending"][r] for r in rows], node_mask(len(rows), len(m["nodes"]), mask_seed), mode)


# ---------------------------------------------------------------------------------------------------------------- constructed cells
GiB = NC.GiB
BIG = 1 << 50


def pod(key, ns, prio, cpu, qos, start=1000, row=-1):
    """a one-container pod of `cpu` millicores and 1 GiB"""
    req = {"v": [cpu, GiB, 0, 0, 0, 0, 0, 0], "p": 0}
    r = {"cpu": cpu, "memory": GiB}
    return {"key": key, "ns": ns, "prio": prio, "start": start, "fit": [cpu, GiB, 0, 1, 0, 0, 0, 0], "req": req, "pdbs": [], "terminating": False, "row": row,
            "init_containers": [], "containers": [{"name": "c0", "requests": r, "limits": dict(r) if qos == CO.NO.GUARANTEED else {}}]}


def one_node(node_cpu, zone_cpu_avail, pods, placement, preemptor, quota=None):
    """One node of two NUMA zones with 4 cpus and 64 GiB each (single-numa-node, container scope) and one preemptor.  Namespace 0 has the
    quota `quota` (max cpu, used cpu; min is 1 cpu and 1 GiB, so whoever asks for more is over it, and every pod of the namespace is
    in its set), namespace 1 one that lends (a min nobody's use reaches, so the aggregate is never over its min), namespace 2 none."""
    res = lambda cpu, mem: {"v": [cpu, mem, 0, 0, 0, 0, 0, 0], "p": 0}
    zones = [{"name": f"node-{z}", "resources": [("cpu", 4000, a), ("memory", 64 * GiB, 32 * GiB)]} for z, a in enumerate(zone_cpu_avail)]
    node = {"present": True, "alloc": [node_cpu, 128 * GiB, 0, 110, 0, 0, 0, 0], "pods": pods, "nominated": [], "alloc_names": {"cpu", "memory", "ephemeral-storage", "pods"},
            "nrt": {"zones": zones, "policy": "single-numa-node", "scope": "container"}, "nrt_fresh": True, "placement": placement}
    quotas = {1: {"min": res(BIG, BIG), "max": res(BIG, BIG), "used": res(0, 0), "pods": set()}}
    if quota is not None:
        mine = [p for p in pods if p["ns"] == 0]
        quotas[0] = {"min": res(1000, GiB), "max": res(quota[0], BIG), "used": res(quota[1], len(mine) * GiB), "pods": {p["key"] for p in mine}}
    return {"n_namespaces": 3, "quotas": quotas, "pdbs": [], "nodes": [node], "pending": [preemptor]}


G, B = CO.NO.GUARANTEED, CO.NO.BURSTABLE
ST = CO.ST
# name -> (model, (status, victims) with the Filter, (status, victims) of spx_preempt_dry_run on the same upload)
DIRECTIONS = {
    # no quota anywhere near: the node's totals (10 cpus) take the preemptor next to both pods, but only zone 0, once v1 is gone, has 4
    # whole cpus: NodeResourcesFit alone reprieves everybody, the Filter keeps v1
    "kept-victim": (one_node(10000, [0, 3000], [pod("v1", 2, 10, 4000, G), pod("v2", 2, 20, 1000, G)], {("v1", "c0"): 0, ("v2", "c0"): 1}, pod("p", 2, 100, 4000, G, row=0)),
                    (ST["CANDIDATE"], [0]), (ST["ALL_REPRIEVED"], [])),
    # with v gone the totals take 6 cpus, no zone of 4 does
    "fits-by-totals-only": (one_node(8000, [0, 4000], [pod("v", 2, 10, 4000, G)], {("v", "c0"): 0}, pod("p", 2, 100, 6000, G, row=0)), (ST["NOT_FIT"], []), (ST["CANDIDATE"], [0])),
    # the same node under a quota whose max (5 cpus) the preemptor's 6 exceed: the reference ends the cell at :607, before the quota test
    "not-fit-before-quota": (one_node(8000, [0, 4000], [pod("v", 0, 10, 4000, G)], {("v", "c0"): 0}, pod("p", 0, 100, 6000, G, row=0), quota=(5000, 4000)),
                             (ST["NOT_FIT"], []), (ST["QUOTA"], [])),
    # a (Burstable, 3 cpus) fits again but puts the quota over its max of 4.5 cpus next to the preemptor's 2: it is removed for the quota
    # and is on NRT's stack from then on.  At b's reprieve it is the whole stack and contributes nothing: "no resources to add", b stays a
    # victim.  With an empty stack, or for NodeResourcesFit alone, b is reprieved.
    "again-pod-on-the-stack": (one_node(16000, [2000, 4000], [pod("b", 0, 10, 2000, G), pod("a", 0, 20, 3000, B)], {("b", "c0"): 0, ("a", "c0"): 1},
                                        pod("p", 0, 100, 2000, G, row=0), quota=(4500, 5000)),
                               (ST["CANDIDATE"], [1, 0]), (ST["CANDIDATE"], [1])),
}


# ---------------------------------------------------------------------------------------------------------------- zones that share a NUMA id
def twin_models():
    """ptol_nrt_cases.twin_models() for CapacityScheduling: every pod in namespace 2, which has no quota, next to namespace 1's lending
    one (as one_node's), so that the Filter alone decides"""
    res = lambda cpu, mem: {"v": [cpu, mem, 0, 0, 0, 0, 0, 0], "p": 0}
    lending = {1: {"min": res(BIG, BIG), "max": res(BIG, BIG), "used": res(0, 0), "pods": set()}}
    return NC.twin_models(ns=2, n_namespaces=3, quotas=lending)


def load(e, t):
    """the quota tables, the preemption tables and the NRT side table onto the engine; flatten_preempt_nodes' columns plus "nrt\""""
    f = e.load_preempt_objects(t)
    f["nrt"] = NC.flatten_nrt(e, t, f)
    e.upload_preempt_nrt(f["nrt"])
    return f


def run(e, t, rows=None, mask=None, mode=True):
    rows = np.arange(int(t["pods"].struct.n_pods)) if rows is None else np.asarray(rows)
    e.preempt_nrt_dry_run(rows, mask, mode)


def run_fit_only(e, t, rows=None, mask=None):
    """spx_preempt_dry_run on the same upload"""
    rows = np.arange(int(t["pods"].struct.n_pods)) if rows is None else np.asarray(rows)
    e.preempt_dry_run(rows, mask)
