"""Shared by the tests of PreemptionToleration's dry run with NRT's Filter in the refit: ptol_cases' model decorated with what
tests/ptol_nrt_oracle.py reads (containers, zones, placement info), the object tables for it, the oracle's answer, and the drivers of the
engine.  Computed once per shape and shared; the cell-by-cell comparison is preempt_cases.assert_dry_run."""
import copy
import functools

import numpy as np

import ptol_cases as TC
import ptol_nrt_oracle as NO
import scheduler_plugins_amd as spx
from preempt_cases import assert_dry_run, node_mask  # noqa: F401  (re-exported)
from scheduler_plugins_amd import objects

GiB = 1 << 30
VECTOR_NAMES = ("cpu", "memory", "ephemeral-storage", None) + objects.PREEMPT_SCALARS  # slot of the 8-vector -> resource name
EXTRA = "example.com/gpu"  # reported by zones, requested by nobody: the eighth slot
UNKNOWN = -2  # SPX_EVICT_CTR_UNKNOWN

# rows x nodes at the wave / lane edges, the list lengths at the words of the 256-bit sets, 1 / 2 / 8 zones, 1 and 8 slots, 1 and 8
# preemptor containers.  LARGEST (the most cells) is the shape the coverage test is about; from 64 x 64 on ptol_model's scenes use the
# last two scalar names, which with EXTRA makes eight slots.
LARGEST = dict(n_nodes=64, n_pending=64, seed=4, zones=(1, 2, 8), max_ctrs=8, extra=True)
SHAPES = {
    "1x1": dict(n_nodes=1, n_pending=1, seed=14, pods_per_node=6.0, zones=(2,), max_ctrs=1),
    "63x65": dict(n_nodes=65, n_pending=63, seed=5, zones=(2, 1), max_ctrs=3),
    "64x64": LARGEST,
    "65x63": dict(n_nodes=63, n_pending=65, seed=3, zones=(8, 2), max_ctrs=2, extra=True),
    "257x3": dict(n_nodes=3, n_pending=257, seed=9, pods_per_node=8.0, zones=(2, 8, 1), max_ctrs=4),
    "lists": dict(n_nodes=14, n_pending=65, seed=6, node_pods=(0, 1, 31, 32, 33, 256, 64), zones=(2, 1, 8), max_ctrs=2),
    "one-slot": dict(n_nodes=20, n_pending=66, seed=12, zones=(2, 1), max_ctrs=2, one_slot=True),
}


def request_dict(req):
    """the model's request vector as a v1.ResourceList: non-zero quantities, and the scalar keys the presence mask names"""
    out = {VECTOR_NAMES[s]: req["v"][s] for s in (0, 1, 2) if req["v"][s] > 0}
    out.update({VECTOR_NAMES[s]: req["v"][s] for s in range(4, 8) if (req["p"] >> s) & 1})
    return out


def split(requests, k):
    """`requests` over k containers that add up to it: cpu in steps of 500 millicores, memory in halves of a GiB, the rest with the first"""
    parts = [dict() for _ in range(k)]
    for name, q in requests.items():
        step = {"cpu": 500, "memory": GiB // 2}.get(name)
        share = (q // k) // step * step if step and k > 1 else 0
        for j in range(k):
            mine = q - share * (k - 1) if j == 0 else share
            if mine > 0 or (j == 0 and name not in ("cpu", "memory", "ephemeral-storage")):
                parts[j][name] = mine
    return parts


def with_containers(p, rng, n_app, n_init, guaranteed):
    requests = request_dict(p["req"])
    lim = (lambda r: dict(r)) if guaranteed else (lambda r: {})
    p["containers"] = [{"name": f"c{j}", "requests": r, "limits": lim(r)} for j, r in enumerate(split(requests, n_app))]
    p["init_containers"] = []
    for j in range(n_init):  # never more than the app containers' sum: the pod's effective request stays p["req"]
        r = {name: (q if rng.random() < 0.5 else q // 2) for name, q in requests.items() if name in ("cpu", "memory") and rng.random() < 0.8}
        p["init_containers"].append({"name": f"init{j}", "requests": r, "limits": lim(r)})


def decorate(m, seed, zones=(2,), max_ctrs=3, extra=False, one_slot=False):
    """ptol_model's dicts with the NRT view of every node and pod.  one_slot: nothing but the first scalar resource is requested or
    reported, and every pod requests it."""
    m = copy.deepcopy(m)
    rng = np.random.default_rng([seed, 0x6E7274])
    pick = lambda xs: xs[int(rng.integers(len(xs)))]
    if one_slot:
        for k, p in enumerate([p for n in m["nodes"] for p in n["pods"] + n["nominated"]] + m["pending"]):
            q = p["req"]["v"][4] or 1 + k % 2
            p["req"] = {"v": [0, 0, 0, 0, q, 0, 0, 0], "p": 1 << 4}
            p["fit"] = [0, 0, 0, 1, q, 0, 0, 0]
        for node in m["nodes"]:
            node["alloc"][4] = node["alloc"][4] or 4
    for i, p in enumerate(m["pending"]):
        if i % 11 == 4 and not one_slot:  # BestEffort without a non-native request: the Filter lets it pass unseen
            p["req"] = {"v": [0, 0, p["req"]["v"][2]] + [0] * 5, "p": 0}
            p["fit"] = [0, 0, p["req"]["v"][2], 1, 0, 0, 0, 0]
        n_c = max_ctrs if i % 5 == 0 else int(rng.integers(1, max_ctrs + 1))
        n_init = min(n_c - 1, pick([0, 1, 1, 2]))
        with_containers(p, rng, n_c - n_init, n_init, rng.random() < 0.65)
    for n, node in enumerate(m["nodes"]):
        for p in node["pods"] + node["nominated"]:
            with_containers(p, rng, pick([1, 1, 2]), 0, rng.random() < 0.6)
        a = node["alloc"]
        node["alloc_names"] = {"cpu", "memory", "ephemeral-storage", "pods"} | {VECTOR_NAMES[s] for s in range(4, 8) if a[s]}
        nz = zones[n % len(zones)]
        ids = [z * pick([1, 1, 3]) + pick([0, 0, 1]) for z in range(nz)] if rng.random() < 0.3 else list(range(nz))
        ids = sorted(set(ids))
        while len(ids) < nz:
            ids.append(ids[-1] + 1)
        if rng.random() < 0.3:
            ids = [ids[k] for k in rng.permutation(nz)]
        # where the kubelet put the containers
        u = rng.random()
        placement = None if u < 0.1 else {}
        if u >= 0.14:
            for p in node["pods"]:
                for c in p["containers"]:
                    v = rng.random()
                    if v < 0.93:
                        placement[(p["key"], c["name"])] = pick(ids) if v < 0.8 else 40 if v < 0.87 else -1
        node["placement"] = placement
        node["nrt_fresh"] = bool(rng.random() >= 0.1)
        if rng.random() < 0.08:
            node["nrt"] = None
            continue
        reported = [VECTOR_NAMES[4]] if one_slot else ["cpu", "memory"] + [VECTOR_NAMES[s] for s in range(4, 8) if a[s] and rng.random() < 0.7] + ([EXTRA] if extra else [])
        total = {"cpu": a[0], "memory": a[1], EXTRA: 4, **{VECTOR_NAMES[s]: a[s] for s in range(4, 8)}}
        zs = []
        for zid in ids:
            res = []
            for name in reported:
                if name == "memory" and nz > 1 and rng.random() < 0.1:
                    continue  # a zone that does not report it
                alloc = -(-total[name] // nz)
                used = sum(c["requests"].get(name, 0) for p in node["pods"] for c in p["containers"] if (placement or {}).get((p["key"], c["name"])) == zid)
                v = rng.random()
                avail = max(0, alloc - used) if v < 0.55 else max(0, alloc - used // 2) if v < 0.8 else pick([0, alloc // 2, alloc])
                res.append((name, alloc, avail))
            zs.append({"name": f"node-{zid}", "resources": res})
        node["nrt"] = {"zones": zs, "policy": "single-numa-node" if rng.random() < 0.75 else pick(["none", "best-effort"]), "scope": pick(["container", "pod"])}
    return m


@functools.lru_cache(maxsize=None)
def model(zones=(2,), max_ctrs=3, extra=False, one_slot=False, **kw):
    return decorate(TC.model(**kw), kw.get("seed", 0), zones, max_ctrs, extra, one_slot)


# ---------------------------------------------------------------------------------------------------------------- zones that share a NUMA id
# decorate() never writes one NUMA id twice (sorted(set(ids))), and the seeded shapes keep their tables.  These hand-built models do:
# every node lists "node-0" twice (twins), container scope, placement present.  A container is charged to both twins
# (subtractResourcesFromNUMANodeList), a victim's release lands on both (GetNRTPostPodsEviction walks every zone of the id), and where the
# smaller twin goes below zero the Filter ends with fwk.Error "inconsistent resource accounting" — a Filter that did not succeed: the node
# is no candidate, a victim is not reprieved.
def twin_pod(key, prio, cpus, start=1000, row=-1, ns=0):
    """a Guaranteed pod with one container per entry of `cpus` (millicores), 1 GiB each"""
    total = sum(cpus)
    mem = GiB * len(cpus)
    ctrs = [{"name": f"c{j}", "requests": {"cpu": q, "memory": GiB}, "limits": {"cpu": q, "memory": GiB}} for j, q in enumerate(cpus)]
    return {"key": key, "ns": ns, "prio": prio, "start": start, "fit": [total, mem, 0, 1, 0, 0, 0, 0], "req": {"v": [total, mem, 0, 0, 0, 0, 0, 0], "p": 0},
            "pdbs": [], "terminating": False, "row": row, "pc": "", "scheduled_at": None, "never": False, "init_containers": [], "containers": ctrs}


def twin_node(avail, pods, ids=(0, 0)):
    """zones named by `ids` with 4 000 millicores allocatable and avail[z] available, 64 GiB with 32 available; every container of
    every pod placed on NUMA id 0"""
    zones = [{"name": f"node-{i}", "resources": [("cpu", 4000, a), ("memory", 64 * GiB, 32 * GiB)]} for i, a in zip(ids, avail)]
    return {"present": True, "alloc": [16000, 128 * GiB, 0, 110, 0, 0, 0, 0], "pods": pods, "nominated": [], "alloc_names": {"cpu", "memory", "ephemeral-storage", "pods"},
            "nrt": {"zones": zones, "policy": "single-numa-node", "scope": "container"}, "nrt_fresh": True,
            "placement": {(p["key"], c["name"]): 0 for p in pods for c in p["containers"]}}


def twin_model(ns=0, n_namespaces=1, quotas=None):
    """nodes (the node's totals, 16 cpus, always take the preemptor; only the zones decide):
      0 uneven     3 000 and 500 available, v (1 cpu).  With v gone the twins hold 4 000 and 1 500: a 3-cpu container fits the larger,
                   is charged to both, and the smaller goes to -1 500 — the Error; a reading without the sign test lets it pass, and
                   reprieves v as well
      1 even       2 000 and 2 000, v (2 cpus): its release lands on both twins, 4 000 and 4 000, and two 2-cpu containers take both
      2 reprieve   1 000 and 0, v1 (2 cpus, priority 10) and v2 (1 cpu, priority 20).  With both gone, 4 000 and 3 000 take 3 cpus.
                   Re-adding v2 leaves 3 000 and 2 000: the larger holds the 3 cpus, the smaller goes below zero, v2 stays evicted
      3 free       node 0's sizes under the ids 0 and 1: the duplicate-free twin
    rows: p0 3 cpus, p1 2 + 2 cpus, p2 3 cpus (priority 100, 90, 80): in the loops p2 meets the nodes p0 and p1 have changed"""
    P = lambda key, prio, cpus, start=1000, row=-1: twin_pod(key, prio, cpus, start, row, ns)
    nodes = [twin_node([3000, 500], [P("u-v", 10, [1000])]),
             twin_node([2000, 2000], [P("e-v", 10, [2000])]),
             twin_node([1000, 0], [P("r-v1", 10, [2000], 1000), P("r-v2", 20, [1000], 2000)]),
             twin_node([3000, 500], [P("f-v", 10, [1000])], ids=(0, 1))]
    pending = [P("p0", 100, [3000], row=0), P("p1", 90, [2000, 2000], row=1), P("p2", 80, [3000], row=2)]
    return {"n_namespaces": n_namespaces, "quotas": dict(quotas or {}), "pdbs": [], "nodes": nodes, "pending": pending, "classes": {}, "now": TC.GOLDEN_NOW}


def twin_models(**kw):
    """name -> model: all four nodes (the even twins and the release on both twins are decided next to the Error there); the uneven node
    with its duplicate-free twin; the reprieve node alone"""
    return {name: dict(twin_model(**kw), nodes=[twin_model(**kw)["nodes"][n] for n in cols]) for name, cols in TWIN_MODELS.items()}


TWIN_MODELS = {"twins": (0, 1, 2, 3), "uneven": (0, 3), "reprieve": (2,)}


def quantity(name, v):
    return f"{v}m" if name == "cpu" else v


def nrt_tables(hdr, m):
    """the model's NRT view as what spx_flatten_preempt_nrt takes besides build_preempt_toleration_tables' tables: "nrt" (spx_nrt_objects),
    "nrt_rc", "ctr_numa", "placement_present", "placement_containers".  The resource ids are build_preempt_tables' (the same names
    interned in the same order), EXTRA after them."""
    res = objects.Resources()
    for name in objects.PREEMPT_SCALARS + (EXTRA,):
        res.id(name)
    nrts = [None if n["nrt"] is None else objects.nrt(
        [{"name": z["name"], "type": "Node", "resources": [(name, quantity(name, alloc), quantity(name, alloc), quantity(name, avail)) for name, alloc, avail in z["resources"]]}
         for z in n["nrt"]["zones"]], attributes={"topologyManagerPolicy": n["nrt"]["policy"], "topologyManagerScope": n["nrt"]["scope"]}) for n in m["nodes"]]
    numa = []
    for n in m["nodes"]:
        for p in n["pods"]:
            numa += [UNKNOWN] * len(p["init_containers"])
            numa += [(n["placement"] or {}).get((p["key"], c["name"]), UNKNOWN) for c in p["containers"]]
    return {"nrt": objects.build_nrt_objects(hdr, res, nrts, fresh=[n["nrt_fresh"] for n in m["nodes"]]), "nrt_rc": res.table(hdr),
            "ctr_numa": np.array(numa + [0], dtype=np.int32), "placement_present": np.array([n["placement"] is not None for n in m["nodes"]], dtype=np.uint8),
            "placement_containers": np.array([len(n["placement"] or {}) for n in m["nodes"]], dtype=np.int32)}


def build_tables(m):
    hdr = spx.header()
    t = objects.build_preempt_toleration_tables(hdr, m)
    t.update(nrt_tables(hdr, m))
    return t


@functools.lru_cache(maxsize=None)
def tables(**kw):
    return build_tables(model(**kw))


@functools.lru_cache(maxsize=None)
def expected(rows=None, mask_seed=None, mode=True, **kw):
    m = model(**kw)
    rows = tuple(range(len(m["pending"]))) if rows is None else rows
    return NO.dry_run(m, [m["pending"][r] for r in rows], node_mask(len(rows), len(m["nodes"]), mask_seed), mode)


def flatten_nrt(h, t, f):
    """h: an Engine or a host-only stand-in; f: flatten_preempt_nodes' columns"""
    return h.flatten_preempt_nrt(t["nodes"], t["nrt"], t["nrt_rc"], t["pods"], t["preempt"], f["pod_src"], t["ctr_numa"], t["placement_present"], t["placement_containers"])


def load(e, t):
    """the preemption tables, the toleration table and the NRT side table onto the engine; flatten_preempt_nodes' columns plus "nrt\""""
    f = e.load_preempt_toleration_objects(t)
    f["nrt"] = flatten_nrt(e, t, f)
    e.upload_preempt_nrt(f["nrt"])
    return f


def run(e, t, rows=None, mask=None, mode=True, now=None):
    rows = np.arange(len(t["priority"])) if rows is None else np.asarray(rows)
    e.preempt_toleration_nrt_dry_run(rows, t["priority"][rows], t["never"][rows], t["now"] if now is None else now, mask, mode)
