"""Shared by the preemption dry run's tests: a model (synth.preempt_model's plain dicts) through the object builders and the flatteners,
the oracle's answer for it, and the cell-by-cell comparison.  Computed once per (model, rows, mask) and shared."""
import functools

import numpy as np

import preempt_oracle as PO
import scheduler_plugins_amd as spx
from scheduler_plugins_amd import objects, synth

LARGEST = dict(n_nodes=1030, n_pending=200, seed=1)


@functools.lru_cache(maxsize=None)
def model(**kw):
    return synth.preempt_model(**dict(kw))


@functools.lru_cache(maxsize=None)
def tables(**kw):
    return objects.build_preempt_tables(spx.header(), model(**kw))


@functools.lru_cache(maxsize=None)
def expected(rows=None, mask_seed=None, **kw):
    """the oracle's dry run for the pending rows `rows` (None = all, in order) and the node mask of mask_seed (None = no mask)"""
    m = model(**kw)
    rows = tuple(range(len(m["pending"]))) if rows is None else rows
    return PO.dry_run(m, [m["pending"][r] for r in rows], node_mask(len(rows), len(m["nodes"]), mask_seed))


def node_mask(n_rows, n_nodes, seed):
    if seed is None:
        return None
    return (np.random.default_rng(seed).random((n_rows, n_nodes)) < 0.7).astype(np.uint8)


def model_position(f, t, node, pos):
    """position `pos` of the flattened table's list of `node` -> position in the model's list of that node"""
    at_node, k = t["assigned_at"][int(f["pod_src"][f["pod_ptr"][node] + pos])]
    assert at_node == node
    return k


def assert_dry_run(e, f, t, want):
    """every cell's status, counts and pick keys, every pick, and the victim lists of the picked cells and of one cell per status"""
    N = len(want[0]["cells"])
    col = lambda k: np.array([[c[k] for c in r["cells"]] for r in want], dtype=np.int64)
    st, nv, nx = e.preempt_cells()
    hi, sm, start = e.preempt_keys()
    for name, got in (("status", st), ("n_victims", nv), ("n_violations", nx), ("hi_prio", hi), ("prio_sum", sm), ("start", start)):
        exp = col(name)
        bad = np.argwhere(got.astype(np.int64) != exp)
        assert bad.size == 0, f"{name}: {len(bad)} of {exp.size} cells differ, first (row, node, got, want) {[(int(i), int(n), int(got[i, n]), int(exp[i, n])) for i, n in bad[:5]]}"
    pick = e.preempt_pick()
    exp_pick = np.array([r["pick"][:3] for r in want], dtype=np.int64)
    assert pick["node"].tolist() == exp_pick[:, 0].tolist()
    assert pick["n_candidates"].tolist() == exp_pick[:, 1].tolist()
    assert pick["n_ties"].tolist() == exp_pick[:, 2].tolist()
    cells = {(i, int(r["pick"][0])) for i, r in enumerate(want) if r["pick"][0] >= 0}
    for i, n in sorted(cells):
        c = want[i]["cells"][n]
        assert (int(pick["n_victims"][i]), int(pick["n_violations"][i])) == (c["n_victims"], c["n_violations"])
    exp_st = col("status")
    for s in np.unique(exp_st):
        i, n = np.argwhere(exp_st == s)[0]
        cells.add((int(i), int(n)))
    for i, n in sorted(cells):
        got_st, pos = e.preempt_victims(i, n)
        assert got_st == want[i]["cells"][n]["status"], (i, n)
        assert [model_position(f, t, n, p) for p in pos] == want[i]["cells"][n]["victims"], (i, n)
    assert N == e.n_nodes


# ---------------------------------------------------------------------------------------------------------------- the reference's tables
GOLDEN_NS = {"ns1": 0, "ns2": 1, "": 2}  # "" = the pods of TestPodEligibleToPreemptOthers that name no namespace
INT64_MAX = (1 << 63) - 1


def golden():
    import json
    from pathlib import Path
    return json.loads((Path(__file__).parent / "golden" / "capacity_preemption.json").read_text())


def golden_model(case):
    """one case of tests/golden/capacity_preemption.json as a model: one node, the preemptor as pending row 0, nil start times as one
    "now" (0), quotas with empty `pods` sets and memory-only Max / Min / Used as the tables write them"""
    mem = lambda v: {"v": [0, v, 0, 0, 0, 0, 0, 0], "p": 0}

    def pod(p, row=-1):
        req = {"v": [p["cpu_milli"], p["memory"], 0, 0, 0, 0, 0, 0], "p": 0}
        return {"key": p["name"], "ns": GOLDEN_NS[p["namespace"]], "prio": p["priority"], "start": 0, "fit": req["v"][:3] + [1] + req["v"][4:], "req": req, "pdbs": [],
                "terminating": p["terminating"], "row": row}

    quotas = {GOLDEN_NS[ns]: {"max": mem(q["max_memory"]), "min": mem(q["min_memory"]), "used": mem(q["used_memory"]), "pods": set()} for ns, q in case["quotas"].items()}
    node = {"present": True, "alloc": [0, case["node"]["memory"], 0, case["node"]["pods"], 0, 0, 0, 0], "pods": [pod(p) for p in case["pods"]], "nominated": []}
    return {"n_namespaces": len(GOLDEN_NS), "quotas": quotas, "pdbs": [], "nodes": [node], "pending": [pod(case["pod"], row=0)]}
