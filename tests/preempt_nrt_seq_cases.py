"""Shared by the tests of CapacityScheduling's sequential preemption loop with NRT's Filter in the refit: the models,
the literal loop's answer (tests/preempt_nrt_seq_oracle.py) computed once per (model, rows, mask, eligible, mode) and shared, the other
three paths' answers on the same models, the driver of the engine, and the two constructed models.  The comparison is
ptol_seq_cases.assert_sequential, at tolerance 0.

The models are preempt_nrt_cases' shapes (kind "shape") and preempt_seq_cases' retuned models, whose quotas sit around their min so that
one eviction flips a gate, decorated with what the Filter reads (kind "retuned")."""
import copy
import functools

import numpy as np

import preempt_nrt_cases as CC
import preempt_nrt_oracle as CO
import preempt_nrt_seq_oracle as NSO
import preempt_seq_cases as SC
import preempt_seq_oracle as SO
import ptol_nrt_cases as NC
import ptol_nrt_seq_cases as TNSC
from ptol_seq_cases import assert_sequential, differing_rows, eligible_column  # noqa: F401  (re-exported)

ST = CO.ST
MODELS = [("retuned", n) for n in SC.RETUNED] + [("shape", n) for n in CC.SHAPES if n != "1x1"]
# (kind, name) -> the columns of the table in DESIGN.md 3.9j that are zero: frozen NRT batch, fit-only loop, mode off, used_moved
ZERO = {("shape", "65x63"): {"used_moved"}, ("shape", "257x3"): {"used_moved"}, ("shape", "lists"): {"fit_only", "mode_off", "used_moved"}}


@functools.lru_cache(maxsize=None)
def model(kind, name):
    if kind == "retuned":
        return NC.decorate(copy.deepcopy(SC.retuned(**SC.RETUNED[name])), 1, (2, 1), 3, False, False)
    return CC.model(**CC.SHAPES[name])


@functools.lru_cache(maxsize=None)
def tables(kind, name):
    return CC.build_tables(model(kind, name))


def _rows(m, rows):
    return tuple(range(len(m["pending"]))) if rows is None else rows


@functools.lru_cache(maxsize=None)
def frozen(kind, name, rows=None, mask_seed=None, mode=True):
    """the frozen NRT batch: preempt_nrt_oracle.dry_run of the rows on the untouched model"""
    m = model(kind, name)
    rows = _rows(m, rows)
    return CO.dry_run(m, [m["pending"][r] for r in rows], CC.node_mask(len(rows), len(m["nodes"]), mask_seed), mode)


@functools.lru_cache(maxsize=None)
def expected(kind, name, rows=None, mask_seed=None, eligible_seed=None, mode=True):
    """(the loop's result per row, its counters) for the pending rows `rows` (None = all, in table order)"""
    m = model(kind, name)
    rows = _rows(m, rows)
    counters = {}
    want = NSO.run(m, [m["pending"][r] for r in rows], CC.node_mask(len(rows), len(m["nodes"]), mask_seed), eligible_column(len(rows), eligible_seed), mode, counters,
                   frozen(kind, name, rows, mask_seed, mode))
    return want, counters


@functools.lru_cache(maxsize=None)
def fit_only(kind, name):
    """preempt_seq_oracle.run on the same model: the loop without the Filter"""
    m = model(kind, name)
    return SO.run(m, m["pending"])


def run(e, t, rows=None, mask=None, eligible=None, mode=True):
    """the loop of the engine for the pending rows `rows` of the tables `t`"""
    rows = np.arange(int(t["pods"].struct.n_pods)) if rows is None else np.asarray(rows)
    e.preempt_nrt_sequential(rows, eligible, mask, mode)


def end(r, n):
    """(status, victims) of cell n of a row"""
    c = r["cells"][n]
    return (c["status"], c["victims"])


# ---------------------------------------------------------------------------------------------------------------- the cross-node model
GiB, BIG = CC.GiB, CC.BIG
A, B = 0, 1
C, NOV, NF, R = ST["CANDIDATE"], ST["NO_VICTIMS"], ST["NOT_FIT"], ST["ALL_REPRIEVED"]


def cross_node_model():
    """-> (model, mask).  Two nodes of 10 cpus, each with two zones of 4 000 millicores, 0 and 3 000 available (single-numa-node,
    container scope).  A holds xa (namespace 0, 4 000, zone 0) and va (no quota, priority 200, 1 000, zone 1), B holds xb (namespace 0,
    4 000, zone 0).  Quota 0: min 5 000, used 8 000, over its min; quota 1 lends.  P0 and P1 (namespace 1, 4 000 whole cpus) borrow back
    from quota 0; P0 is masked to A and P1 to B.
    P0 removes xa; the totals take xa back next to P0 (10 000), NodeResourcesFit alone reprieves it; with xa back the Filter's stack is
    empty and no zone has 4 000: xa stays a victim and leaves quota 0, whose Used drops to 4 000, under its min.  On B, a node no step
    touched, xb is then no longer borrowed: P1 finds no victims.  The fit-only loop reprieves xa, so Used stays and P1 removes xb and
    reprieves it the same way; with the mode off nothing releases zone 0 on either node; the frozen batch takes xb for P1 as it took
    xa for P0."""
    res = lambda cpu, mem: {"v": [cpu, mem, 0, 0, 0, 0, 0, 0], "p": 0}
    G = CC.G

    def node(pods, placement):
        zones = [{"name": f"node-{z}", "resources": [("cpu", 4000, a), ("memory", 64 * GiB, 32 * GiB)]} for z, a in enumerate((0, 3000))]
        return {"present": True, "alloc": [10000, 128 * GiB, 0, 110, 0, 0, 0, 0], "pods": pods, "nominated": [], "alloc_names": {"cpu", "memory", "ephemeral-storage", "pods"},
                "nrt": {"zones": zones, "policy": "single-numa-node", "scope": "container"}, "nrt_fresh": True, "placement": placement}

    nodes = [node([CC.pod("xa", 0, 10, 4000, G), CC.pod("va", 2, 200, 1000, G)], {("xa", "c0"): 0, ("va", "c0"): 1}), node([CC.pod("xb", 0, 10, 4000, G)], {("xb", "c0"): 0})]
    quotas = {0: {"min": res(5000, BIG), "max": res(BIG, BIG), "used": res(8000, 2 * GiB), "pods": {"xa", "xb"}},
              1: {"min": res(BIG, BIG), "max": res(BIG, BIG), "used": res(0, 0), "pods": set()}}
    pending = [CC.pod("P0", 1, 100, 4000, G, row=0), CC.pod("P1", 1, 100, 4000, G, row=1)]
    return {"n_namespaces": 3, "quotas": quotas, "pdbs": [], "nodes": nodes, "pending": pending}, np.array([[1, 0], [0, 1]], np.uint8)


# path -> (cell (P0, A), cell (P1, B))
CROSS_NODE = {"loop": ((C, [0]), (NOV, [])), "fit_only": ((R, []), (R, [])), "mode_off": ((NF, []), (NF, [])), "frozen": ((C, [0]), (C, [0]))}

# ---------------------------------------------------------------------------------------------------------------- the second visit (T5)
second_visit_model = TNSC.second_visit_model  # one node, no quotas: ptol_nrt_seq_cases describes it
SECOND_VISIT = TNSC.SECOND_VISIT
row_end = TNSC.end  # a row of a one-node model: (pick, status, victims) of its only cell
