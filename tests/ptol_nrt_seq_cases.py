"""Shared by the tests of PreemptionToleration's sequential preemption loop with NRT's Filter in the refit: the literal loop's answer
(tests/ptol_nrt_seq_oracle.py) for a model of ptol_nrt_cases, computed once per (model, rows, mask, eligible, mode) and shared, the
driver of the engine, and the constructed model that pins T5.  The comparison is ptol_seq_cases.assert_sequential, at tolerance 0."""
import functools

import numpy as np

import ptol_cases as TC
import ptol_nrt_cases as NC
import ptol_nrt_oracle as NO
import ptol_nrt_seq_oracle as NSO
import ptol_seq_oracle as SO
from ptol_seq_cases import assert_sequential, differing_rows, eligible_column  # noqa: F401  (re-exported)

ST = NO.ST


@functools.lru_cache(maxsize=None)
def expected(rows=None, mask_seed=None, eligible_seed=None, mode=True, **kw):
    """(the loop's result per row, its counters) for the pending rows `rows` (None = all, in table order)"""
    m = NC.model(**kw)
    rows = tuple(range(len(m["pending"]))) if rows is None else rows
    counters = {}
    want = NSO.run(m, [m["pending"][r] for r in rows], NC.node_mask(len(rows), len(m["nodes"]), mask_seed), eligible_column(len(rows), eligible_seed), mode, counters)
    return want, counters


@functools.lru_cache(maxsize=None)
def fit_only(**kw):
    """ptol_seq_oracle.run on the same model: the loop without the Filter"""
    m = NC.model(**kw)
    return SO.run(m, m["pending"])


def run(e, t, rows=None, mask=None, eligible=None, mode=True, now=None):
    """the loop of the engine for the pending rows `rows` of the tables `t`"""
    rows = np.arange(len(t["priority"])) if rows is None else np.asarray(rows)
    e.preempt_toleration_nrt_sequential(rows, t["priority"][rows], t["never"][rows], t["now"] if now is None else now, eligible, mask, mode)


def end(r):
    """a row of a one-node model: (pick, status, victims) of its only cell"""
    c = r["cells"][0]
    return (r["pick"][0], c["status"], c["victims"])


# ---------------------------------------------------------------------------------------------------------------- the second visit (T5)
def second_visit_model():
    """One node of 8 cpus, two zones of 4 000 millicores with 0 available (container scope, placement present).  Guaranteed pods a
    (zone 0, start 1000) and b (zone 1, start 2000) of 4 000 each, priority 0; Guaranteed rows p0 (priority 10) and p1 (priority 20) of
    4 000 each.
    p0 removes both; a, the earlier start, is tried first and stays (the totals take it and b's release leaves zone 1 with 4 000); b
    does not fit the totals and goes.  p1 (p0's nomination is below it and not charged) removes a; adding a back fits the totals, and
    the Filter then has an empty stack on zones with 0 available: a goes.  b is no longer on the node, so nothing releases zone 1; a
    loop that credited b's cpus to zone 1 would reprieve a, as NodeResourcesFit alone does."""
    GiB = NC.GiB

    def pod(key, prio, start=1000, row=-1):
        r = {"cpu": 4000, "memory": GiB}
        return {"key": key, "ns": 0, "prio": prio, "start": start, "fit": [4000, GiB, 0, 1, 0, 0, 0, 0], "req": {"v": [4000, GiB, 0, 0, 0, 0, 0, 0], "p": 0}, "pdbs": [],
                "terminating": False, "row": row, "pc": "", "scheduled_at": None, "never": False, "init_containers": [],
                "containers": [{"name": "c0", "requests": r, "limits": dict(r)}]}

    zones = [{"name": f"node-{z}", "resources": [("cpu", 4000, 0), ("memory", 64 * GiB, 32 * GiB)]} for z in range(2)]
    node = {"present": True, "alloc": [8000, 128 * GiB, 0, 110, 0, 0, 0, 0], "pods": [pod("a", 0, 1000), pod("b", 0, 2000)], "nominated": [],
            "alloc_names": {"cpu", "memory", "ephemeral-storage", "pods"}, "nrt": {"zones": zones, "policy": "single-numa-node", "scope": "container"}, "nrt_fresh": True,
            "placement": {("a", "c0"): 0, ("b", "c0"): 1}}
    return {"n_namespaces": 1, "quotas": {}, "pdbs": [], "nodes": [node], "pending": [pod("p0", 10, row=0), pod("p1", 20, row=1)], "classes": {}, "now": TC.GOLDEN_NOW}


C, R, NF = ST["CANDIDATE"], ST["ALL_REPRIEVED"], ST["NOT_FIT"]
SECOND_VISIT = {"loop": [(0, C, [1]), (0, C, [0])], "fit_only_p1": (-1, R, []), "frozen_p1": (0, C, [1]), "mode_off": [(-1, NF, []), (-1, NF, [])]}
