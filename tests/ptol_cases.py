"""Shared by PreemptionToleration's dry-run tests: a model (synth.ptol_model's plain dicts) through the object builders, the oracle's answer
for it, and the drivers of the engine.  Computed once per (model, rows, mask, now) and shared; the cell-by-cell comparison is
preempt_cases.assert_dry_run."""
import functools
import json
from pathlib import Path

import numpy as np

import ptol_oracle as TO
import scheduler_plugins_amd as spx
from preempt_cases import assert_dry_run, node_mask  # noqa: F401  (re-exported)
from scheduler_plugins_amd import objects, synth

LARGEST = dict(n_nodes=1030, n_pending=200, seed=1)
SHAPES = {
    "1x1": dict(n_nodes=1, n_pending=1, seed=14, pods_per_node=6.0),
    "63x65": dict(n_nodes=63, n_pending=65, seed=3),
    "64x64": dict(n_nodes=64, n_pending=64, seed=4),
    "65x63": dict(n_nodes=65, n_pending=63, seed=5),
    "1030x200": LARGEST,
    "lists": dict(n_nodes=14, n_pending=65, seed=6, node_pods=(0, 1, 31, 32, 33, 256, 64)),
}
SEC = 10**9


@functools.lru_cache(maxsize=None)
def model(**kw):
    return synth.ptol_model(**dict(kw))


@functools.lru_cache(maxsize=None)
def tables(**kw):
    return objects.build_preempt_toleration_tables(spx.header(), model(**kw))


@functools.lru_cache(maxsize=None)
def expected(rows=None, mask_seed=None, now=None, **kw):
    """the oracle's dry run for the pending rows `rows` (None = all, in order), the node mask of mask_seed (None = no mask) and the
    clock `now` (None = the model's)"""
    m = model(**kw)
    rows = tuple(range(len(m["pending"]))) if rows is None else rows
    snap = m if now is None else dict(m, now=now)
    return TO.dry_run(snap, [m["pending"][r] for r in rows], node_mask(len(rows), len(m["nodes"]), mask_seed))


def run(e, t, rows=None, mask=None, now=None):
    """the toleration dry run of the engine for the pending rows `rows` of the tables `t`"""
    rows = np.arange(len(t["priority"])) if rows is None else np.asarray(rows)
    e.preempt_toleration_dry_run(rows, t["priority"][rows], t["never"][rows], t["now"] if now is None else now, mask)


# ---------------------------------------------------------------------------------------------------------------- the reference's tables
def golden():
    return json.loads((Path(__file__).parent / "golden" / "preemption_toleration.json").read_text())


GOLDEN_NOW = synth.PTOL_NOW
GOLDEN_CLASS = "priority-class-for-victim-candidates"


def golden_class(pc):
    """a case's PriorityClass (None = the lister has none) as the model's `classes`"""
    return {} if pc is None else {GOLDEN_CLASS: {"value": pc["value"], "annotations": dict(pc["annotations"])}}


def golden_scheduled_at(offset_s, now=GOLDEN_NOW):
    """"scheduled_at_offset_s": seconds relative to now; "zero" = the zero time.Time, ages before any int64 nanosecond clock; None = no
    PodScheduled condition"""
    if offset_s is None:
        return None
    return -(1 << 63) if offset_s == "zero" else now + offset_s * SEC


def golden_integration_model(case):
    """one scenario of test/integration/preemption_toleration_test.go: node-a (3 cpu, 3Gi), the victim candidate (2 cpu, 1Gi, priority
    1000) scheduled `scheduled_before_s` ago, the preemptor (2 cpu, 1Gi) as pending row 0"""
    g = golden()["integration_fixture"]

    def pod(key, prio, row=-1):
        req = {"v": [g["pod_cpu_milli"], g["pod_memory"], 0, 0, 0, 0, 0, 0], "p": 0}
        return {"key": key, "ns": 0, "prio": prio, "start": 0, "fit": req["v"][:3] + [1] + req["v"][4:], "req": req, "pdbs": [], "terminating": False, "row": row}

    victim = dict(pod("victim-candidate", g["victim_priority"]), pc=GOLDEN_CLASS,
                  scheduled_at=golden_scheduled_at("zero" if case["scheduled_before_s"] == "forever" else -case["scheduled_before_s"]))
    pre = dict(pod("p", case["preemptor_priority"], row=0), never=case["preempt_never"])
    node = {"present": True, "alloc": [g["node_cpu_milli"], g["node_memory"], 0, g["node_pods"], 0, 0, 0, 0], "pods": [victim], "nominated": []}
    return {"n_namespaces": 1, "quotas": {}, "pdbs": [], "nodes": [node], "pending": [pre], "classes": golden_class(case["priority_class"]), "now": GOLDEN_NOW}
