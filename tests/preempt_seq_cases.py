"""Shared by the tests of CapacityScheduling's sequential preemption loop: the models, the literal loop's answer
(tests/preempt_seq_oracle.py) computed once per (model, rows, mask, eligible) and shared, the driver of the engine, and the comparison
of everything the fetches give, at tolerance 0 (ptol_seq_cases.assert_sequential: the fetches are the same).

The models.  The project's generator as it stands barely reaches the quota coupling: replayed one preemptor at a time, no quota's Used
moves at 64 x 64, 65 x 63 or 1030 x 200.  So next to the plain generator there is a retuned form of it: synth.preempt_model(...,
seed=1, scenarios=False) with every quota's min set to int(used * f) per slot (min's key mask = used's), f = (0.5, 2.0, 0.9, 1.5, 1.0)
by namespace, and max unbounded — quotas that sit just above, at and below their min, so that one eviction flips a gate.  And hand-built
three-node models, one per effect (HAND)."""
import copy
import functools

import numpy as np

import preempt_cases as PC
import preempt_oracle as PO
import preempt_seq_oracle as SO
import scheduler_plugins_amd as spx
from ptol_seq_cases import assert_sequential, differing_rows, eligible_column  # noqa: F401  (the fetches are shared)
from scheduler_plugins_amd import objects, synth

INT64_MAX = (1 << 63) - 1
RETUNE_F = (0.5, 2.0, 0.9, 1.5, 1.0)
RETUNED = {
    "12x40": dict(n_nodes=12, n_pending=40, pods_per_node=6.0),
    "63x65": dict(n_nodes=63, n_pending=65, pods_per_node=3.0),
    "64x64": dict(n_nodes=64, n_pending=64, pods_per_node=3.0),
    "65x63": dict(n_nodes=65, n_pending=63, pods_per_node=6.0),
    "200x257": dict(n_nodes=200, n_pending=257, pods_per_node=6.0),  # 257 rows cross a 256-row block of the cell buffer
}
PLAIN = {  # the generator as it is; its scenes apply from 64 x 64 on
    "1x1": dict(n_nodes=1, n_pending=1, seed=1),
    "63x65": dict(n_nodes=63, n_pending=65, seed=1),
    "64x64": dict(n_nodes=64, n_pending=64, seed=1),
    "65x63": dict(n_nodes=65, n_pending=63, seed=1),
}


@functools.lru_cache(maxsize=None)
def retuned(**kw):
    m = copy.deepcopy(synth.preempt_model(seed=1, scenarios=False, **kw))
    for ns, q in m["quotas"].items():
        q["min"] = {"v": [int(u * RETUNE_F[ns]) for u in q["used"]["v"]], "p": q["used"]["p"]}
        q["max"] = {"v": [INT64_MAX] * 3 + [0] * 5, "p": 0}
    return m


def model(kind, **kw):
    return retuned(**kw) if kind == "retuned" else PC.model(**kw)


@functools.lru_cache(maxsize=None)
def tables(kind, **kw):
    return objects.build_preempt_tables(spx.header(), model(kind, **kw))


@functools.lru_cache(maxsize=None)
def frozen(kind, rows=None, mask_seed=None, **kw):
    m = model(kind, **kw)
    rows = tuple(range(len(m["pending"]))) if rows is None else rows
    return PO.dry_run(m, [m["pending"][r] for r in rows], PC.node_mask(len(rows), len(m["nodes"]), mask_seed))


@functools.lru_cache(maxsize=None)
def expected(kind, rows=None, mask_seed=None, eligible_seed=None, **kw):
    """(the loop's result per row, its counters) for the pending rows `rows` (None = all, in table order)"""
    m = model(kind, **kw)
    rows = tuple(range(len(m["pending"]))) if rows is None else rows
    counters = {}
    want = SO.run(m, [m["pending"][r] for r in rows], PC.node_mask(len(rows), len(m["nodes"]), mask_seed), eligible_column(len(rows), eligible_seed), counters,
                  frozen(kind, rows=rows, mask_seed=mask_seed, **kw))
    return want, counters


def run(e, t, rows=None, mask=None, eligible=None):
    """the loop of the engine for the pending rows `rows` of the tables `t`"""
    rows = np.arange(int(t["pods"].struct.n_pods)) if rows is None else np.asarray(rows)
    e.preempt_sequential(rows, eligible, mask)


def statuses(want):
    return {c["status"] for r in want for c in r["cells"]}


# ---------------------------------------------------------------------------------------------------------------- the hand-built models
# Three nodes A, B, C with cpu alone and every row masked to one node.  Namespaces 0 (X) and 1 (Y) have quotas, 2 has none, 3 (where a
# model has it) is a quota with a huge min and no use, which keeps the aggregate-min gate open.  Max is unbounded everywhere.  Each
# model is (model, mask, eligible, what): `what` names the probe row and node whose cell shows the effect, that cell in the loop
# ("seq") and in the frozen batch ("frozen"), and the counters of the literal loop that must come out as given.
def _pod(key, ns, prio, cpu, row=-1):
    return {"key": key, "ns": ns, "prio": prio, "start": 1000, "fit": [cpu, 0, 0, 1, 0, 0, 0, 0], "req": {"v": [cpu, 0, 0, 0, 0, 0, 0, 0], "p": 0}, "pdbs": [],
            "terminating": False, "row": row}


def _quota(mn, used, pods):
    cpu = lambda v: {"v": [v, 0, 0, 0, 0, 0, 0, 0], "p": 0}
    return {"min": cpu(mn), "max": {"v": [INT64_MAX] * 3 + [0] * 5, "p": 0}, "used": cpu(used), "pods": set(pods)}


SLACK = lambda: _quota(1_000_000, 0, ())


def _node(cpu, pods, nominated=()):
    return {"present": True, "alloc": [cpu, 0, 0, 110, 0, 0, 0, 0], "pods": list(pods), "nominated": list(nominated)}


def _hand(quotas, nodes, pending, on, eligible=None):
    """pending: [(key, ns, prio, cpu)]; on: the node each row is masked to; a nominated entry {"key": K} stands for pending row K"""
    pend = [_pod(k, ns, prio, cpu, row=i) for i, (k, ns, prio, cpu) in enumerate(pending)]
    by_key = {p["key"]: p for p in pend}
    for nd in nodes:
        nd["nominated"] = [dict(by_key[x["key"]]) if x["key"] in by_key else x for x in nd["nominated"]]
    mask = np.zeros((len(pend), len(nodes)), np.uint8)
    mask[np.arange(len(pend)), on] = 1
    return {"n_namespaces": 4, "quotas": quotas, "pdbs": [], "nodes": nodes, "pending": pend}, mask, None if eligible is None else np.array(eligible, np.uint8)


A, B, C = 0, 1, 2
CAND, NOV, NOFIT, QUOTA, ALLREP = (PO.ST[k] for k in ("CANDIDATE", "NO_VICTIMS", "NOT_FIT", "QUOTA", "ALL_REPRIEVED"))


def hand_t1(in_set, probe=True):
    """T1 with and without the in-set bit.  X: min 2500, used 3000.  Y is far under its min, so a preemptor of Y borrows back from X's
    pods while X is over its min.  P0 (Y) evicts xa (1000) on A.  With xa in X's set Used drops to 2000, under the min, and P1 (Y)
    finds nothing to take on B, a node no step touched; with xa outside the set Used stays 3000 and xb is still a victim.  P1 is a
    probe unless probe is False (hand_cross_node)."""
    quotas = {0: _quota(2500, 3000, {"xb"} | ({"xa"} if in_set else set())), 1: _quota(100000, 0, ())}
    nodes = [_node(1000, [_pod("xa", 0, 0, 1000)]), _node(1000, [_pod("xb", 0, 0, 1000)]), _node(1000, [])]
    m, mask, el = _hand(quotas, nodes, [("P0", 1, 50, 1000), ("P1", 1, 50, 1000)], [A, B], [1, 0] if probe else None)
    moved = {"used_moved": 1, "over_min_flips": 1, "untouched_cells_differ": 1} if in_set else {"used_moved": 0 if probe else 1, "over_min_flips": 0, "untouched_cells_differ": 0}
    return m, mask, el, dict(moved, row=1, node=B, seq=(NOV, []) if in_set else (CAND, [0]), frozen=(CAND, [0]))


def hand_cross_node():
    """A victim on node A takes namespace X back under its min, so that X's pods on the untouched node B stop being removable:
    hand_t1 with the bit set and P1 applying what it finds (nothing)"""
    return hand_t1(True, probe=False)


def hand_t2_same_namespace():
    """T2 entering a same-namespace row's first sum.  X: min 2000, used 1000; Y: min 0, so always over it.  P0 (X, 1000) is not over
    its min with its request (1000 + 1000), borrows ya back on A and is nominated there.  P1 (X, same priority) then counts P0:
    1000 + 2000 > 2000, over its min, so it takes the lower pod of its OWN namespace on B, xb; frozen, it borrows yb back instead."""
    quotas = {0: _quota(2000, 1000, {"xb"}), 1: _quota(0, 2000, {"ya", "yb"}), 3: SLACK()}
    nodes = [_node(1000, [_pod("ya", 1, 0, 1000)]), _node(2000, [_pod("xb", 0, 0, 1000), _pod("yb", 1, 0, 1000)]), _node(1000, [])]
    m, mask, el = _hand(quotas, nodes, [("P0", 0, 50, 1000), ("P1", 0, 50, 1000)], [A, B])
    return m, mask, el, {"row": 1, "node": B, "seq": (CAND, [0]), "frozen": (CAND, [1]), "branch_flips": 1, "used_moved": 2}


def hand_t2_other_namespace(over_min):
    """T2 entering another namespace's second sum only while that quota is not over its min.  Three quotas: X (used 0), Y (used 2000),
    Z (min 0, used 1000, always over it); aggregate min 3000 in both variants.  P0 (Y, 1000) is over its min with its request, takes
    ya of its own namespace on A and is nominated there: Y's Used is 1000, the aggregate 2000.  P1 (X, 500), a probe, borrows zb back
    on B, where everything fits, so the reprieve's aggregatedUsedOverMinWith(nominatedPodsReqWithPodReq) alone decides: 2000 + 500
    stays within 3000, 2000 + 500 + P0's 1000 does not.  P0 counts while Y is not over its min (min 1500 >= 1000: zb is a victim), and
    does not when it is (min 500 < 1000: zb is reprieved)."""
    y_min = 500 if over_min else 1500
    quotas = {0: _quota(3000 - y_min, 0, ()), 1: _quota(y_min, 2000, {"ya"}), 3: _quota(0, 1000, {"zb"})}
    nodes = [_node(1000, [_pod("ya", 1, 0, 1000)]), _node(10000, [_pod("zb", 3, 0, 1000)]), _node(1000, [])]
    m, mask, el = _hand(quotas, nodes, [("P0", 1, 50, 1000), ("P1", 0, 50, 500)], [A, B], [1, 0])
    return m, mask, el, {"row": 1, "node": B, "seq": (ALLREP, []) if over_min else (CAND, [0]), "used_moved": 1}


def hand_t3():
    """T3.  nomB (X, priority 20, 1500) is nominated to B and counts in the first sum of P1 (X, priority 10): used 1000 + 500 + 1500 >
    min 2500, over its min, so xc of its own namespace goes on C.  P0 (priority 50, no quota) evicts the quota-less fb on B and
    clears nomB: P1 is then under its min and borrows yc back instead."""
    quotas = {0: _quota(2500, 1000, {"xc"}), 1: _quota(0, 1000, {"yc"}), 3: SLACK()}
    nodes = [_node(1000, []), _node(3000, [_pod("fb", 2, 0, 1000)], [_pod("nomB", 0, 20, 1500)]), _node(2000, [_pod("xc", 0, 0, 1000), _pod("yc", 1, 0, 1000)])]
    m, mask, el = _hand(quotas, nodes, [("P0", 2, 50, 3000), ("P1", 0, 10, 500)], [B, C])
    return m, mask, el, {"row": 1, "node": C, "seq": (CAND, [1]), "frozen": (CAND, [0]), "t3_cleared": 1, "branch_flips": 1}


def hand_t4(candidate):
    """Both forms of T4.  P0 (X, priority 50, 1500) comes nominated to C, where the Filter charges it for P1 (X, priority 10, 500):
    frozen, C is full with it, P1 is over its min through it and xc has to go.  P0 is masked to A.  With a candidate there (ya) its
    nomination moves to A: it still counts in P1's first sum, but C has room again and xc is reprieved.  Without one the nomination is
    dropped: P1 is under its min, borrows yc back, and yc is reprieved."""
    quotas = {0: _quota(2500, 1000, {"xc"}), 1: _quota(0, 2500 if candidate else 1000, {"yc"} | ({"ya"} if candidate else set())), 3: SLACK()}
    nodes = [_node(1500, [_pod("ya", 1, 0, 1500)] if candidate else []), _node(1000, []), _node(3500, [_pod("xc", 0, 0, 1000), _pod("yc", 1, 0, 1000)], [{"key": "P0"}])]
    m, mask, el = _hand(quotas, nodes, [("P0", 0, 50, 1500), ("P1", 0, 10, 500)], [A, C])
    return m, mask, el, {"row": 1, "node": C, "seq": (ALLREP, []), "frozen": (CAND, [0]), "t4_moved": int(candidate), "t4_dropped": int(not candidate),
                         "branch_flips": int(not candidate)}


def hand_own_branch():
    """A row whose own over-min branch flips through Used alone.  X: min 2000, used 2500, so P1 (X, 500) is over its min and takes the
    lower pods of X.  P0 (Y, under its min) first borrows xa (1000) back on A: X's Used is 1500, P1 is no longer over its min, and
    there is nothing to borrow back on B, since Y is under its min."""
    quotas = {0: _quota(2000, 2500, {"xa", "xb"}), 1: _quota(100000, 0, ())}
    nodes = [_node(1000, [_pod("xa", 0, 0, 1000)]), _node(1000, [_pod("xb", 0, 0, 1000)]), _node(1000, [])]
    m, mask, el = _hand(quotas, nodes, [("P0", 1, 50, 1000), ("P1", 0, 50, 500)], [A, B])
    return m, mask, el, {"row": 1, "node": B, "seq": (NOV, []), "frozen": (CAND, [0]), "branch_flips": 1, "used_moved": 1}


HAND = {
    "t1_in_set": lambda: hand_t1(True), "t1_not_in_set": lambda: hand_t1(False), "t2_same_namespace": hand_t2_same_namespace,
    "t2_other_namespace_not_over_min": lambda: hand_t2_other_namespace(False), "t2_other_namespace_over_min": lambda: hand_t2_other_namespace(True),
    "t3": hand_t3, "t4_moved": lambda: hand_t4(True), "t4_dropped": lambda: hand_t4(False), "cross_node": hand_cross_node, "own_branch": hand_own_branch,
}
