"""Shared by the tests of PreemptionToleration's sequential preemption loop: the literal loop's answer (tests/ptol_seq_oracle.py) for a
model of ptol_cases, computed once per (model, rows, mask, eligible, now) and shared, the driver of the engine, and the comparison of
everything the fetches give, at tolerance 0."""
import functools

import numpy as np

import ptol_cases as TC
import ptol_seq_oracle as SO
from preempt_cases import model_position


def eligible_column(n_rows, seed):
    if seed is None:
        return None
    return (np.random.default_rng(seed).random(n_rows) < 0.6).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def expected(rows=None, mask_seed=None, eligible_seed=None, now=None, **kw):
    """(the loop's result per row, its counters) for the pending rows `rows` (None = all, in table order)"""
    m = TC.model(**kw)
    rows = tuple(range(len(m["pending"]))) if rows is None else rows
    snap = m if now is None else dict(m, now=now)
    counters = {}
    want = SO.run(snap, [m["pending"][r] for r in rows], TC.node_mask(len(rows), len(m["nodes"]), mask_seed), eligible_column(len(rows), eligible_seed), counters)
    return want, counters


def run(e, t, rows=None, mask=None, eligible=None, now=None):
    """the loop of the engine for the pending rows `rows` of the tables `t`"""
    rows = np.arange(len(t["priority"])) if rows is None else np.asarray(rows)
    e.preempt_toleration_sequential(rows, t["priority"][rows], t["never"][rows], t["now"] if now is None else now, eligible, mask)


def differing_rows(seq, frozen):
    """rows that end with another node or other victims in the loop than in the frozen batch"""
    end = lambda r: (r["pick"][0], r["cells"][r["pick"][0]]["victims"] if r["pick"][0] >= 0 else [])
    return sum(end(a) != end(b) for a, b in zip(seq, frozen))


def assert_sequential(e, f, t, want):
    """every row's pick, every cell's status, counts and keys as the row saw them at its step, and the stored victim list of every
    picked cell"""
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
    for i, r in enumerate(want):
        n = int(r["pick"][0])
        if n < 0:
            assert (int(pick["n_victims"][i]), int(pick["n_violations"][i])) == (0, 0)
            continue
        c = r["cells"][n]
        assert (int(pick["n_victims"][i]), int(pick["n_violations"][i])) == (c["n_victims"], c["n_violations"])
        got_st, pos = e.preempt_victims(i, n)
        assert got_st == c["status"] == 0, (i, n)
        assert [model_position(f, t, n, p) for p in pos] == c["victims"], (i, n)
