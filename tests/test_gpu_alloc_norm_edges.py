"""NodeResourcesAllocatable's feasibility-aware NormalizeScore — lo / hi of the raw scores over a pod's feasible nodes, then
(s - lo) * 100 / (hi - lo) in Go's int64 arithmetic — against a plain-integer reference on CONSTRUCTED node tables and feasible
sets (tests/alloc_norm_cases.py; tests/test_alloc_norm_cases.py holds that reference to the oracle on the CPU).  Every byte is
compared at tolerance 0; a mismatch names table class, group (lo, R), row name, row range, node, got and want.

Engine.set_allocatable(mode, {1: 1}) + Engine.upload_alloc_nodes make the raw score of node n the uploaded value ("Least": its
negation) and Engine.upload_feasible_mask gives the feasible sets: no flattener or synthesiser stands between the test and the
kernels.  The copies of the operation and what selects them (alloc_norm_cases.selects / branch):
  * class A  (global range 2^32 - 1): the compact forms — alloc_masked_compact under spx_eval, the two fused forms of k_net_cls
    under spx_eval with NetworkOverhead over a row range (SPX_OPT_NET_ALLOC_FUSED), k_decide_masked under spx_decide;
  * class B1 (global range 2^32) and B2 (2^42 - 1): k_alloc_masked's int64 passes, every row in the "small" branch (one float64
    product; B2's offsets of 2^32 and more go through the two-halves fma);
  * class C  (global range above 2^63): k_alloc_masked, rows in the small branch, the wide branch (range >= 2^42: integer division)
    and, from floor(2^63 / 100) + 1 on, the rows on which the reference's int64 product wraps; run in "Most" and in "Least" mode.
The engine does not report which copy ran except through spx_decide (the folded form leaves Allocatable's table unwritten).

This file is the independent anchor of the tests that hold one copy to another (fused against unfused in
tests/test_gpu_profile.py, spx_decide against spx_eval + spx_eval_best in tests/test_gpu_decide.py); the copy in the cooperative
commit kernel stays held to the oracle by tests/test_gpu_commit*.py (spx_commit_sequential takes no caller mask)."""
import numpy as np
import pytest

import alloc_norm_cases as ac
import best_cases as bc
from helpers import ALLOCATABLE, NETOVERHEAD, TLP
from scheduler_plugins_amd import SpxError
from scheduler_plugins_amd.engine import Engine, mask_of
from test_gpu_best_edges import COLUMNS, RANGES, RANGE_SHAPES

pytestmark = pytest.mark.gpu

SHAPES = RANGE_SHAPES   # (17, 1025, 16385): a single-row launch puts 16 waves on the row, 16385 nodes wrap them once
OPTIONS = {"default": {}, "row_workgroup": {"ROW_WORKGROUP": 1}, "row_align_16": {"ROW_ALIGN": 16}}
_tables = {}


def tables(name, n_nodes):
    if (name, n_nodes) not in _tables:   # built once (the reference with them) and left unchanged
        _tables[(name, n_nodes)] = ac.build(name, n_nodes, seed=0)   # the seed tests/test_alloc_norm_cases.py checks
    return _tables[(name, n_nodes)]


def load(e, t, mode="Most"):
    """the raw column, the TargetLoadPacking columns that go with it (alloc_norm_cases.tlp_bytes) and one pod per row"""
    e.set_allocatable(mode, {1: 1})
    e.upload_alloc_nodes(t.alloc(mode))
    nodes, pods = ac.trimaran_columns(t)
    e.upload_trimaran_nodes(nodes)
    e.upload_trimaran_pods(pods)
    assert np.array_equal(e.raw(ALLOCATABLE, 0), np.array(t.raw, dtype=np.int64))


def report(failures):
    """how many cells differ, in which rows, and the first messages in full"""
    import collections
    import re
    rows = collections.Counter(m.group(0) for f in failures for m in [re.search(r"part \d+ seed \d+, row \d+ '[^']*'", f)] if m)
    return "\n".join([f"{len(failures)} reported cells (at most 6 per row range) in {len(rows)} rows: {dict(rows)}"] + failures[:8])


def ranges_of(t):
    return [(0, t.n_rows)] + list(RANGES)


# ------------------------------------------------------------------------------------------ (a) spx_eval under a caller mask
@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("n_nodes", SHAPES)
@pytest.mark.parametrize("name,mode", [("A", "Most"), ("B1", "Most"), ("B2", "Most"), ("C", "Most"), ("C", "Least")])
def test_masked_normalisation_on_constructed_tables(gpu_required, name, mode, n_nodes, option):
    """spx_eval(ALLOCATABLE) with a caller mask: alloc_masked_compact for class A, k_alloc_masked for B1, B2 and C — whole batches
    (a wave per row; a workgroup per row under SPX_OPT_ROW_WORKGROUP), single rows (16 waves on the row) and batches whose begin and
    count are no multiple of 4, rows padded to 128 and to 16 bytes.  Without the mask every row is the "all nodes feasible" row
    (k_alloc_prepare's own, signed, quotient)."""
    failures = []
    with Engine(0) as e:
        for k, v in OPTIONS[option].items():
            e.set_option(k, v)
        for t in tables(name, n_nodes):
            assert ac.selects(max(t.raw) - min(t.raw)) == t.klass.copy == (ac.COMPACT if name == "A" else ac.GENERAL)
            load(e, t, mode)
            e.upload_feasible_mask(t.masks)
            for rb, re in ranges_of(t):
                e.eval(mask_of(ALLOCATABLE), rb, re)
                e.sync()
                failures += t.mismatches(e.all_scores(ALLOCATABLE, rb, re), rb, re, (mode, option))
            e.upload_feasible_mask(None)
            e.eval(mask_of(ALLOCATABLE))
            e.sync()
            whole = next(r for r, row in enumerate(t.rows) if row is not None and row.name == "all nodes feasible")
            got = e.all_scores(ALLOCATABLE)
            for r in np.flatnonzero((got != t.want[whole]).any(axis=1))[:2]:
                n = int(np.flatnonzero(got[r] != t.want[whole])[0])
                failures.append(f"{(mode, option)} class {name} part {t.part}: unmasked row {r} node {n} (raw {t.raw[n]}): got {got[r, n]} want {t.want[whole, n]}")
    assert not failures, report(failures)


# ------------------------------------------------------------------- (b) the two fused forms in the NetworkOverhead sweep
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("n_nodes", SHAPES)
def test_normalisation_fused_into_the_network_sweep(gpu_required, hdr, oracle, n_nodes, fused):
    """spx_eval(ALLOCATABLE | NETOVERHEAD) over class A with SPX_OPT_NET_ALLOC_FUSED on (k_net_cls writes Allocatable's rows: the
    dependency-free form for the pods of even rows, which belong to no AppGroup, the form with dependencies for the others) and off
    (alloc_masked_compact in its own launch; also what a single row takes), both against the reference.  The feasible set is the
    caller's mask AND NetworkOverhead's Filter verdict, read back; tests/test_alloc_norm_cases.py checks with the oracle that this
    snapshot leaves the rows usable and keeps a dependency's host feasible (the branch that reads that node's offset singly)."""
    parts = tables("A", n_nodes)
    snap = ac.network_snapshot(hdr, parts[0], ac.NET_SEEDS[n_nodes])
    osnap = oracle.Snapshot(snap["nodes"], snap["pods"], appgroups=snap["appgroups"], nettopo=snap["nettopo"])
    verdict = osnap.filter_rows(NETOVERHEAD)
    mask = mask_of(ALLOCATABLE, NETOVERHEAD)
    failures = []
    with Engine(0) as e:
        e.set_option("NET_ALLOC_FUSED", fused)
        e.load_network_objects(snap["nodes"], snap["pods"], snap["appgroups"], snap["nettopo"])
        assert e.kernel_path(NETOVERHEAD) == 1   # the class-table sweep: the one that can carry Allocatable's rows
        for t in parts:
            assert ac.network_conditions(t, snap, verdict) == []
            load(e, t)
            e.upload_feasible_mask(t.masks)
            feasible = (t.masks != 0) & (verdict == 0)
            want = np.stack([ac.reference(t.raw, feasible[r]) for r in range(t.n_rows)])
            for rb, re in ranges_of(t):
                e.eval(mask, rb, re)
                e.sync()
                assert np.array_equal(e.all_status(NETOVERHEAD, rb, re), verdict[rb:re])
                got = e.all_scores(ALLOCATABLE, rb, re)
                for r, n in np.argwhere(got != want[rb:re])[:6]:
                    failures.append(f"fused {fused} {t.describe(rb + int(r))}, AppGroup {snap['pods'].array('appgroup')[rb + r]}, row range {(rb, re)}, "
                                    f"node {n} (raw {t.raw[n]}): got {got[r, n]} want {want[rb + r, n]}")
    assert not failures, report(failures)


# ------------------------------------------------------------------------------------------- (c) spx_decide: k_decide_masked
@pytest.mark.parametrize("n_nodes", SHAPES)
@pytest.mark.parametrize("name", ["A", "B1"])
def test_decide_folds_the_normalisation(gpu_required, name, n_nodes):
    """spx_decide(ALLOCATABLE | TLP), weights 1 : 1, under a caller mask.  TargetLoadPacking's columns make every node's TLP byte
    100 - (its Allocatable byte in its group's "every cell" row), so every total of such a row is 100: the decision must be score 100,
    ties == feasible == |F|, the lowest feasible node — an Allocatable byte one too high anywhere wins alone, one too low drops out
    of the tie count.  Every row is compared with best_cases.reference over (the reference's Allocatable bytes, the TLP bytes read
    back).  Class A: the folded form (k_decide_masked) runs and leaves Allocatable's table unwritten; class B1 is not compact:
    spx_decide falls back to spx_eval + spx_eval_best and still matches."""
    mask, weights = mask_of(ALLOCATABLE, TLP), {ALLOCATABLE: 1, TLP: 1}
    failures = []
    with Engine(0) as e:
        for t in tables(name, n_nodes):
            load(e, t)
            e.upload_feasible_mask(t.masks)
            e.set_plugin_weights(weights)
            e.eval(mask_of(TLP))
            e.sync()
            tlp = e.all_scores(TLP)
            assert np.array_equal(tlp, np.broadcast_to(ac.tlp_bytes(t), tlp.shape))   # precondition: TLP holds exactly those bytes
            want = bc.reference({ALLOCATABLE: t.want, TLP: tlp}, weights, [(t.masks == 0).astype(np.uint8)], n_nodes)
            for r, row in enumerate(t.rows):
                if row is not None and row.name.startswith("every cell of group"):
                    f = np.flatnonzero(t.masks[r])
                    assert (want[0][r], want[1][r], want[2][r], want[3][r]) == (f[0], 100, len(f), len(f)), t.describe(r)
            for rb, re in ranges_of(t):
                e.decide(mask, rb, re)
                for col, g, w in zip(COLUMNS, e.best(rb, re), want):
                    for r in np.flatnonzero(g.astype(np.int64) != w[rb:re])[:4]:
                        failures.append(f"{t.describe(rb + int(r))}, row range {(rb, re)}, {col}: got {g[r]} want {w[rb + r]}")
                if name == "A":
                    with pytest.raises(SpxError):    # the folded form ran: nothing was written to Allocatable's table
                        e.all_scores(ALLOCATABLE, rb, re)
                else:
                    failures += t.mismatches(e.all_scores(ALLOCATABLE, rb, re), rb, re, "spx_decide's fall-back")
    assert not failures, report(failures)
