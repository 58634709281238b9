"""spx_decide: the per-pod decision (best node, weighted score, ties, feasible) computed without materialising score tables
must equal spx_eval + spx_eval_best exactly — it is the same float32/float64 cell code with the argmax folded in.

That equality holds code under test to code under test: it rests on spx_eval_best being right.  The independent anchor is
tests/test_gpu_best_edges.py, which holds spx_eval_best's kernels to a numpy int64 reference (tests/best_cases.py) on constructed
tables; the threshold tests at the end of this file apply the same reference to the tables a separate spx_eval wrote, so that a
disagreement names which of the three (spx_decide, spx_eval_best, the reference over spx_eval's bytes) is off.
The masked normalisation folded into k_decide_masked has its own anchor on constructed tables: tests/test_gpu_alloc_norm_edges.py."""
import numpy as np
import pytest

from best_cases import reference
from helpers import ALLOCATABLE, CAPACITY, LROC, LVRB, NETOVERHEAD, NRT, PEAKS, TLP
from scheduler_plugins_amd import synth
from scheduler_plugins_amd import SpxError
from scheduler_plugins_amd.engine import Engine, mask_of

pytestmark = pytest.mark.gpu


def both(e, mask, rb=0, re=None):
    e.eval(mask, rb, re)
    e.eval_best(mask, rb, re)
    want = [x.copy() for x in e.best(rb, re)]
    e.decide(mask, rb, re)
    got = e.best(rb, re)
    return want, got


@pytest.mark.parametrize("n_nodes,n_pods,seed,round_frac", [(1, 1, 1, 0.0), (17, 5, 2, 1.0), (1023, 70, 3, 0.3), (1025, 130, 4, 0.0),
                                                              (3000, 257, 5, 1.0), (10_000, 300, 6, 0.1)])
@pytest.mark.parametrize("plugins,weights", [((ALLOCATABLE, TLP), {ALLOCATABLE: 1, TLP: 1}), ((TLP,), {TLP: 3}),
                                             ((ALLOCATABLE, TLP), {ALLOCATABLE: 5, TLP: 2}), ((ALLOCATABLE, TLP), {ALLOCATABLE: 0, TLP: 1})])
def test_decide_equals_eval_plus_argmax(gpu_required, hdr, n_nodes, n_pods, seed, round_frac, plugins, weights):
    snap = synth.trimaran_snapshot(hdr, n_nodes, n_pods, seed=seed, round_frac=round_frac)
    with Engine(0) as e:
        e.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])
        e.set_plugin_weights(weights)
        want, got = both(e, mask_of(*plugins))
    for name, w, g in zip(("node", "score", "ties", "feasible"), want, got):
        assert (w == g).all(), (name, np.flatnonzero(w != g)[:5], w[w != g][:5], g[w != g][:5])
    assert (want[2] > 1).any() or round_frac == 0.0 or n_nodes < 1000   # the larger rounded snapshots do produce ties


def test_partial_rows_and_unfused_profiles(gpu_required, hdr):
    snap = synth.trimaran_snapshot(hdr, 777, 200, seed=8, round_frac=0.5)
    with Engine(0) as e:
        e.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])
        want, got = both(e, mask_of(ALLOCATABLE, TLP), 37, 151)
        for w, g in zip(want, got):
            assert (w == g).all()
        # LVRB joins the fused form as a table that is read once (see test_decide_folds_score_only_tables)
        want, got = both(e, mask_of(ALLOCATABLE, TLP, LVRB), 11, 190)
        for w, g in zip(want, got):
            assert (w == g).all()
        # SPX_OPT_DECIDE_UNFUSED runs eval + eval_best inside: same answer by definition, tables evaluated
        e.set_option("DECIDE_UNFUSED", 1)
        want, got = both(e, mask_of(ALLOCATABLE, TLP, LVRB))
        for w, g in zip(want, got):
            assert (w == g).all()
        e.set_option("DECIDE_UNFUSED", 0)
        # a caller feasibility mask also takes the unfused route
        rng = np.random.default_rng(1)
        e.upload_feasible_mask((rng.random((200, 777)) < 0.7).astype(np.uint8))
        want, got = both(e, mask_of(ALLOCATABLE, TLP))
        for w, g in zip(want, got):
            assert (w == g).all()


@pytest.mark.parametrize("n_nodes,n_pods,seed,round_frac", [(17, 5, 2, 1.0), (1025, 130, 4, 0.0), (3000, 257, 5, 1.0), (10_000, 300, 6, 0.1)])
@pytest.mark.parametrize("plugins,weights", [((ALLOCATABLE, TLP, LVRB), {ALLOCATABLE: 1, TLP: 1, LVRB: 1}),
                                             ((TLP, LVRB), {TLP: 2, LVRB: 7}),
                                             ((ALLOCATABLE, TLP, LVRB, LROC, PEAKS), {ALLOCATABLE: 1, TLP: 1, LVRB: 1, LROC: 1, PEAKS: 1}),
                                             ((ALLOCATABLE, TLP, LROC, PEAKS), {ALLOCATABLE: 3, TLP: 1, LROC: 4, PEAKS: 2})])
def test_decide_folds_score_only_tables(gpu_required, hdr, n_nodes, n_pods, seed, round_frac, plugins, weights):
    """Profiles that add LoadVariationRiskBalancing / LowRiskOverCommitment / Peaks to {Allocatable, TargetLoadPacking}: those
    plugins' tables are evaluated and read ONCE by the fused sweep; Allocatable's and TargetLoadPacking's are never
    written and no second pass (spx_eval_best) runs.  Decisions identical to spx_eval + spx_eval_best."""
    snap = synth.trimaran_snapshot(hdr, n_nodes, n_pods, seed=seed, round_frac=round_frac, with_node_pods=True)
    snap["power_models"] = synth.synth_power_models(hdr, n_nodes, seed)

    def load(e):
        e.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])
        if LROC in plugins:
            e.set_lroc()
            e.load_lroc_objects(snap["nodes"], snap["node_pods"], snap["pods"])
        if PEAKS in plugins:
            e.load_peaks_objects(snap["nodes"], snap["metrics"], snap["power_models"], snap["pods"])
        e.set_plugin_weights(weights)

    with Engine(0) as e:
        load(e)
        want, got = both(e, mask_of(*plugins))
    for name, w, g in zip(("node", "score", "ties", "feasible"), want, got):
        assert (w == g).all(), (name, np.flatnonzero(w != g)[:5], w[w != g][:5], g[w != g][:5])
    with Engine(0) as e:   # the fused form ran: TargetLoadPacking's table was never evaluated, the folded plugins' were
        load(e)
        e.decide(mask_of(*plugins))
        assert (e.best()[0] == want[0]).all()
        with pytest.raises(SpxError):
            e.all_scores(TLP, 0, n_pods)
        for p in plugins:
            if p not in (ALLOCATABLE, TLP):
                assert e.all_scores(p, 0, n_pods).shape == (n_pods, n_nodes)


def test_config2_size(gpu_required, hdr):
    snap = synth.trimaran_snapshot(hdr, 10_000, 100_000)
    with Engine(0) as e:
        e.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])
        want, got = both(e, mask_of(ALLOCATABLE, TLP))
        for w, g in zip(want, got):
            assert (w == g).all()
        want, got = both(e, mask_of(ALLOCATABLE, TLP, LVRB))
    for w, g in zip(want, got):
        assert (w == g).all()


# ------------------------------------------------------------------ profiles with Filter plugins (k_decide_masked)
def _full(e, hdr, n_nodes, n_pods, seed, weights):
    from test_gpu_profile import load_all
    snap = synth.full_snapshot(hdr, n_nodes, n_pods, seed=seed, pods_per_group=20, n_namespaces=20)
    load_all(e, hdr, snap)
    e.set_plugin_weights(weights)
    return snap


@pytest.mark.parametrize("n_nodes,n_pods,seed", [(300, 200, 1), (65, 33, 2), (17, 9, 3), (2100, 150, 4)])
@pytest.mark.parametrize("weights", [{ALLOCATABLE: 1, TLP: 2, LVRB: 1, NRT: 3, NETOVERHEAD: 2}, {ALLOCATABLE: 7, TLP: 0, LVRB: 1, NRT: 1, NETOVERHEAD: 1}])
@pytest.mark.parametrize("row_workgroup", [0, 1])
def test_decide_with_filter_plugins(gpu_required, hdr, n_nodes, n_pods, seed, weights, row_workgroup):
    """the whole profile (CapacityScheduling PreFilter, NRT and NetworkOverhead Filters, five scoring plugins): Allocatable's
    feasibility-aware NormalizeScore happens inside the argmax kernel and its table is not written — same decisions"""
    from test_gpu_profile import ALL
    with Engine(0) as e:
        e.set_option("ROW_WORKGROUP", row_workgroup)  # 1: a whole workgroup per row in batch launches (what very wide rows take)
        _full(e, hdr, n_nodes, n_pods, seed, weights)
        want, got = both(e, mask_of(*ALL))
        for name, w, g in zip(("node", "score", "ties", "feasible"), want, got):
            assert (w == g).all(), (name, np.flatnonzero(w != g)[:5], w[w != g][:5], g[w != g][:5])
        assert (want[0] < 0).any() or n_pods < 30      # pods without a feasible node / rejected by PreFilter are in the batch
        with pytest.raises(SpxError):                   # nothing was written to Allocatable's table by the fused form
            e.all_scores(ALLOCATABLE)
        assert e.all_scores(NRT).shape == (n_pods, n_nodes)   # the Filter plugins' tables are there as after spx_eval
        # subsets of the profile, partial rows, a single row (a whole workgroup on the row)
        for mask in (mask_of(ALLOCATABLE, NRT), mask_of(ALLOCATABLE, TLP, NETOVERHEAD), mask_of(ALLOCATABLE, NRT, NETOVERHEAD, CAPACITY)):
            want, got = both(e, mask)
            for w, g in zip(want, got):
                assert (w == g).all()
        if n_pods > 40:
            for rb, re in ((7, 8), (11, 40), (0, n_pods)):
                want, got = both(e, mask_of(*ALL), rb, re)
                for w, g in zip(want, got):
                    assert (w == g).all()


def test_decide_with_a_caller_mask_and_the_unfused_switch(gpu_required, hdr):
    from test_gpu_profile import ALL
    weights = {ALLOCATABLE: 2, TLP: 1, LVRB: 1, NRT: 1, NETOVERHEAD: 1}
    with Engine(0) as e:
        _full(e, hdr, 500, 120, 6, weights)
        e.upload_feasible_mask((np.random.default_rng(3).random((120, 500)) < 0.6).astype(np.uint8))
        want, got = both(e, mask_of(*ALL))
        for w, g in zip(want, got):
            assert (w == g).all()
        want, got = both(e, mask_of(ALLOCATABLE, TLP))       # the caller's mask alone makes Allocatable feasibility-aware
        for w, g in zip(want, got):
            assert (w == g).all()
        e.set_option("DECIDE_UNFUSED", 1)
        want, got = both(e, mask_of(*ALL))
        for w, g in zip(want, got):
            assert (w == g).all()
        assert e.all_scores(ALLOCATABLE).shape == (120, 500)   # the unfused route is spx_eval + spx_eval_best: table written


def test_decide_with_filter_plugins_falls_back_on_a_wide_allocatable_range(gpu_required, hdr):
    """raw Allocatable scores spanning more than 2^32 have no compact form: spx_decide runs spx_eval + spx_eval_best"""
    from test_gpu_profile import ALL, load_all
    snap = synth.full_snapshot(hdr, 200, 60, seed=9, pods_per_group=20, n_namespaces=20)
    snap["nodes"].array("alloc_mem")[:] *= 64
    with Engine(0) as e:
        e.set_allocatable("Least", {1: 1})
        load_all(e, hdr, snap)
        want, got = both(e, mask_of(*ALL))
        for w, g in zip(want, got):
            assert (w == g).all()
        assert e.all_scores(ALLOCATABLE).shape == (60, 200)


# ------------------------------------------------------------------ the dispatch thresholds, against the numpy reference
def three_way(e, plugins, weights, filters=(), prefilter=None):
    """(reference over the tables of a separate spx_eval, spx_eval_best, spx_decide) on one engine, every row; asserts all equal"""
    mask = mask_of(*plugins)
    e.set_plugin_weights(weights)
    e.eval(mask)
    e.sync()
    scores = {p: e.all_scores(p) for p in plugins if p in weights}
    statuses = [e.all_status(p) for p in filters]
    rejected = (e.prefilter(prefilter) != 0) if prefilter is not None else None
    want = reference(scores, weights, statuses, e.n_nodes, rejected)
    e.eval_best(mask)
    unfused = [x.copy() for x in e.best()]
    e.decide(mask)
    decided = e.best()
    for name, w, u, d in zip(("node", "score", "ties", "feasible"), want, unfused, decided):
        bad_u, bad_d = np.flatnonzero(u != w), np.flatnonzero(d != w)
        assert len(bad_u) == 0, ("spx_eval_best differs from the reference", name, weights, bad_u[:5], u[bad_u[:5]], w[bad_u[:5]])
        assert len(bad_d) == 0, ("spx_decide differs from the reference", name, weights, bad_d[:5], d[bad_d[:5]], w[bad_d[:5]])
    return want


@pytest.mark.parametrize("n_nodes,seed", [(1025, 4), (3000, 5)])
# the weights of the mask sum to 8000: the last sum the fused sweep's 32-bit key admits (8000 << 11, the multiplier v_mad_u32_u24 takes,
# is 2 % below 2^24); 8001 is the first sum that leaves the fused form
@pytest.mark.parametrize("plugins,weights,fused", [
    ((TLP,), {TLP: 8000}, True),
    ((ALLOCATABLE, TLP, LVRB), {ALLOCATABLE: 3999, TLP: 4000, LVRB: 1}, True),
    ((TLP, LVRB), {TLP: 1, LVRB: 7999}, True),
    ((ALLOCATABLE, TLP), {ALLOCATABLE: 8000, TLP: 0}, True),
    ((TLP,), {TLP: 8001}, False),
])
def test_decide_at_the_fused_sweeps_weight_limit(gpu_required, hdr, n_nodes, seed, plugins, weights, fused):
    n_pods = 100
    snap = synth.trimaran_snapshot(hdr, n_nodes, n_pods, seed=seed, round_frac=1.0)

    def load(e):
        e.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])

    with Engine(0) as e:
        load(e)
        want = three_way(e, plugins, weights)
    # rounded metrics: ties exist wherever the load-based plugins decide (Allocatable's normalised byte has one maximum among the
    # generator's nodes, and with a weight in the thousands it separates the totals)
    assert (want[2] > 1).any() or ALLOCATABLE in plugins
    assert want[1].max() <= sum(weights.values()) * 100 and (want[3] == n_nodes).all()
    with Engine(0) as e:   # which form ran: the fused sweep never writes TargetLoadPacking's table
        load(e)
        e.set_plugin_weights(weights)
        e.decide(mask_of(*plugins))
        for w, g in zip(want, e.best()):
            assert (w == g).all()
        if fused:
            with pytest.raises(SpxError):
                e.all_scores(TLP, 0, n_pods)
        else:
            assert e.all_scores(TLP, 0, n_pods).shape == (n_pods, n_nodes)


@pytest.mark.parametrize("row_workgroup", [0, 1])
def test_decide_with_filter_plugins_at_the_weight_thresholds(gpu_required, hdr, row_workgroup):
    """k_decide_masked is admitted for weights < 2^23 with sum(weight * 255) < 2^31 (decide_masked_ok): just under the bound it
    runs and leaves Allocatable's table unwritten; just over, and with a negative weight, spx_decide is spx_eval + spx_eval_best
    through the general int64 argmax"""
    from test_gpu_profile import ALL
    tables, filters = (ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD), (NRT, NETOVERHEAD)
    under = {ALLOCATABLE: 8388607, TLP: 32892, LVRB: 1, NRT: 1, NETOVERHEAD: 1}
    over = {**under, TLP: 32898}
    assert sum(under.values()) * 255 < 2 ** 31 <= sum(over.values()) * 255 and max(under.values()) < 2 ** 23
    with Engine(0) as e:
        e.set_option("ROW_WORKGROUP", row_workgroup)
        _full(e, hdr, 300, 200, 1, under)
        want = three_way(e, ALL, under, filters, CAPACITY)
        assert (want[0] < 0).any() and (want[0] >= 0).any() and want[1].max() > 2 ** 29
        with pytest.raises(SpxError):        # the fused form ran: nothing was written to Allocatable's table
            e.all_scores(ALLOCATABLE)
        three_way(e, ALL, over, filters, CAPACITY)
        assert e.all_scores(ALLOCATABLE).shape == (200, 300)   # the unfused route: table written
        e.set_plugin_weights(under)
        e.decide(mask_of(*ALL))
        with pytest.raises(SpxError):        # (and fused again under the bound, so that the next line says something)
            e.all_scores(ALLOCATABLE)
        negative = {ALLOCATABLE: -1, TLP: 2, LVRB: 1, NRT: 3, NETOVERHEAD: 2}
        want = three_way(e, ALL, negative, filters, CAPACITY)
        assert e.all_scores(ALLOCATABLE).shape == (200, 300)
        assert (want[0] >= 0).any()
