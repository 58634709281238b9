"""GPU parity (through the C ABI) for PreemptionToleration's sequential preemption loop with NodeResourceTopologyMatch's single-NUMA
Filter in the refit (spx_preempt_toleration_nrt_sequential) with the literal loop of tests/ptol_nrt_seq_oracle.py, at
tolerance 0 and through ptol_seq_cases.assert_sequential's fields: every row's pick, candidate and tie counts, every cell's status,
counts and five keys as the row saw them at its own step, and the stored victim list of every picked cell.  Shapes: those of the NRT dry
run's suite (tests/ptol_nrt_cases.py); 257 x 3 straddles the 64-row blocks of the re-evaluation, so that blocks leave early and lanes of
finished rows store nothing.  The oracle's answers are computed once per case and shared (ptol_nrt_seq_cases.expected)."""
import numpy as np
import pytest

import ptol_nrt_cases as NC
import ptol_nrt_oracle as NO
import ptol_nrt_seq_cases as NSC
import ptol_nrt_seq_oracle as NSO
import ptol_oracle as TO
import ptol_seq_cases as SC
import ptol_seq_oracle as SO
import scheduler_plugins_amd as spx
from preempt_cases import model_position
from scheduler_plugins_amd import SpxError
from scheduler_plugins_amd.engine import Engine
from test_oracle_ptol_nrt import without_nrt

K = spx.header().consts
ST = TO.ST


def raises(code, fn):
    with pytest.raises(SpxError) as err:
        fn()
    assert err.value.code == code, err.value
    return err.value.msg


def snapshot(e):
    """everything the fetches give, the victims of every picked cell included"""
    cells, keys, pick = e.preempt_cells(), e.preempt_keys(), e.preempt_pick()
    victims = [e.preempt_victims(i, int(n)) for i, n in enumerate(pick["node"]) if n >= 0]
    return [a.tolist() for a in (*cells, *keys, *pick.values())] + [(s, v.tolist()) for s, v in victims]


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NC.SHAPES))
def test_parity_with_the_literal_loop(gpu_required, name):
    kw = NC.SHAPES[name]
    t = NC.tables(**kw)
    want, _ = NSC.expected(**kw)
    with Engine(0) as e:  # no quota upload
        f = NC.load(e, t)
        NSC.run(e, t)
        NSC.assert_sequential(e, f, t, want)
        assert e.last_eval_ms() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["64x64", "257x3"])
def test_mode_off_is_the_ordinary_filter_at_every_step(gpu_required, name):
    kw = NC.SHAPES[name]
    t = NC.tables(**kw)
    on, off = NSC.expected(**kw)[0], NSC.expected(mode=False, **kw)[0]
    assert NSC.differing_rows(on, off) > 0
    with Engine(0) as e:
        f = NC.load(e, t)
        NSC.run(e, t, mode=False)
        NSC.assert_sequential(e, f, t, off)
        NSC.run(e, t, mode=True)
        NSC.assert_sequential(e, f, t, on)


@pytest.mark.gpu
def test_the_second_visit_pins_t5(gpu_required):
    """a pod evicted at an earlier step releases nothing at a later one; the fit-only loop, the frozen NRT batch and the loop with mode
    off give their other answers on the same upload"""
    m = NSC.second_visit_model()
    want = NSC.SECOND_VISIT
    t = NC.build_tables(m)

    def end(i):  # (pick, status, victims) of row i as the fetches give them
        n = int(e.preempt_pick()["node"][i])
        if n < 0:
            return (n, int(e.preempt_cells()[0][i, 0]), [])
        status, pos = e.preempt_victims(i, n)
        return (n, status, [model_position(f, t, n, p) for p in pos])

    with Engine(0) as e:
        f = NC.load(e, t)
        loop = NSO.run(m, m["pending"])
        assert [NSC.end(r) for r in loop] == want["loop"]
        NSC.run(e, t)
        NSC.assert_sequential(e, f, t, loop)
        assert [end(0), end(1)] == want["loop"]
        SC.run(e, t)  # spx_preempt_toleration_sequential
        SC.assert_sequential(e, f, t, SO.run(m, m["pending"]))
        assert end(1) == want["fit_only_p1"]
        NC.run(e, t)  # spx_preempt_toleration_nrt_dry_run
        NC.assert_dry_run(e, f, t, NO.dry_run(m, m["pending"]))
        assert end(1) == want["frozen_p1"]
        NSC.run(e, t, mode=False)
        NSC.assert_sequential(e, f, t, NSO.run(m, m["pending"], mode=False))
        assert [end(0), end(1)] == want["mode_off"]


@pytest.mark.gpu
def test_rows_out_of_order_with_a_node_mask(gpu_required):
    kw = NC.SHAPES["65x63"]
    rows = (40, 3, 62, 0, 17, 18, 5, 61, 33, 2, 50, 9)
    mask = NC.node_mask(len(rows), kw["n_nodes"], 11)
    assert (mask == 0).any()
    t = NC.tables(**kw)
    with Engine(0) as e:
        f = NC.load(e, t)
        NSC.run(e, t, rows)
        NSC.assert_sequential(e, f, t, NSC.expected(rows=rows, **kw)[0])
        NSC.run(e, t, rows, mask)
        want, counters = NSC.expected(rows=rows, mask_seed=11, **kw)
        assert counters["applied"] > 1
        NSC.assert_sequential(e, f, t, want)


@pytest.mark.gpu
def test_rows_that_are_not_eligible_are_evaluated_and_move_nothing(gpu_required):
    kw = NC.SHAPES["64x64"]
    t = NC.tables(**kw)
    eligible = NSC.eligible_column(kw["n_pending"], 21)
    assert 0 < eligible.sum() < len(eligible)
    want, counters = NSC.expected(eligible_seed=21, **kw)
    assert counters["applied"] < NSC.expected(**kw)[1]["applied"]
    assert [r["pick"] for r in want] != [r["pick"] for r in NSC.expected(**kw)[0]]
    with Engine(0) as e:
        f = NC.load(e, t)
        NSC.run(e, t, eligible=eligible)
        NSC.assert_sequential(e, f, t, want)


# ---------------------------------------------------------------------------------------------------------------- next to the runs the tree had
@pytest.mark.gpu
def test_a_list_of_preempt_never_rows_is_the_nrt_dry_run_byte_for_byte(gpu_required):
    kw = NC.SHAPES["63x65"]
    t = NC.tables(**kw)
    rows = np.arange(kw["n_pending"])
    never = np.ones(len(rows), np.uint8)
    m = NC.model(**kw)
    pres = [dict(p, never=True) for p in m["pending"]]
    want = NO.dry_run(m, pres)
    assert any(r["pick"][0] >= 0 for r in want)
    with Engine(0) as e:
        f = NC.load(e, t)
        e.preempt_toleration_nrt_dry_run(rows, t["priority"], never, t["now"])
        NC.assert_dry_run(e, f, t, want)
        batch = snapshot(e)
        e.preempt_toleration_nrt_sequential(rows, t["priority"], never, t["now"])
        NSC.assert_sequential(e, f, t, want)
        assert snapshot(e) == batch


@pytest.mark.gpu
def test_without_any_nrt_it_is_the_fit_only_loop_byte_for_byte(gpu_required):
    m = without_nrt(NC.model(**NC.SHAPES["65x63"]))
    t = NC.build_tables(m)
    with Engine(0) as e:
        f = NC.load(e, t)
        assert not (f["nrt"]["node_flags"] & K["SPX_NRT_F_HAS_NRT"]).any()
        SC.run(e, t)
        old = snapshot(e)
        SC.assert_sequential(e, f, t, SO.run(m, m["pending"]))
        for mode in (True, False):
            NSC.run(e, t, mode=mode)
            assert snapshot(e) == old


@pytest.mark.gpu
def test_the_uploaded_tables_are_never_written(gpu_required):
    """NRT dry run -> loop -> NRT dry run, and fit-only loop -> this loop -> fit-only loop, with identical results"""
    kw = NC.SHAPES["65x63"]
    t = NC.tables(**kw)
    with Engine(0) as e:
        f = NC.load(e, t)
        NC.run(e, t)
        batch = snapshot(e)
        NSC.run(e, t)
        NSC.assert_sequential(e, f, t, NSC.expected(**kw)[0])
        assert snapshot(e) != batch
        NC.run(e, t)
        assert snapshot(e) == batch
        NC.assert_dry_run(e, f, t, NC.expected(**kw))
        SC.run(e, t)
        plain = snapshot(e)
        NSC.run(e, t)  # the loop starts from the uploaded state every time
        NSC.assert_sequential(e, f, t, NSC.expected(**kw)[0])
        assert snapshot(e) != plain
        SC.run(e, t)
        assert snapshot(e) == plain
        SC.assert_sequential(e, f, t, NSC.fit_only(**kw))


# ---------------------------------------------------------------------------------------------------------------- state
@pytest.mark.gpu
def test_refusals_and_staleness(gpu_required):
    kw = NC.SHAPES["63x65"]
    t = NC.tables(**kw)
    want, _ = NSC.expected(**kw)
    STATE, ARG = K["SPX_ERR_STATE"], K["SPX_ERR_ARG"]
    fetches = lambda e: (e.preempt_cells, e.preempt_pick, e.preempt_keys, lambda: e.preempt_victims(0, 0))
    with Engine(0) as e:
        raises(STATE, lambda: NSC.run(e, t))  # no tables
        f = e.load_preempt_toleration_objects(t)
        g = NC.flatten_nrt(e, t, f)
        assert "spx_upload_preempt_nrt" in raises(STATE, lambda: NSC.run(e, t))  # no side table yet
        e.upload_preempt_nrt(g)
        raises(ARG, lambda: NSC.run(e, t, now=(1 << 63) - 1))
        raises(ARG, lambda: e.preempt_toleration_nrt_sequential([len(t["priority"])], [5], [0], t["now"]))  # no row of the batch
        assert "twice" in raises(ARG, lambda: e.preempt_toleration_nrt_sequential([3, 7, 3], [5, 5, 5], [0, 0, 0], t["now"]))  # a row listed twice
        raises(ARG, lambda: e.preempt_toleration_nrt_sequential([], [], [], t["now"]))  # an empty list
        fit = e.flatten_quota(t["pods"], t["rc"], t["quota"])["cols"]["pod_req"].reshape(-1, 8)
        uploads = (lambda: e.upload_preempt_nrt(g), lambda: e.upload_preempt_toleration(f["toleration"]), lambda: (e.upload_preempt_pods(fit), e.upload_preempt_nrt(g)),
                   lambda: e.upload_preempt_nodes(f))
        for again in uploads:  # every upload marks the results stale
            NSC.run(e, t)
            e.preempt_pick()
            again()
            for fetch in fetches(e):
                raises(STATE, fetch)
        # the nodes were uploaded again: neither the toleration table nor the side table is in place
        assert "spx_upload_preempt_toleration" in raises(STATE, lambda: NSC.run(e, t))
        e.upload_preempt_toleration(f["toleration"])
        assert "spx_upload_preempt_nrt" in raises(STATE, lambda: NSC.run(e, t))
        SC.run(e, t)  # the fit-only loop needs no side table
        e.upload_preempt_nrt(g)
        NSC.run(e, t)
        NSC.assert_sequential(e, f, t, want)
        # the victims of a cell other than the picked one: the state it saw is gone
        i = next(i for i, r in enumerate(want) if r["pick"][0] >= 0 and r["pick"][1] > 1)
        other = next(n for n, c in enumerate(want[i]["cells"]) if c["status"] == ST["CANDIDATE"] and n != want[i]["pick"][0])
        raises(ARG, lambda: e.preempt_victims(i, other))
        none = next(i for i, r in enumerate(want) if r["pick"][0] < 0)
        raises(ARG, lambda: e.preempt_victims(none, 0))
        assert e.preempt_victims(i, want[i]["pick"][0])[0] == ST["CANDIDATE"]  # the refusals left the results in place


# ---------------------------------------------------------------------------------------------------------------- zones that share a NUMA id
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NC.TWIN_MODELS))
def test_twin_zones_and_the_accounting_error(gpu_required, name):
    """the loop over nodes that list one NUMA id twice: a twin charged below zero is the Filter's fwk.Error at every step, and a later
    row meets the node an earlier one changed"""
    m = NC.twin_models()[name]
    want = NSO.run(m, m["pending"])
    t = NC.build_tables(m)
    with Engine(0) as e:
        f = NC.load(e, t)
        NSC.run(e, t)
        NSC.assert_sequential(e, f, t, want)
