"""GPU parity (through the C ABI) for CapacityScheduling's dry run with NodeResourceTopologyMatch's single-NUMA Filter in the refit
(spx_preempt_nrt_dry_run).  Everything is integer: every cell's status, victim and violation counts and pick keys, every
pick, and the victim lists of the picked cells and of one cell per status are compared with the literal oracle
(tests/preempt_nrt_oracle.py) at tolerance 0.  Shapes: the wave / lane edges of the wave-per-node, lane-per-preemptor mapping, the words
of the 256-bit sets, 1 / 2 / 8 zones, 1 and 8 slots, 1 and 8 preemptor containers (tests/preempt_nrt_cases.py)."""
import copy

import numpy as np
import pytest

import preempt_cases as PC
import preempt_nrt_cases as CC
import preempt_nrt_oracle as CO
import preempt_oracle as PO
import ptol_cases as TC
import ptol_nrt_cases as NC
import ptol_nrt_oracle as NO
import scheduler_plugins_amd as spx
from scheduler_plugins_amd import SpxError
from scheduler_plugins_amd.engine import Engine
from test_oracle_ptol_nrt import without_nrt

K = spx.header().consts
ST = PO.ST


def snapshot(e):
    """everything the fetches answer, as lists"""
    cells, keys, pick = e.preempt_cells(), e.preempt_keys(), e.preempt_pick()
    victims = [e.preempt_victims(i, int(n)) for i, n in enumerate(pick["node"]) if n >= 0]
    return [a.tolist() for a in (*cells, *keys, *pick.values())] + [(s, v.tolist()) for s, v in victims]


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CC.SHAPES))
def test_parity_with_oracle(gpu_required, name):
    kw = CC.SHAPES[name]
    t = CC.tables(**kw)
    with Engine(0) as e:
        f = CC.load(e, t)
        assert f["nrt"]["R"] == {"64x64": 8, "one-slot": 1}.get(name, f["nrt"]["R"])
        if name == "lists":
            assert {len(n["pods"]) for n in CC.model(**kw)["nodes"]} >= {0, 1, 31, 32, 33, 256}
        CC.run(e, t)
        CC.assert_dry_run(e, f, t, CC.expected(**kw))
        assert e.last_eval_ms() > 0


@pytest.mark.gpu
def test_mode_disabled_against_the_oracle_and_where_the_modes_differ(gpu_required):
    kw = CC.LARGEST
    t = CC.tables(**kw)
    on, off = CC.expected(**kw), CC.expected(mode=False, **kw)
    assert [[c["status"] for c in r["cells"]] for r in on] != [[c["status"] for c in r["cells"]] for r in off]
    with Engine(0) as e:
        f = CC.load(e, t)
        CC.run(e, t, mode=False)
        CC.assert_dry_run(e, f, t, off)
        CC.run(e, t, mode=True)
        CC.assert_dry_run(e, f, t, on)


def pdb_model():
    """one node whose 40 pods match 32 distinct PDBs, budgets -1, 0 and 1 in turn; decorated"""
    m = copy.deepcopy(PC.model(n_nodes=66, n_pending=65, seed=8, node_pods=(40, 3), n_pdbs=32, scenarios=False))
    m["pdbs"][:] = [(-1, 0, 1)[k % 3] for k in range(32)]
    for k, p in enumerate(m["nodes"][0]["pods"]):
        p["pdbs"] = [0, 1, 2] if k == 0 else [k % 32]
    return NC.decorate(m, 8, zones=(2, 8), max_ctrs=3)


@pytest.mark.gpu
def test_32_pdbs_on_one_node(gpu_required):
    m = pdb_model()
    t = CC.build_tables(m)
    want = CO.dry_run(m, m["pending"])
    assert any(c["n_violations"] > 0 for r in want for c in r["cells"])
    with Engine(0) as e:
        f = CC.load(e, t)
        assert f["pdb_ptr"][1] - f["pdb_ptr"][0] == 32
        CC.run(e, t)
        CC.assert_dry_run(e, f, t, want)


@pytest.mark.gpu
def test_rows_out_of_order_with_gaps_and_a_node_mask(gpu_required):
    kw = CC.SHAPES["63x65"]
    rows = (40, 3, 62, 0, 17, 18, 5)
    mask = CC.node_mask(len(rows), kw["n_nodes"], 11)
    assert (mask == 0).any()
    t = CC.tables(**kw)
    with Engine(0) as e:
        f = CC.load(e, t)
        CC.run(e, t, rows)
        CC.assert_dry_run(e, f, t, CC.expected(rows=rows, **kw))
        CC.run(e, t, rows, mask)
        want = CC.expected(rows=rows, mask_seed=11, **kw)
        assert sum(c["status"] == ST["SKIPPED"] for r in want for c in r["cells"]) >= int((mask == 0).sum())
        CC.assert_dry_run(e, f, t, want)


# ---------------------------------------------------------------------------------------------------------------- the constructed directions
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CC.DIRECTIONS))
def test_the_filter_changes_the_outcome(gpu_required, name):
    m, with_filter, fit_only = CC.DIRECTIONS[name]
    want = CO.dry_run(m, m["pending"])
    assert (want[0]["cells"][0]["status"], want[0]["cells"][0]["victims"]) == with_filter
    plain = PO.dry_run(m, m["pending"])
    assert (plain[0]["cells"][0]["status"], plain[0]["cells"][0]["victims"]) == fit_only
    t = CC.build_tables(m)
    with Engine(0) as e:
        f = CC.load(e, t)
        CC.run(e, t)
        CC.assert_dry_run(e, f, t, want)
        got = e.preempt_victims(0, 0)
        assert (got[0], [PC.model_position(f, t, 0, p) for p in got[1]]) == with_filter
        CC.run_fit_only(e, t)  # spx_preempt_dry_run on the same upload gives the other answer
        CC.assert_dry_run(e, f, t, plain)
        got = e.preempt_victims(0, 0)
        assert (got[0], [PC.model_position(f, t, 0, p) for p in got[1]]) == fit_only


# ---------------------------------------------------------------------------------------------------------------- next to the other dry runs
@pytest.mark.gpu
def test_without_any_nrt_it_is_the_old_dry_run_byte_for_byte(gpu_required):
    m = without_nrt(CC.model(**CC.SHAPES["65x63"]))
    t = CC.build_tables(m)
    with Engine(0) as e:
        f = CC.load(e, t)
        assert not (f["nrt"]["node_flags"] & K["SPX_NRT_F_HAS_NRT"]).any()
        CC.run_fit_only(e, t)
        old = snapshot(e)
        CC.assert_dry_run(e, f, t, PO.dry_run(m, m["pending"]))
        for mode in (True, False):
            CC.run(e, t, mode=mode)
            assert snapshot(e) == old


def both_plugins_model(**kw):
    """preempt_nrt_cases' model (quotas, NRT view) with ptol_model's decoration: a snapshot all three dry runs can be asked about"""
    m, deco = copy.deepcopy(CC.model(**kw)), TC.model(**{k: v for k, v in kw.items() if k not in ("zones", "max_ctrs", "extra", "one_slot")})
    pool = [(p["pc"], p["scheduled_at"]) for n in deco["nodes"] for p in n["pods"]]
    for i, p in enumerate(p for n in m["nodes"] for p in n["pods"]):
        p["pc"], p["scheduled_at"] = pool[i % len(pool)]
    for i, p in enumerate(m["pending"]):
        p["never"] = i % 10 == 3
    m["classes"], m["now"] = deco["classes"], deco["now"]
    return m


@pytest.mark.gpu
def test_the_other_dry_runs_are_the_same_before_and_after(gpu_required):
    """spx_preempt_dry_run and spx_preempt_toleration_nrt_dry_run on one engine, then the new entry, then both again: each gives what
    it gave, and the fetches after a later spx_preempt_dry_run answer for that run"""
    m = both_plugins_model(**CC.SHAPES["63x65"])
    assert m["quotas"]
    hdr = spx.header()
    t = spx.objects.build_preempt_toleration_tables(hdr, m)
    t.update(NC.nrt_tables(hdr, m))
    cwant, twant, want = PO.dry_run(m, m["pending"]), NO.dry_run(m, m["pending"]), CO.dry_run(m, m["pending"])
    with Engine(0) as e:
        f = CC.load(e, t)
        e.upload_preempt_toleration(e.flatten_preempt_toleration(t["classes"], t["pod_class"], t["pod_scheduled"], t["pod_scheduled_at_ns"], f["pod_src"]))
        CC.run_fit_only(e, t)
        CC.assert_dry_run(e, f, t, cwant)
        capacity = snapshot(e)
        NC.run(e, t)
        NC.assert_dry_run(e, f, t, twant)
        toleration = snapshot(e)
        CC.run(e, t)
        CC.assert_dry_run(e, f, t, want)
        mine = snapshot(e)
        assert mine != capacity and mine != toleration
        NC.run(e, t)
        assert snapshot(e) == toleration
        CC.run(e, t)
        assert snapshot(e) == mine
        CC.run_fit_only(e, t)  # the fetches answer for the run that came last
        assert snapshot(e) == capacity
        CC.assert_dry_run(e, f, t, cwant)


# ---------------------------------------------------------------------------------------------------------------- state
def raises(code, fn):
    with pytest.raises(SpxError) as err:
        fn()
    assert err.value.code == code, err.value
    return err.value.msg


@pytest.mark.gpu
def test_refusals_and_staleness(gpu_required):
    kw = CC.SHAPES["63x65"]
    t = CC.tables(**kw)
    STATE, ARG = K["SPX_ERR_STATE"], K["SPX_ERR_ARG"]
    fetches = lambda e: (e.preempt_cells, e.preempt_pick, e.preempt_keys, lambda: e.preempt_victims(0, 0))
    with Engine(0) as e:
        raises(STATE, lambda: CC.run(e, t))  # nothing uploaded
        f = e.load_preempt_objects(t)
        assert "spx_upload_preempt_nrt" in raises(STATE, lambda: CC.run(e, t))  # no side table yet; the toleration table is never needed
        g = NC.flatten_nrt(e, t, f)
        e.upload_preempt_nrt(g)
        raises(ARG, lambda: e.preempt_nrt_dry_run([], None))  # an empty row list
        raises(ARG, lambda: e.preempt_nrt_dry_run([int(t["pods"].struct.n_pods)], None))  # no row of the batch
        raises(ARG, lambda: e.preempt_nrt_dry_run([-1], None))
        with pytest.raises(ValueError):
            e.preempt_nrt_dry_run([0, 1], np.ones((1, e.n_nodes), np.uint8))
        for again in (lambda: e.upload_preempt_nrt(g), lambda: e.upload_preempt_nominated_quota(f["nominated_quota"]), lambda: e.upload_preempt_pods(np.zeros((e.n_pods, 8), np.int64))):
            CC.run(e, t)
            e.preempt_pick()
            again()
            for fetch in fetches(e):
                raises(STATE, fetch)  # an upload marks results stale
        assert "spx_upload_preempt_nrt" in raises(STATE, lambda: CC.run(e, t))  # spx_upload_preempt_pods dropped the side table
        f = CC.load(e, t)
        CC.run(e, t)
        e.upload_preempt_nodes(f)  # drops the side table
        for fetch in fetches(e):
            raises(STATE, fetch)
        assert "spx_upload_preempt_nrt" in raises(STATE, lambda: CC.run(e, t))
        CC.run_fit_only(e, t)  # the old dry run needs no side table
        PC.assert_dry_run(e, f, t, PO.dry_run(CC.model(**kw), CC.model(**kw)["pending"]))
        e.upload_preempt_nrt(g)
        CC.run(e, t)
        CC.assert_dry_run(e, f, t, CC.expected(**kw))


# ---------------------------------------------------------------------------------------------------------------- zones that share a NUMA id
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NC.TWIN_MODELS))
def test_twin_zones_and_the_accounting_error(gpu_required, name):
    """nodes that list one NUMA id twice: the charge and the release land on both twins, and a twin charged below zero is the Filter's
    fwk.Error — no candidate, no reprieve (tests/test_nrt_refit_twins_host.py shows the models hold that edge)"""
    m = CC.twin_models()[name]
    trace = set()
    want = CO.dry_run(m, m["pending"], trace=trace)
    assert "accounting-error" in trace
    t = CC.build_tables(m)
    with Engine(0) as e:
        f = CC.load(e, t)
        CC.run(e, t)
        CC.assert_dry_run(e, f, t, want)
