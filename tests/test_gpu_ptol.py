"""GPU parity (through the C ABI) for PreemptionToleration.PostFilter's preemption dry run (pkg/preemptiontoleration/
preemption_toleration.go:129-299 and upstream's pickOneNodeForPreemption).  Everything is integer: every cell's status, victim and
violation counts and pick keys, every pick, and the victim lists of the picked cells and of one cell per status are compared with the
literal oracle (tests/ptol_oracle.py) at tolerance 0.  No cell is left out.  Shapes: the wave / lane edges of the wave-per-node,
lane-per-preemptor mapping, the words of the 256-bit sets and the cap of a node's list.  The engines here never see a quota table,
except where the test is about switching between the two dry runs."""
import numpy as np
import pytest

import preempt_cases as PC
import preempt_oracle as PO
import ptol_cases as TC
import ptol_oracle as TO
import scheduler_plugins_amd as spx
from scheduler_plugins_amd import SpxError
from scheduler_plugins_amd.engine import Engine

K = spx.header().consts
SEC = TC.SEC


# ---------------------------------------------------------------------------------------------------------------- the generator (CPU)
def test_generator_reaches_every_status_level_and_exit():
    """the condition on synth.ptol_model: on the largest shape the oracle's output holds each of the six reachable statuses (SKIPPED
    with a mask too), a pick decided at each of the six levels of pickOneNodeForPreemption, and among the (preemptor, lower-priority
    pod) pairs each of the eight exits of ExemptedFromPreemption, with the last one answering both ways"""
    m, exits = TC.model(**TC.LARGEST), set()
    want = TO.dry_run(m, m["pending"], None, exits)
    assert want == TC.expected(**TC.LARGEST)
    reachable = {TO.ST[k] for k in ("CANDIDATE", "NO_VICTIMS", "NOT_FIT", "ALL_REPRIEVED", "CLASS_ERROR", "SKIPPED")}
    status = np.array([[c["status"] for c in r["cells"]] for r in want])
    assert set(np.unique(status).tolist()) == reachable
    assert (status == TO.ST["CLASS_ERROR"]).mean() < 0.1  # the missing classes sit on few nodes
    assert {r["pick"][3] for r in want} >= {1, 2, 3, 4, 5, 6}
    assert exits == set(TO.EXITS)
    by_time = {TO.exempted(m["classes"], p, pre, m["now"]) for pre in m["pending"][:50] if not pre["never"] for n in m["nodes"][:200] for p in n["pods"]
               if p["prio"] < pre["prio"] and p["pc"] in m["classes"]}
    assert by_time >= {(True, "BY_TIME"), (False, "BY_TIME")}
    masked = TC.expected(mask_seed=11, **TC.LARGEST)
    n_absent = sum(not n["present"] for n in m["nodes"])
    assert sum(c["status"] == TO.ST["SKIPPED"] for c in masked[0]["cells"]) > n_absent > 0
    assert 0.05 < np.mean([p["never"] for p in m["pending"]]) < 0.2


def test_the_undecorated_model_is_preempt_models():
    kw = dict(n_nodes=70, n_pending=66, seed=7)
    plain = PC.model(quotas=False, **kw)
    strip = lambda p: {k: v for k, v in p.items() if k not in ("pc", "scheduled_at", "never")}
    deco = TC.model(**kw)
    assert [strip(p) for p in deco["pending"]] == plain["pending"] and deco["pdbs"] == plain["pdbs"]
    assert [[strip(p) for p in n["pods"]] for n in deco["nodes"]] == [n["pods"] for n in plain["nodes"]]


def test_lists_shape_has_the_lengths_it_is_named_for():
    lens = {len(n["pods"]) for n in TC.model(**TC.SHAPES["lists"])["nodes"]}
    assert lens >= {0, 1, 31, 32, 33, 256}


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TC.SHAPES))
def test_parity_with_oracle(gpu_required, name):
    kw = TC.SHAPES[name]
    t = TC.tables(**kw)
    with Engine(0) as e:  # no quota upload
        f = e.load_preempt_toleration_objects(t)
        TC.run(e, t)
        TC.assert_dry_run(e, f, t, TC.expected(**kw))
        assert e.last_eval_ms() > 0


def pdb_model():
    """one node whose 40 pods match 32 distinct PDBs (pod k: PDB k mod 32), pod 0 three of them; budgets -1, 0 and 1 in turn"""
    m = TC.model(n_nodes=66, n_pending=65, seed=8, node_pods=(40, 3), n_pdbs=32, scenarios=False)
    m["pdbs"][:] = [(-1, 0, 1)[k % 3] for k in range(32)]
    for k, p in enumerate(m["nodes"][0]["pods"]):
        p["pdbs"] = [0, 1, 2] if k == 0 else [k % 32]
    return m


@pytest.mark.gpu
def test_pdb_budgets_a_pod_matching_three_and_32_on_one_node(gpu_required):
    m = pdb_model()
    assert len({b for p in m["nodes"][0]["pods"] for b in p["pdbs"]}) == 32 and set(m["pdbs"]) == {-1, 0, 1}
    t = spx.objects.build_preempt_toleration_tables(spx.header(), m)
    want = TO.dry_run(m, m["pending"])
    assert any(c["n_violations"] > 0 for r in want for c in r["cells"])
    with Engine(0) as e:
        f = e.load_preempt_toleration_objects(t)
        assert f["pdb_ptr"][1] - f["pdb_ptr"][0] == 32
        TC.run(e, t)
        TC.assert_dry_run(e, f, t, want)


@pytest.mark.gpu
def test_rows_out_of_order_with_gaps_and_a_node_mask(gpu_required):
    kw = TC.SHAPES["65x63"]
    rows = (40, 3, 62, 0, 17, 18, 5)
    mask = TC.node_mask(len(rows), kw["n_nodes"], 11)
    assert (mask == 0).any()
    t = TC.tables(**kw)
    with Engine(0) as e:
        f = e.load_preempt_toleration_objects(t)
        TC.run(e, t, rows)
        TC.assert_dry_run(e, f, t, TC.expected(rows=rows, **kw))
        TC.run(e, t, rows, mask)
        want = TC.expected(rows=rows, mask_seed=11, **kw)
        assert sum(c["status"] == TO.ST["SKIPPED"] for r in want for c in r["cells"]) >= int((mask == 0).sum())
        TC.assert_dry_run(e, f, t, want)


@pytest.mark.gpu
def test_three_clocks_around_the_end_of_a_toleration(gpu_required):
    """pods scheduled at now - 30 s under a 30 s toleration stop being exempted exactly when the clock reaches now: one snapshot, three
    values of now_ns, and the cells change where the oracle's do"""
    kw = TC.SHAPES["65x63"]
    t, now = TC.tables(**kw), TC.model(**kw)["now"]
    clocks = (now - 1, now, now + 1)
    wants = [TC.expected(now=c, **kw) for c in clocks]
    status = [[[c["status"] for c in r["cells"]] for r in w] for w in wants]
    assert status[0] != status[1] and status[1] == status[2]  # until == now is no longer exempted; a nanosecond later nothing else ends
    with Engine(0) as e:
        f = e.load_preempt_toleration_objects(t)
        for c, want in zip(clocks, wants):
            TC.run(e, t, now=c)
            TC.assert_dry_run(e, f, t, want)


# ---------------------------------------------------------------------------------------------------------------- state
def raises(code, fn):
    with pytest.raises(SpxError) as err:
        fn()
    assert err.value.code == code, err.value


@pytest.mark.gpu
def test_refusals_and_staleness(gpu_required):
    kw = TC.SHAPES["63x65"]
    t = TC.tables(**kw)
    STATE, ARG = K["SPX_ERR_STATE"], K["SPX_ERR_ARG"]
    fetches = lambda e: (e.preempt_cells, e.preempt_pick, e.preempt_keys, lambda: e.preempt_victims(0, 0))
    with Engine(0) as e:
        cols = {"min_preemptable": np.zeros(1, np.int32), "exempt_until_ns": np.zeros(1, np.int64), "flags": np.zeros(1, np.uint8)}
        raises(STATE, lambda: e.upload_preempt_toleration(cols))  # before spx_upload_preempt_nodes
        raises(STATE, lambda: TC.run(e, t))
        f = e.load_preempt_toleration_objects(t)
        tol = f["toleration"]
        raises(ARG, lambda: e.upload_preempt_toleration({k: v[:-1] for k, v in tol.items()}))  # a length that is not the node table's
        both = dict(tol, flags=tol["flags"].copy())
        both["flags"][3] = K["SPX_PTOL_POD_HAS_CLASS"] | K["SPX_PTOL_POD_CLASS_MISSING"]
        raises(ARG, lambda: e.upload_preempt_toleration(both))
        raises(ARG, lambda: TC.run(e, t, now=(1 << 63) - 1))
        raises(ARG, lambda: e.preempt_toleration_dry_run([len(t["priority"])], [5], [0], t["now"]))  # no row of the batch
        for again in (lambda: e.upload_preempt_toleration(tol), lambda: e.upload_preempt_nodes(f)):
            TC.run(e, t)
            e.preempt_pick()
            again()
            for fetch in fetches(e):
                raises(STATE, fetch)
        raises(STATE, lambda: TC.run(e, t))  # the nodes were uploaded again and no toleration table since
        e.upload_preempt_toleration(tol)
        TC.run(e, t)
        TC.assert_dry_run(e, f, t, TC.expected(**kw))


def both_plugins_model(**kw):
    """preempt_model WITH quotas, its pods decorated with the classes and times of the toleration model of the same shape: one node
    table that both dry runs can be asked about"""
    import copy
    m, deco = copy.deepcopy(PC.model(**kw)), TC.model(**kw)
    pool = [(p["pc"], p["scheduled_at"]) for n in deco["nodes"] for p in n["pods"]]
    for i, p in enumerate(p for n in m["nodes"] for p in n["pods"]):
        p["pc"], p["scheduled_at"] = pool[i % len(pool)]
    for i, p in enumerate(m["pending"]):
        p["never"] = i % 10 == 3
    m["classes"], m["now"] = deco["classes"], deco["now"]
    return m


@pytest.mark.gpu
def test_switching_between_the_two_dry_runs(gpu_required):
    """capacity, toleration, capacity on one engine with quotas: every fetch answers for the run before it, and the capacity results
    are the same before and after"""
    m = both_plugins_model(n_nodes=70, n_pending=66, seed=7)
    assert m["quotas"]
    t = spx.objects.build_preempt_toleration_tables(spx.header(), m)
    cwant, twant = PO.dry_run(m, m["pending"]), TO.dry_run(m, m["pending"])
    assert [[c["status"] for c in r["cells"]] for r in cwant] != [[c["status"] for c in r["cells"]] for r in twant]
    rows = np.arange(len(m["pending"]))

    def snapshot(e):
        cells, keys, pick = e.preempt_cells(), e.preempt_keys(), e.preempt_pick()
        victims = [e.preempt_victims(i, int(n)) for i, n in enumerate(pick["node"]) if n >= 0]
        return [a.tolist() for a in (*cells, *keys, *pick.values())] + [(s, v.tolist()) for s, v in victims]

    with Engine(0) as e:
        f = e.load_preempt_objects(t)  # with the quota tables
        e.preempt_dry_run(rows)
        PC.assert_dry_run(e, f, t, cwant)
        before = snapshot(e)
        e.upload_preempt_toleration(e.flatten_preempt_toleration(t["classes"], t["pod_class"], t["pod_scheduled"], t["pod_scheduled_at_ns"], f["pod_src"]))
        raises(K["SPX_ERR_STATE"], e.preempt_cells)
        TC.run(e, t)
        TC.assert_dry_run(e, f, t, twant)
        assert snapshot(e) != before
        e.preempt_dry_run(rows)
        PC.assert_dry_run(e, f, t, cwant)
        assert snapshot(e) == before


# ---------------------------------------------------------------------------------------------------------------- the reference's scenarios
@pytest.mark.gpu
def test_the_references_integration_scenarios_through_the_engine(gpu_required):
    with Engine(0) as e:
        for case in TC.golden()["integration"]:
            m = TC.golden_integration_model(case)
            t = spx.objects.build_preempt_toleration_tables(spx.header(), m)
            want = TO.dry_run(m, m["pending"])
            assert (want[0]["pick"][0] == -1) == case["can_tolerate"], case["source"]
            f = e.load_preempt_toleration_objects(t)
            TC.run(e, t)
            TC.assert_dry_run(e, f, t, want)
