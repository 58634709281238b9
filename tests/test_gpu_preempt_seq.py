"""GPU parity (through the C ABI) for CapacityScheduling's sequential preemption loop (spx_preempt_sequential) with the
literal loop of tests/preempt_seq_oracle.py, at tolerance 0: every row's pick with its candidate and tie counts, every cell's status,
counts and five keys as the row saw them at its own step, and the stored victim list of every picked cell.  Models: the generator
retuned so that quotas sit around their min (preempt_seq_cases: Used moves, over-min branches flip, cells change on nodes no step
touched), the generator as it is, and one hand-built model per effect.  Shapes: the wave / lane edges of the column kernel's four nodes
per workgroup, 257 rows (past a 256-row block of the cell buffer), a node at the cap of 256 pods with 32 PDBs.  The oracle's answers
are computed once per case and shared (preempt_seq_cases.expected)."""
import copy

import numpy as np
import pytest

import preempt_cases as PC
import preempt_oracle as PO
import preempt_seq_cases as SC
import preempt_seq_oracle as SO
import ptol_seq_cases as TSC
import ptol_seq_oracle as TSO
import scheduler_plugins_amd as spx
from scheduler_plugins_amd import SpxError
from scheduler_plugins_amd.engine import Engine
from test_gpu_ptol import both_plugins_model

K = spx.header().consts
STATE, ARG = K["SPX_ERR_STATE"], K["SPX_ERR_ARG"]


def raises(code, fn):
    with pytest.raises(SpxError) as err:
        fn()
    assert err.value.code == code, err.value


def snapshot(e):
    """everything the fetches give, the victims of every picked cell included"""
    cells, keys, pick = e.preempt_cells(), e.preempt_keys(), e.preempt_pick()
    victims = [e.preempt_victims(i, int(n)) for i, n in enumerate(pick["node"]) if n >= 0]
    return [a.tolist() for a in (*cells, *keys, *pick.values())] + [(s, v.tolist()) for s, v in victims]


def check_model(m, mask=None, eligible=None):
    """one model through the tables, the engine's loop and the literal loop"""
    t = spx.objects.build_preempt_tables(spx.header(), m)
    want = SO.run(m, m["pending"], mask, eligible)
    with Engine(0) as e:
        f = e.load_preempt_objects(t)
        SC.run(e, t, mask=mask, eligible=eligible)
        SC.assert_sequential(e, f, t, want)
    return want


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.gpu
@pytest.mark.parametrize("kind,name", [("retuned", n) for n in SC.RETUNED] + [("plain", n) for n in SC.PLAIN])
def test_parity_with_the_literal_loop(gpu_required, kind, name):
    kw = (SC.RETUNED if kind == "retuned" else SC.PLAIN)[name]
    t = SC.tables(kind, **kw)
    want, counters = SC.expected(kind, **kw)
    if (kind, name) == ("retuned", "200x257"):
        assert len(want) == 257 and counters["used_moved"] > 100 and counters["untouched_cells_differ"] > 1000
    with Engine(0) as e:
        f = e.load_preempt_objects(t)
        SC.run(e, t)
        SC.assert_sequential(e, f, t, want)
        assert e.last_eval_ms() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SC.HAND))
def test_the_hand_built_models(gpu_required, name):
    m, mask, eligible, what = SC.HAND[name]()
    want = check_model(m, mask, eligible)
    c = want[what["row"]]["cells"][what["node"]]
    assert (c["status"], c["victims"]) == what["seq"]


@pytest.mark.gpu
def test_rows_out_of_order_with_a_node_mask(gpu_required):
    kw = SC.RETUNED["65x63"]
    rows = (40, 3, 62, 0, 17, 18, 5, 61, 33, 2, 50, 9)
    mask = PC.node_mask(len(rows), kw["n_nodes"], 11)
    assert (mask == 0).any()
    t = SC.tables("retuned", **kw)
    with Engine(0) as e:
        f = e.load_preempt_objects(t)
        SC.run(e, t, rows)
        SC.assert_sequential(e, f, t, SC.expected("retuned", rows=rows, **kw)[0])
        SC.run(e, t, rows, mask)
        want, counters = SC.expected("retuned", rows=rows, mask_seed=11, **kw)
        assert counters["applied"] == len(rows) and sum(r["pick"][0] >= 0 for r in want) > 1
        SC.assert_sequential(e, f, t, want)


@pytest.mark.gpu
def test_rows_that_are_not_eligible_are_evaluated_and_move_nothing(gpu_required):
    kw = SC.RETUNED["64x64"]
    t = SC.tables("retuned", **kw)
    eligible = SC.eligible_column(kw["n_pending"], 21)
    assert 0 < eligible.sum() < len(eligible)
    want, counters = SC.expected("retuned", eligible_seed=21, **kw)
    assert counters["applied"] == eligible.sum() < SC.expected("retuned", **kw)[1]["applied"]
    assert [r["pick"] for r in want] != [r["pick"] for r in SC.expected("retuned", **kw)[0]]
    with Engine(0) as e:
        f = e.load_preempt_objects(t)
        SC.run(e, t, eligible=eligible)
        SC.assert_sequential(e, f, t, want)


@pytest.mark.gpu
def test_every_row_alone_is_the_dry_run_of_that_row(gpu_required):
    """a one-row loop is spx_preempt_dry_run of that row, bit for bit: the side table's sums against the quota table's"""
    kw = SC.RETUNED["63x65"]
    t = SC.tables("retuned", **kw)
    m = SC.model("retuned", **kw)
    assert sum(len(nd["nominated"]) for nd in m["nodes"]) > 0
    with Engine(0) as e:
        e.load_preempt_objects(t)
        picked = 0
        for r in range(kw["n_pending"]):
            e.preempt_dry_run([r])
            batch = snapshot(e)
            e.preempt_sequential([r])
            assert snapshot(e) == batch, r
            picked += batch[6][0] >= 0
        assert picked > 10


@pytest.mark.gpu
@pytest.mark.parametrize("case", PC.golden()["dry_run"] + PC.golden()["post_filter"], ids=lambda c: c["name"])
def test_the_references_tables_as_one_row_loops(gpu_required, case):
    m = PC.golden_model(case)
    want = check_model(m)
    assert want == PO.dry_run(m, m["pending"]) and want[0]["pick"][0] == 0


def cap_model():
    """test_gpu_preempt's lists shape with the retuned quotas; its first node of 256 pods is exactly full (Allocatable = what its pods
    charge, 256 pods allowed), so that every preemptor has to evict there, and carries 32 PDBs: pod k matches PDB k mod 32, pod 0 three"""
    m = copy.deepcopy(PC.model(n_nodes=14, n_pending=65, seed=6, node_pods=(0, 1, 31, 32, 33, 256, 64), n_pdbs=32, scenarios=False))
    for ns, q in m["quotas"].items():
        q["min"] = {"v": [int(u * SC.RETUNE_F[ns]) for u in q["used"]["v"]], "p": q["used"]["p"]}
        q["max"] = {"v": [SC.INT64_MAX] * 3 + [0] * 5, "p": 0}
    node = m["nodes"][5]
    node["alloc"] = [sum(p["fit"][s] for p in node["pods"]) if s != 3 else 256 for s in range(8)]
    m["pdbs"][:] = [(-1, 0, 1, 2)[k % 4] for k in range(32)]
    for k, p in enumerate(node["pods"]):
        p["pdbs"] = [0, 1, 2] if k == 0 else [k % 32]
    return m


@pytest.mark.gpu
def test_a_node_with_256_pods_and_32_pdbs(gpu_required):
    m = cap_model()
    assert len(m["nodes"][5]["pods"]) == 256 and len({b for p in m["nodes"][5]["pods"] for b in p["pdbs"]}) == 32
    want = check_model(m)
    assert sum(r["pick"][0] == 5 for r in want) > 1  # the node is picked, its set shrinks, and it is picked again
    assert any(c["n_violations"] > 0 for r in want for c in r["cells"])


# ---------------------------------------------------------------------------------------------------------------- state
@pytest.mark.gpu
def test_the_batch_dry_run_is_the_same_before_and_after_the_loop(gpu_required):
    kw = SC.RETUNED["65x63"]
    t = SC.tables("retuned", **kw)
    rows = np.arange(kw["n_pending"])
    with Engine(0) as e:
        f = e.load_preempt_objects(t)
        e.preempt_dry_run(rows)
        PC.assert_dry_run(e, f, t, SC.frozen("retuned", **kw))
        before = snapshot(e)
        SC.run(e, t)
        SC.assert_sequential(e, f, t, SC.expected("retuned", **kw)[0])
        assert snapshot(e) != before
        e.preempt_dry_run(rows)
        assert snapshot(e) == before
        PC.assert_dry_run(e, f, t, SC.frozen("retuned", **kw))  # one cell per status again, not only the picked ones
        SC.run(e, t)  # and the loop starts from the uploaded state every time
        SC.assert_sequential(e, f, t, SC.expected("retuned", **kw)[0])


@pytest.mark.gpu
def test_the_toleration_loop_is_the_same_before_and_after_the_capacity_loop(gpu_required):
    m = both_plugins_model(n_nodes=70, n_pending=66, seed=7)
    t = spx.objects.build_preempt_toleration_tables(spx.header(), m)
    twant, cwant = TSO.run(m, m["pending"]), SO.run(m, m["pending"])
    with Engine(0) as e:
        f = e.load_preempt_objects(t)  # with the quota tables and the side table
        e.upload_preempt_toleration(e.flatten_preempt_toleration(t["classes"], t["pod_class"], t["pod_scheduled"], t["pod_scheduled_at_ns"], f["pod_src"]))
        TSC.run(e, t)
        TSC.assert_sequential(e, f, t, twant)
        before = snapshot(e)
        SC.run(e, t)
        SC.assert_sequential(e, f, t, cwant)
        assert snapshot(e) != before
        TSC.run(e, t)
        assert snapshot(e) == before
        SC.run(e, t)
        SC.assert_sequential(e, f, t, cwant)


@pytest.mark.gpu
def test_refusals_and_staleness(gpu_required):
    kw = SC.RETUNED["63x65"]
    t = SC.tables("retuned", **kw)
    want, _ = SC.expected("retuned", **kw)
    fetches = lambda e: (e.preempt_cells, e.preempt_pick, e.preempt_keys, lambda: e.preempt_victims(0, 0))
    with Engine(0) as e:
        raises(STATE, lambda: SC.run(e, t))  # no tables
        f = e.load_preempt_objects(t)
        side, M = f["nominated_quota"], len(f["nom_priority"])
        assert M > 0
        raises(ARG, lambda: e.preempt_sequential([kw["n_pending"]]))  # no row of the batch
        raises(ARG, lambda: e.preempt_sequential([3, 7, 3]))  # a row listed twice
        raises(ARG, lambda: e.preempt_sequential([]))
        raises(ARG, lambda: e.upload_preempt_nominated_quota({k: v[:M - 1] for k, v in side.items()}))  # not the node table's count
        fq = e.flatten_quota(t["pods"], t["rc"], t["quota"])
        used = fq["ns"]["used"].reshape(-1, 8)
        uploads = (lambda: e.upload_preempt_nominated_quota(side), lambda: e.upload_preempt_pods(fq["cols"]["pod_req"].reshape(-1, 8)), lambda: e.upload_quota(fq),
                   lambda: e.update_quota_used([0], used[0], fq["ns"]["used_present"][:1], fq["cols"]["agg_used"], fq["cols"]["agg_used_present"]),
                   lambda: e.upload_preempt_nodes(f))
        for again in uploads:  # every upload
            SC.run(e, t)
            e.preempt_pick()
            again()
            for fetch in fetches(e):
                raises(STATE, fetch)
        raises(STATE, lambda: SC.run(e, t))  # the nodes were uploaded again and no side table since
        e.upload_preempt_nominated_quota(side)
        SC.run(e, t)
        SC.assert_sequential(e, f, t, want)
        # the victims of a cell other than the picked one: the state it saw is gone
        i = next(i for i, r in enumerate(want) if r["pick"][0] >= 0 and r["pick"][1] > 1)
        other = next(n for n, c in enumerate(want[i]["cells"]) if c["status"] == PO.ST["CANDIDATE"] and n != want[i]["pick"][0])
        raises(ARG, lambda: e.preempt_victims(i, other))
        none = next(i for i, r in enumerate(want) if r["pick"][0] < 0)
        raises(ARG, lambda: e.preempt_victims(none, 0))
        assert e.preempt_victims(i, want[i]["pick"][0])[0] == PO.ST["CANDIDATE"]  # the refusals left the results in place


@pytest.mark.gpu
def test_a_node_table_without_nominated_records_needs_no_side_table(gpu_required):
    m = copy.deepcopy(SC.model("retuned", **SC.RETUNED["12x40"]))
    for nd in m["nodes"]:
        nd["nominated"] = []
    t = spx.objects.build_preempt_tables(spx.header(), m)
    want = SO.run(m, m["pending"])
    with Engine(0) as e:
        f = e.load_preempt_objects(t)
        e.upload_preempt_nodes(f)  # drops the (empty) side table
        SC.run(e, t)
        SC.assert_sequential(e, f, t, want)
