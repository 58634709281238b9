"""GPU parity (through the C ABI) for CapacityScheduling.PostFilter's preemption dry run (capacity_scheduling.go:486-677, :889-934, and
upstream's pickOneNodeForPreemption).  Everything is integer: every cell's status, victim and violation counts and pick keys, every
pick, and the victim lists of the picked cells and of one cell per status are compared with the literal oracle
(tests/preempt_oracle.py) at tolerance 0.  No cell is left out.  Ties in (priority, start time) are part of the data: both sides break
them by the order of the table.  Shapes: the wave / lane edges of the wave-per-node, lane-per-preemptor mapping (and of its
transpose), the words of the 256-bit sets and the cap of a node's list."""
import numpy as np
import pytest

import preempt_cases as PC
import preempt_oracle as PO
import scheduler_plugins_amd as spx
from scheduler_plugins_amd import SpxError
from scheduler_plugins_amd.engine import Engine

SHAPES = {
    "1x1": dict(n_nodes=1, n_pending=1, seed=14, pods_per_node=6.0),
    "63x65": dict(n_nodes=63, n_pending=65, seed=3),
    "64x64": dict(n_nodes=64, n_pending=64, seed=4),
    "65x63": dict(n_nodes=65, n_pending=63, seed=5),
    "1030x200": PC.LARGEST,
    "lists": dict(n_nodes=14, n_pending=65, seed=6, node_pods=(0, 1, 31, 32, 33, 256, 64)),
    "no-quotas": dict(n_nodes=70, n_pending=66, seed=7, quotas=False),
}


def test_generator_reaches_every_status_and_every_level_of_the_pick():
    """the condition on synth.preempt_model (CPU): on the largest shape the oracle's output holds each of the seven statuses and a pick
    decided at each of the six levels of pickOneNodeForPreemption"""
    want = PC.expected(**PC.LARGEST)
    assert {c["status"] for r in want for c in r["cells"]} == set(PO.ST.values())
    assert {r["pick"][3] for r in want} >= {1, 2, 3, 4, 5, 6}


def test_lists_shape_has_the_lengths_it_is_named_for():
    lens = {len(n["pods"]) for n in PC.model(**SHAPES["lists"])["nodes"]}
    assert lens >= {0, 1, 31, 32, 33, 256}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_parity_with_oracle(gpu_required, name):
    kw = SHAPES[name]
    with Engine(0) as e:
        f = e.load_preempt_objects(PC.tables(**kw))
        e.preempt_dry_run(np.arange(kw["n_pending"]))
        PC.assert_dry_run(e, f, PC.tables(**kw), PC.expected(**kw))


def pdb_model():
    """one node whose 40 pods match 32 distinct PDBs (pod k: PDB k mod 32), pod 0 three of them; budgets -1, 0 and 1 in turn"""
    m = PC.model(n_nodes=66, n_pending=65, seed=8, node_pods=(40, 3), n_pdbs=32, scenarios=False)
    m["pdbs"][:] = [(-1, 0, 1)[k % 3] for k in range(32)]
    for k, p in enumerate(m["nodes"][0]["pods"]):
        p["pdbs"] = [0, 1, 2] if k == 0 else [k % 32]
    return m


@pytest.mark.gpu
def test_pdb_budgets_a_pod_matching_three_and_32_on_one_node(gpu_required):
    m = pdb_model()
    assert len({b for p in m["nodes"][0]["pods"] for b in p["pdbs"]}) == 32 and set(m["pdbs"]) == {-1, 0, 1}
    t = spx.objects.build_preempt_tables(spx.header(), m)
    want = PO.dry_run(m, m["pending"])
    assert any(c["n_violations"] > 0 for r in want for c in r["cells"])
    with Engine(0) as e:
        f = e.load_preempt_objects(t)
        assert f["pdb_ptr"][1] - f["pdb_ptr"][0] == 32
        e.preempt_dry_run(np.arange(len(m["pending"])))
        PC.assert_dry_run(e, f, t, want)


@pytest.mark.gpu
def test_rows_out_of_order_with_gaps_and_a_node_mask(gpu_required):
    kw = SHAPES["65x63"]
    rows = (40, 3, 62, 0, 17, 18, 5)
    mask = PC.node_mask(len(rows), kw["n_nodes"], 11)
    assert (mask == 0).any()
    with Engine(0) as e:
        f = e.load_preempt_objects(PC.tables(**kw))
        e.preempt_dry_run(rows)
        PC.assert_dry_run(e, f, PC.tables(**kw), PC.expected(rows=rows, **kw))
        e.preempt_dry_run(rows, mask)
        want = PC.expected(rows=rows, mask_seed=11, **kw)
        assert sum(c["status"] == PO.ST["SKIPPED"] for r in want for c in r["cells"]) >= int((mask == 0).sum())
        PC.assert_dry_run(e, f, PC.tables(**kw), want)


@pytest.mark.gpu
def test_reupload_makes_results_stale(gpu_required):
    kw = SHAPES["63x65"]
    t = PC.tables(**kw)
    state = spx.header().consts["SPX_ERR_STATE"]
    with Engine(0) as e:
        with pytest.raises(SpxError) as err:  # nothing uploaded
            e.preempt_dry_run([0])
        assert err.value.code == state
        f = e.load_preempt_objects(t)
        fq = e.flatten_quota(t["pods"], t["rc"], t["quota"])
        for again in (lambda: e.upload_preempt_nodes(f), lambda: e.upload_preempt_pods(fq["cols"]["pod_req"].reshape(-1, 8)), lambda: e.upload_quota(fq)):
            e.preempt_dry_run(np.arange(kw["n_pending"]))
            e.preempt_pick()
            again()
            for fetch in (e.preempt_cells, e.preempt_pick, e.preempt_keys, lambda: e.preempt_victims(0, 0)):
                with pytest.raises(SpxError) as err:
                    fetch()
                assert err.value.code == state
        e.preempt_dry_run(np.arange(kw["n_pending"]))
        PC.assert_dry_run(e, f, t, PC.expected(**kw))


@pytest.mark.gpu
@pytest.mark.parametrize("case", PC.golden()["dry_run"] + PC.golden()["post_filter"], ids=lambda c: c["name"])
def test_the_references_tables_through_the_engine(gpu_required, case):
    m = PC.golden_model(case)
    t = spx.objects.build_preempt_tables(spx.header(), m)
    want = PO.dry_run(m, m["pending"])
    assert want[0]["pick"][0] == 0  # node-a is nominated in every case
    with Engine(0) as e:
        f = e.load_preempt_objects(t)
        e.preempt_dry_run([0])
        PC.assert_dry_run(e, f, t, want)
