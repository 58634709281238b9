"""GPU parity (through the C ABI) for PreemptionToleration's dry run with NodeResourceTopologyMatch's single-NUMA Filter in the refit
(spx_preempt_toleration_nrt_dry_run).  Everything is integer: every cell's status, victim and violation counts and pick
keys, every pick, and the victim lists of the picked cells and of one cell per status are compared with the literal oracle
(tests/ptol_nrt_oracle.py) at tolerance 0.  Shapes: the wave / lane edges of the wave-per-node, lane-per-preemptor mapping, the words of
the 256-bit sets, 1 / 2 / 8 zones, 1 and 8 slots, 1 and 8 preemptor containers (tests/ptol_nrt_cases.py)."""
import copy

import numpy as np
import pytest

import ptol_cases as TC
import ptol_nrt_cases as NC
import ptol_nrt_oracle as NO
import ptol_oracle as TO
import scheduler_plugins_amd as spx
from scheduler_plugins_amd import SpxError
from scheduler_plugins_amd.engine import Engine
from test_oracle_ptol_nrt import without_nrt

K = spx.header().consts
ST = TO.ST
GiB = 1 << 30


def snapshot(e):
    """everything the fetches answer, as lists"""
    cells, keys, pick = e.preempt_cells(), e.preempt_keys(), e.preempt_pick()
    victims = [e.preempt_victims(i, int(n)) for i, n in enumerate(pick["node"]) if n >= 0]
    return [a.tolist() for a in (*cells, *keys, *pick.values())] + [(s, v.tolist()) for s, v in victims]


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NC.SHAPES))
def test_parity_with_oracle(gpu_required, name):
    kw = NC.SHAPES[name]
    t = NC.tables(**kw)
    with Engine(0) as e:
        f = NC.load(e, t)
        assert f["nrt"]["R"] == {"64x64": 8, "one-slot": 1}.get(name, f["nrt"]["R"])
        NC.run(e, t)
        NC.assert_dry_run(e, f, t, NC.expected(**kw))
        assert e.last_eval_ms() > 0


@pytest.mark.gpu
def test_mode_disabled_against_the_oracle_and_where_the_modes_differ(gpu_required):
    kw = NC.LARGEST
    t = NC.tables(**kw)
    on, off = NC.expected(**kw), NC.expected(mode=False, **kw)
    assert [[c["status"] for c in r["cells"]] for r in on] != [[c["status"] for c in r["cells"]] for r in off]
    with Engine(0) as e:
        f = NC.load(e, t)
        NC.run(e, t, mode=False)
        NC.assert_dry_run(e, f, t, off)
        NC.run(e, t, mode=True)
        NC.assert_dry_run(e, f, t, on)


def pdb_model():
    """test_gpu_ptol's: one node whose 40 pods match 32 distinct PDBs, budgets -1, 0 and 1 in turn; decorated"""
    m = copy.deepcopy(TC.model(n_nodes=66, n_pending=65, seed=8, node_pods=(40, 3), n_pdbs=32, scenarios=False))
    m["pdbs"][:] = [(-1, 0, 1)[k % 3] for k in range(32)]
    for k, p in enumerate(m["nodes"][0]["pods"]):
        p["pdbs"] = [0, 1, 2] if k == 0 else [k % 32]
    return NC.decorate(m, 8, zones=(2, 8), max_ctrs=3)


@pytest.mark.gpu
def test_32_pdbs_on_one_node(gpu_required):
    m = pdb_model()
    t = NC.build_tables(m)
    want = NO.dry_run(m, m["pending"])
    assert any(c["n_violations"] > 0 for r in want for c in r["cells"])
    with Engine(0) as e:
        f = NC.load(e, t)
        assert f["pdb_ptr"][1] - f["pdb_ptr"][0] == 32
        NC.run(e, t)
        NC.assert_dry_run(e, f, t, want)


@pytest.mark.gpu
def test_rows_out_of_order_with_gaps_and_a_node_mask(gpu_required):
    kw = NC.SHAPES["63x65"]
    rows = (40, 3, 62, 0, 17, 18, 5)
    mask = NC.node_mask(len(rows), kw["n_nodes"], 11)
    assert (mask == 0).any()
    t = NC.tables(**kw)
    with Engine(0) as e:
        f = NC.load(e, t)
        NC.run(e, t, rows)
        NC.assert_dry_run(e, f, t, NC.expected(rows=rows, **kw))
        NC.run(e, t, rows, mask)
        want = NC.expected(rows=rows, mask_seed=11, **kw)
        assert sum(c["status"] == ST["SKIPPED"] for r in want for c in r["cells"]) >= int((mask == 0).sum())
        NC.assert_dry_run(e, f, t, want)


# ---------------------------------------------------------------------------------------------------------------- the three directions
def pod(key, prio, cpu, qos, start=1000, row=-1):
    """a one-container pod of `cpu` millicores and 1 GiB"""
    req = {"v": [cpu, GiB, 0, 0, 0, 0, 0, 0], "p": 0}
    r = {"cpu": cpu, "memory": GiB}
    return {"key": key, "ns": 0, "prio": prio, "start": start, "fit": [cpu, GiB, 0, 1, 0, 0, 0, 0], "req": req, "pdbs": [], "terminating": False, "row": row,
            "pc": "", "scheduled_at": None, "never": False, "init_containers": [],
            "containers": [{"name": "c0", "requests": r, "limits": dict(r) if qos == NO.GUARANTEED else {}}]}


def one_node(node_cpu, zone_cpu_avail, pods, placement, preemptor_cpu):
    """one node of two NUMA zones with 4 cpus and 64 GiB each (container scope), and one Guaranteed preemptor of priority 100"""
    zones = [{"name": f"node-{z}", "resources": [("cpu", 4000, a), ("memory", 64 * GiB, 32 * GiB)]} for z, a in enumerate(zone_cpu_avail)]
    node = {"present": True, "alloc": [node_cpu, 128 * GiB, 0, 110, 0, 0, 0, 0], "pods": pods, "nominated": [], "alloc_names": {"cpu", "memory", "ephemeral-storage", "pods"},
            "nrt": {"zones": zones, "policy": "single-numa-node", "scope": "container"}, "nrt_fresh": True, "placement": placement}
    return {"n_namespaces": 1, "quotas": {}, "pdbs": [], "nodes": [node], "pending": [pod("p", 100, preemptor_cpu, NO.GUARANTEED, row=0)], "classes": {}, "now": TC.GOLDEN_NOW}


DIRECTIONS = {
    # the node's totals (10 cpus) take the preemptor next to both pods, but only zone 0, once v1 is gone, has 4 whole cpus: NodeResourcesFit
    # alone reprieves everybody, the Filter keeps v1
    "kept-victim": (one_node(10000, [0, 3000], [pod("v1", 10, 4000, NO.GUARANTEED), pod("v2", 20, 1000, NO.GUARANTEED)], {("v1", "c0"): 0, ("v2", "c0"): 1}, 4000),
                    (ST["CANDIDATE"], [0]), (ST["ALL_REPRIEVED"], [])),
    # with v gone the totals take 6 cpus, no zone of 4 does
    "fits-by-totals-only": (one_node(8000, [0, 4000], [pod("v", 10, 4000, NO.GUARANTEED)], {("v", "c0"): 0}, 6000), (ST["NOT_FIT"], []), (ST["CANDIDATE"], [0])),
    # every potential victim is Burstable: the simulation has nothing to add and the Filter answers Unschedulable, on zones that would fit
    "all-burstable": (one_node(4000, [4000, 4000], [pod("v", 10, 3000, NO.BURSTABLE)], {("v", "c0"): 0}, 2000), (ST["NOT_FIT"], []), (ST["CANDIDATE"], [0])),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DIRECTIONS))
def test_the_filter_changes_the_outcome(gpu_required, name):
    m, with_filter, fit_only = DIRECTIONS[name]
    want = NO.dry_run(m, m["pending"])
    assert (want[0]["cells"][0]["status"], want[0]["cells"][0]["victims"]) == with_filter
    plain = TO.dry_run(m, m["pending"])
    assert (plain[0]["cells"][0]["status"], plain[0]["cells"][0]["victims"]) == fit_only
    t = NC.build_tables(m)
    with Engine(0) as e:
        f = NC.load(e, t)
        NC.run(e, t)
        NC.assert_dry_run(e, f, t, want)
        got = e.preempt_victims(0, 0)
        assert (got[0], got[1].tolist()) == with_filter
        TC.run(e, t)  # spx_preempt_toleration_dry_run on the same upload gives the other answer
        TC.assert_dry_run(e, f, t, plain)
        got = e.preempt_victims(0, 0)
        assert (got[0], got[1].tolist()) == fit_only


# ---------------------------------------------------------------------------------------------------------------- next to the old dry run
@pytest.mark.gpu
def test_without_any_nrt_it_is_the_old_dry_run_byte_for_byte(gpu_required):
    m = without_nrt(NC.model(**NC.SHAPES["65x63"]))
    t = NC.build_tables(m)
    with Engine(0) as e:
        f = NC.load(e, t)
        assert not (f["nrt"]["node_flags"] & K["SPX_NRT_F_HAS_NRT"]).any()
        TC.run(e, t)
        old = snapshot(e)
        TC.assert_dry_run(e, f, t, TO.dry_run(m, m["pending"]))
        for mode in (True, False):
            NC.run(e, t, mode=mode)
            assert snapshot(e) == old


@pytest.mark.gpu
def test_the_old_dry_run_is_the_same_before_and_after_the_upload(gpu_required):
    kw = NC.SHAPES["63x65"]
    t = NC.tables(**kw)
    with Engine(0) as e:
        f = e.load_preempt_toleration_objects(t)
        TC.run(e, t)
        before = snapshot(e)
        e.upload_preempt_nrt(NC.flatten_nrt(e, t, f))
        with pytest.raises(SpxError):
            e.preempt_cells()  # an upload marks results stale
        TC.run(e, t)
        assert snapshot(e) == before
        NC.run(e, t)
        assert snapshot(e) != before
        TC.run(e, t)
        assert snapshot(e) == before


# ---------------------------------------------------------------------------------------------------------------- state
def raises(code, fn):
    with pytest.raises(SpxError) as err:
        fn()
    assert err.value.code == code, err.value
    return err.value.msg


@pytest.mark.gpu
def test_refusals_and_staleness(gpu_required):
    kw = NC.SHAPES["63x65"]
    t = NC.tables(**kw)
    STATE, ARG = K["SPX_ERR_STATE"], K["SPX_ERR_ARG"]
    fetches = lambda e: (e.preempt_cells, e.preempt_pick, e.preempt_keys, lambda: e.preempt_victims(0, 0))
    with Engine(0) as e:
        g = NC.flatten_nrt(e, t, e.flatten_preempt_nodes(t["nodes"], t["rc"], t["quota"], t["preempt"]))
        raises(STATE, lambda: e.upload_preempt_nrt(g))  # before spx_upload_preempt_nodes / _pods
        f = e.load_preempt_toleration_objects(t)
        raises(STATE, lambda: NC.run(e, t))  # no side table yet
        e.upload_preempt_nrt(g)
        # sizes that are not the tables'
        cut = dict(g, pod_contributes=g["pod_contributes"][:-1], rel_ptr=g["rel_ptr"][:-1])
        assert "pods" in raises(ARG, lambda: e.upload_preempt_nrt(cut))
        fewer = dict(g, pods=type(g["pods"])({k: v[:len(v) // len(g["pods"]["qos"]) * (len(g["pods"]["qos"]) - 1)] for k, v in g["pods"].items()}))
        assert "pod rows" in raises(ARG, lambda: e.upload_preempt_nrt(fewer))
        fewer_nodes = dict(g, N=g["N"] - 1)
        assert "nodes" in raises(ARG, lambda: e.upload_preempt_nrt(fewer_nodes))
        # the limits, named
        n = int(np.flatnonzero(g["n_zones"])[0])
        room = g["zone_headroom"].copy()
        room[n, 0, 0] = -1
        assert f"node {n}" in raises(ARG, lambda: e.upload_preempt_nrt(dict(g, zone_headroom=room)))
        j = int(np.flatnonzero(np.diff(g["rel_ptr"]))[0])
        qty = g["rel_qty"].copy()
        qty[g["rel_ptr"][j]] = -1
        assert f"assigned pod {j}" in raises(ARG, lambda: e.upload_preempt_nrt(dict(g, rel_qty=qty)))
        # two releases of one node in one slot that sum to 2^62
        node_of = np.searchsorted(f["pod_ptr"], np.repeat(np.arange(len(g["pod_contributes"])), np.diff(g["rel_ptr"])), side="right") - 1
        seen = {}
        for k, (n2, s2) in enumerate(zip(node_of.tolist(), g["rel_slot"].tolist())):
            if (n2, s2) in seen:
                break
            seen[(n2, s2)] = k
        qty = g["rel_qty"].copy()
        qty[[seen[(n2, s2)], k]] = 1 << 61
        assert f"node {n2}" in raises(ARG, lambda: e.upload_preempt_nrt(dict(g, rel_qty=qty)))
        NC.run(e, t)  # a refused upload leaves the table of the last good one in place
        e.upload_preempt_nrt(g)
        raises(ARG, lambda: NC.run(e, t, now=(1 << 63) - 1))
        raises(ARG, lambda: e.preempt_toleration_nrt_dry_run([len(t["priority"])], [5], [0], t["now"]))  # no row of the batch
        for again in (lambda: e.upload_preempt_nrt(g), lambda: e.upload_preempt_toleration(f["toleration"])):
            NC.run(e, t)
            e.preempt_pick()
            again()
            for fetch in fetches(e):
                raises(STATE, fetch)
        NC.run(e, t)
        e.upload_preempt_nodes(f)  # drops the side table with the toleration table
        for fetch in fetches(e):
            raises(STATE, fetch)
        e.upload_preempt_toleration(f["toleration"])
        assert "spx_upload_preempt_nrt" in raises(STATE, lambda: NC.run(e, t))
        TC.run(e, t)  # the old dry run needs no side table
        e.upload_preempt_nrt(g)
        NC.run(e, t)
        NC.assert_dry_run(e, f, t, NC.expected(**kw))


# ---------------------------------------------------------------------------------------------------------------- zones that share a NUMA id
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NC.TWIN_MODELS))
def test_twin_zones_and_the_accounting_error(gpu_required, name):
    """nodes that list one NUMA id twice: the charge and the release land on both twins, and a twin charged below zero is the Filter's
    fwk.Error — no candidate, no reprieve (tests/test_nrt_refit_twins_host.py shows the models hold that edge)"""
    m = NC.twin_models()[name]
    trace = set()
    want = NO.dry_run(m, m["pending"], trace=trace)
    assert "accounting-error" in trace
    t = NC.build_tables(m)
    with Engine(0) as e:
        f = NC.load(e, t)
        NC.run(e, t)
        NC.assert_dry_run(e, f, t, want)
