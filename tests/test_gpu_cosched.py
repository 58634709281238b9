"""GPU parity (through the C ABI) for Coscheduling's PreFilter gate (pkg/coscheduling/core/core.go:243-305, :406-467).  Everything is
integer: every status byte, every per-slot pass / open bit and every gap is compared with the literal oracle (tests/cosched_oracle.py)
at tolerance 0.  The shapes are the smallest that reach each code path of kernels_cosched.hip: a single node, a wave edge, a
workgroup-chunk edge with its carry, several chunks with step lists shorter and longer than a wave and than an LDS tile of steps."""
import functools

import numpy as np
import pytest

import cosched_cases as CC
import cosched_oracle as CO
import scheduler_plugins_amd as spx
from scheduler_plugins_amd import SpxError, synth
from scheduler_plugins_amd.engine import ALLOCATABLE, COSCHED, TLP, Engine, mask_of

pytestmark = pytest.mark.gpu

# name -> draws of cosched_cases.draw_snapshot.  With 3 groups one draw cannot hold four failing statuses: the single-node shape is
# two draws, and the five statuses are asserted over both.
SHAPES = {
    "1x3": [dict(seed=1, n_nodes=1, n_groups=3, n_walk=1, kinds=[0, 1, 2], edges=[3]), dict(seed=2, n_nodes=1, n_groups=3, n_walk=2, kinds=[3, 0, 6], edges=[5, 2, 3])],
    "63": [dict(seed=3, n_nodes=63, n_groups=23, n_walk=9, first_absent=True)],
    "64": [dict(seed=4, n_nodes=64, n_groups=23, n_walk=9, last_absent=False)],
    "65": [dict(seed=5, n_nodes=65, n_groups=23, n_walk=9, last_absent=True)],
    "1023": [dict(seed=6, n_nodes=1023, n_groups=40, n_walk=20)],
    "1025": [dict(seed=7, n_nodes=1025, n_groups=40, n_walk=20, last_absent=False)],
    "2500": [dict(seed=8, n_nodes=2500, n_groups=300, n_walk=60, step_lens=[70, 2, 1, 300], first_absent=False, last_absent=False)],
}


@functools.lru_cache(maxsize=None)
def case(name, i):
    """(snapshot, flattened columns, oracle status, oracle verdicts) of one draw, computed once for every test that needs it"""
    hdr = spx.header()
    snap = CC.draw_snapshot(**SHAPES[name][i])
    res, nodes, objects = CC.build(hdr, snap)
    with Engine(0) as e:
        f = e.flatten_cosched(nodes, objects)
    status, verdicts = CC.expected(snap, res, f["slot_res"])
    verdicts = verdicts + [(0, 0, {})] * (f["G"] - len(verdicts))  # labels without a PodGroup object: no request
    return snap, f, status, verdicts


def assert_gate(e, f, status, verdicts):
    got = e.prefilter(COSCHED)
    bad = np.flatnonzero(got != status)
    assert bad.size == 0, f"{bad.size} status bytes differ, first {[(int(p), int(got[p]), int(status[p])) for p in bad[:5]]}"
    pm, om, gap = e.cosched_gap()
    want_gap = np.zeros_like(gap)
    for g, (_, _, gaps) in enumerate(verdicts):
        for s, v in gaps.items():
            want_gap[g, s] = v
    assert pm.tolist() == [v[0] for v in verdicts]
    assert om.tolist() == [v[1] for v in verdicts]
    assert np.array_equal(gap, want_gap), np.argwhere(gap != want_gap)[:5]


@pytest.mark.parametrize("name", list(SHAPES))
def test_parity_with_oracle(gpu_required, name):
    seen = set()
    for i in range(len(SHAPES[name])):
        snap, f, status, verdicts = case(name, i)
        seen |= set(status.tolist())
        assert f["S"] == 4 and (f["left_base"] < 0).any()  # slots {cpu, memory, pods, one scalar}; over-requested nodes
        assert not f["node_present"].all() or f["N"] == 1
        n_walk = int((np.diff(f["step_ptr"]) > 0).sum())
        assert n_walk > 0 and (name == "1x3" or n_walk < f["G"])
        with Engine(0) as e:
            e.upload_cosched(f)
            e.eval(mask_of(COSCHED))
            e.sync()
            assert e.kernel_path(COSCHED) == n_walk
            assert_gate(e, f, status, verdicts)
    assert seen == {CO.SUCCESS, CO.BACKED_OFF, CO.FEW_SIBLINGS, CO.GATED, CO.RESOURCE_GAP}, seen  # no case is vacuous


def test_large_shape_reaches_every_step_list_path(gpu_required):
    snap, f, status, verdicts = case("2500", 0)
    lens = np.diff(f["step_ptr"])
    assert {1, 2, 70, 300} <= set(lens.tolist())  # one step, two, longer than a wave, longer than an LDS tile of steps (128)
    assert f["step_node"][f["step_ptr"][0]] == 0 and f["step_node"][f["step_ptr"][2] - 1] == f["N"] - 1  # steps on node 0 and on the last node
    assert f["N"] > 9 * 256  # several chunks of the scan
    passes_with_steps = [g for g in range(f["G"]) if lens[g] > 0 and verdicts[g][1] == 0 and verdicts[g][0]]
    assert passes_with_steps and any(v[1] for g, v in enumerate(verdicts) if lens[g] > 0)  # walks that close and walks that stay open


def test_partial_rows(gpu_required):
    snap, f, status, verdicts = case("1023", 0)
    with Engine(0) as e:
        e.upload_cosched(f)
        e.eval(mask_of(COSCHED), 5, 40)
        assert np.array_equal(e.prefilter(COSCHED, 5, 40), status[5:40])
        with pytest.raises(SpxError):
            e.prefilter(COSCHED, 0, 40)
        e.eval(mask_of(COSCHED), 40, f["P"])
        assert np.array_equal(e.prefilter(COSCHED, 5, f["P"]), status[5:])


def test_reupload_with_one_permitted_flag_flipped(gpu_required):
    snap, f, status, verdicts = case("1025", 0)
    # a group whose pods are turned away by the resource check alone
    g = next(g for g in range(f["G"]) if verdicts[g][1] and (status[f["pod_group"] == g] == CO.RESOURCE_GAP).all() and (f["pod_group"] == g).any())
    with Engine(0) as e:
        e.upload_cosched(f)
        e.eval(mask_of(COSCHED))
        before = e.prefilter(COSCHED)
        flipped = dict(f, permitted=f["permitted"].copy())
        flipped["permitted"][g] = 1
        e.upload_cosched(flipped)
        with pytest.raises(SpxError):  # the gate is stale after any upload
            e.prefilter(COSCHED)
        e.eval(mask_of(COSCHED))
        after = e.prefilter(COSCHED)
        pm, om, gap = e.cosched_gap()
    assert np.array_equal(before, status)
    changed = np.flatnonzero(before != after)
    assert changed.tolist() == np.flatnonzero(f["pod_group"] == g).tolist() and (after[changed] == 0).all()
    assert om.tolist() == [v[1] for v in verdicts]  # the verdicts themselves do not depend on permittedPG


def test_best_reports_gated_pods_unschedulable(gpu_required, hdr):
    N, P = 257, 200
    tri = synth.trimaran_snapshot(hdr, N, P, seed=21, round_frac=0.3)
    snap = CC.draw_snapshot(seed=9, n_nodes=N, n_groups=60, n_walk=15, n_pending=P)
    res, nodes, objects = CC.build(hdr, snap)
    AT = mask_of(ALLOCATABLE, TLP)
    with Engine(0) as e:
        e.load_trimaran_objects(tri["nodes"], tri["rc"], tri["pods"], tri["metrics"], tri["assigned"])
        f = e.flatten_cosched(nodes, objects)
        status, _ = CC.expected(snap, res, f["slot_res"])
        failed = status != 0
        assert failed.any() and not failed.all() and set(status.tolist()) == {0, 1, 2, 3, 4}
        e.upload_cosched(f)
        e.eval(AT)
        e.eval_best(AT)
        plain = [x.copy() for x in e.best()]
        e.decide(AT)
        plain_decide = [x.copy() for x in e.best()]
        e.eval(AT | mask_of(COSCHED))
        e.eval_best(AT | mask_of(COSCHED))
        gated = [x.copy() for x in e.best()]
        assert np.array_equal(e.prefilter(COSCHED), status)
        e.decide(AT | mask_of(COSCHED))
        gated_decide = [x.copy() for x in e.best()]
    for without, with_gate in ((plain, gated), (plain_decide, gated_decide)):
        node, score, ties, feasible = with_gate
        assert (node[failed] == -1).all() and (feasible[failed] == 0).all() and (score[failed] == 0).all() and (ties[failed] == 0).all()
        for w, g in zip(without, with_gate):
            assert np.array_equal(w[~failed], g[~failed])
        assert (without[0] >= 0).all()  # the gate is the only reason for a pod to come back without a node


def test_commit_sequential_refuses_the_gate(gpu_required, hdr):
    tri = synth.trimaran_snapshot(hdr, 64, 16, seed=22)
    with Engine(0) as e:
        e.load_trimaran_objects(tri["nodes"], tri["rc"], tri["pods"], tri["metrics"], tri["assigned"])
        with pytest.raises(SpxError) as err:
            e.commit_sequential(mask_of(ALLOCATABLE, TLP, COSCHED))
        assert err.value.code == spx.header().consts["SPX_ERR_ARG"] and "Coscheduling" in str(err.value)


def test_upload_refuses_sums_beyond_int64(gpu_required):
    snap, f, status, verdicts = case("63", 0)
    big = dict(f, left_base=f["left_base"].copy())
    big["left_base"][1, :2] = (1 << 61)  # slot 1 (memory): two nodes of 2^61 reach 2^62
    with Engine(0) as e:
        with pytest.raises(SpxError) as err:
            e.upload_cosched(big)
        assert err.value.code == spx.header().consts["SPX_ERR_ARG"] and "slot 1" in str(err.value)
        e.upload_cosched(f)
        e.eval(mask_of(COSCHED))
        assert_gate(e, f, status, verdicts)
