"""NetworkOverhead on snapshots whose costs need 64 bits (kernels_network_wide.hip), against the CPU oracle at tolerance 0.

The fixture is synth.network_snapshot with every NetworkTopology cost shifted left by s bits (plus cost % 7, so that the low bits are
not all zero) and every dependency's MaxNetworkCost set to (d << s) + 6: c <= d is equivalent to (c << s) + c % 7 <= (d << s) + 6,
so the Filter statuses are those of the unscaled snapshot, while the accumulated costs pass 2^31 (s = 31), 2^40 and 2^50.  Beyond
2^53 the reference's float64 NormalizeScore no longer equals exact integer division; the largest shift has such cells (counted
in the oracle's own output: a condition on the fixture).  Measured on the CPU oracle: 28 such cells at s = 40, none at s = 50, 51
and 53, 126 at s = 52 — so the third shape runs at s = 50 and at s = 52, the largest shift whose cells differ while the engine's
bound, (largest entry) x (most pairs of a workload key), stays below 2^63 (0.49 x 2^63 there)."""
import ctypes as C

import numpy as np
import pytest

from golden import network as GN
from helpers import NETOVERHEAD
from scheduler_plugins_amd import synth
from scheduler_plugins_amd import SpxError
from scheduler_plugins_amd.engine import Engine, mask_of
from test_oracle_golden_network import build

pytestmark = pytest.mark.gpu

I64P = C.POINTER(C.c_int64)
SHAPES = [(64, 40, 2, 5, 31), (1030, 129, 4, 10, 40), (257, 200, 5, 200, 50), (257, 200, 5, 200, 52)]  # (nodes, pods, seed, pods per group, shift)


def shifted(hdr, n_nodes, n_pods, seed, ppg, s):
    snap = synth.network_snapshot(hdr, n_nodes, n_pods, seed=seed, pods_per_group=ppg)
    for col in ("rc_cost", "zc_cost"):
        c = snap["nettopo"].array(col)
        c[:] = (c << s) + c % 7
    d = snap["appgroups"].array("dep_max_cost")
    d[:] = (d << s) + 6
    return snap


def load(e, snap):
    e.load_network_objects(snap["nodes"], snap["pods"], snap["appgroups"], snap["nettopo"])


def osnap_of(oracle, snap):
    return oracle.Snapshot(snap["nodes"], snap["pods"], appgroups=snap["appgroups"], nettopo=snap["nettopo"])


_want = {}


def want(hdr, oracle, shape):
    """the oracle's tables of one shape, computed once and shared: Filter statuses (and those of the unscaled snapshot), normalised
    scores, and the number of cells where float64 NormalizeScore differs from exact integer division"""
    if shape not in _want:
        n_nodes, n_pods, seed, ppg, s = shape
        snap = shifted(hdr, n_nodes, n_pods, seed, ppg, s)
        o = osnap_of(oracle, snap)
        status = o.filter_rows(NETOVERHEAD)
        raw, norm = o.score_rows(NETOVERHEAD)
        plain = synth.network_snapshot(hdr, n_nodes, n_pods, seed=seed, pods_per_group=ppg)
        status0 = osnap_of(oracle, plain).filter_rows(NETOVERHEAD)
        differs = 0
        for p in range(n_pods):
            f = status[p] == 0
            if not f.any():
                continue
            cost = [int(x) for x in raw[p][f]]
            mn, mx = min(cost), max(cost)
            if mx == mn:
                continue
            exact = np.array([100 - (100 * (c - mn)) // (mx - mn) for c in cost])
            differs += int((exact != norm[p][f]).sum())
        for a in (status, norm, status0):
            a.setflags(write=False)
        _want[shape] = dict(snap=snap, status=status, norm=norm, status0=status0, differs=differs)
    return _want[shape]


def check_tables(e, w, rows=None):
    r0, r1 = rows if rows else (0, w["status"].shape[0])
    got_st, got_sc = e.all_status(NETOVERHEAD, r0, r1), e.all_scores(NETOVERHEAD, r0, r1).astype(np.int64)
    assert np.array_equal(got_st, w["status"][r0:r1])
    bad = np.argwhere(got_sc != w["norm"][r0:r1])
    assert bad.size == 0, f"{len(bad)} mismatches, first {[(int(p), int(n), int(got_sc[p, n]), int(w['norm'][r0 + p, n])) for p, n in bad[:5]]}"


@pytest.mark.parametrize("kernel", ["class_table", "per_node"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"N{s[0]}-s{s[4]}")
def test_shifted_snapshot_equals_oracle(gpu_required, hdr, oracle, kernel, shape):
    n_nodes, n_pods = shape[0], shape[1]
    w = want(hdr, oracle, shape)
    snap = w["snap"]
    assert np.array_equal(w["status"], w["status0"])  # the shift leaves every Filter verdict where it was
    evaluated = ~(w["status"] == 255).any(axis=1) & (w["norm"].max(axis=1) > 0)
    share = (w["status"][evaluated] == 0).mean()
    assert 0.2 < share < 0.5, share
    if shape == SHAPES[-1]:
        assert w["differs"] >= 1, "fixture: no cell where float64 NormalizeScore differs from integer division"
    with Engine(0) as e:
        if kernel == "per_node":
            e.force_reference_kernels(NETOVERHEAD)
        load(e, snap)
        assert e.kernel_path(NETOVERHEAD) == 2
        e.eval(mask_of(NETOVERHEAD))
        e.sync()
        check_tables(e, w)
        for r in sorted({0, n_pods // 2, n_pods - 1}):
            sat, vio, cost = (np.zeros(n_nodes, np.int64) for _ in range(3))
            oracle.lib().orc_net_prefilter(snap["nodes"].ref(), snap["pods"].ref(), snap["appgroups"].ref(), snap["nettopo"].ref(), r,
                                           sat.ctypes.data_as(I64P), vio.ctypes.data_as(I64P), cost.ctypes.data_as(I64P))
            assert np.array_equal(e.raw(NETOVERHEAD, r, 0), cost)
            assert np.array_equal(e.raw(NETOVERHEAD, r, 1), sat)
            assert np.array_equal(e.raw(NETOVERHEAD, r, 2), vio)
        if shape == SHAPES[0]:
            assert int(max(e.raw(NETOVERHEAD, r, 0).max() for r in range(n_pods))) >= 2**31


@pytest.mark.parametrize("kernel", ["class_table", "per_node"])
@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: f"N{s[0]}-s{s[4]}")
def test_other_filter_plugin_and_row_range(gpu_required, hdr, oracle, kernel, shape):
    """a caller feasibility mask (another Filter plugin's verdict) and a row range: phase 3 walks the nodes, the minimum and maximum
    are those of the nodes that pass both"""
    n_nodes, n_pods = shape[0], shape[1]
    w = want(hdr, oracle, shape)
    rng = np.random.default_rng(shape[2])
    mask = (rng.random((n_pods, n_nodes)) < 0.7).astype(np.uint8)
    mask[n_pods // 3] = 0     # a row without a feasible node
    mask[n_pods // 3 + 1] = 1
    _, norm = osnap_of(oracle, w["snap"]).score_rows(NETOVERHEAD, mask=mask, want_raw=False)
    r0, r1 = n_pods // 4, n_pods - 3
    with Engine(0) as e:
        if kernel == "per_node":
            e.force_reference_kernels(NETOVERHEAD)
        load(e, w["snap"])
        e.upload_feasible_mask(mask)
        assert e.kernel_path(NETOVERHEAD) == 2
        e.eval(mask_of(NETOVERHEAD), r0, r1)
        e.sync()
        check_tables(e, dict(status=w["status"], norm=norm), (r0, r1))
        e.eval(mask_of(NETOVERHEAD))  # and the whole table with the mask in place
        e.sync()
        check_tables(e, dict(status=w["status"], norm=norm))


def test_one_wide_entry_is_enough(gpu_required, hdr, oracle):
    """an unscaled snapshot with a single zone-cost entry of 2^40: the object loader takes the wide tables on its own"""
    snap = synth.network_snapshot(hdr, 257, 200, seed=5, pods_per_group=200)
    snap["nettopo"].array("zc_cost")[29] = 2**40  # an entry that feasible nodes of several rows are charged (checked below, on the oracle)
    o = osnap_of(oracle, snap)
    raw, norm = o.score_rows(NETOVERHEAD)
    w = dict(status=o.filter_rows(NETOVERHEAD), norm=norm)
    rows = np.flatnonzero(((raw >= 2**40) & (w["status"] == 0)).any(axis=1))
    assert rows.size > 0, "fixture: the wide entry is not in play"
    with Engine(0) as e:
        load(e, snap)
        assert e.kernel_path(NETOVERHEAD) == 2
        e.eval(mask_of(NETOVERHEAD))
        e.sync()
        check_tables(e, w)
        r = int(rows[0])
        feasible = w["status"][r] == 0
        assert np.array_equal(e.raw(NETOVERHEAD, r, 0)[feasible], raw[r][feasible]) and int(raw[r].max()) >= 2**40


def test_narrow_snapshot_keeps_its_path_around_a_wide_upload(gpu_required, hdr, oracle):
    """a snapshot whose entries fit reports kernel_path 1 and gives the same bytes before a wide table was uploaded and after a narrow
    one replaced it; the wide table itself (unchanged values) gives those bytes through the 64-bit sweep"""
    snap = synth.network_snapshot(hdr, 1030, 129, seed=4, pods_per_group=10)
    with Engine(0) as e:
        f = e.flatten_network(snap["nodes"], snap["pods"], snap["appgroups"], snap["nettopo"])
        assert f["rcost"].dtype == np.int32 and f["zcost"].dtype == np.int32
        e.upload_network(f)
        assert e.kernel_path(NETOVERHEAD) == 1
        e.eval(mask_of(NETOVERHEAD))
        e.sync()
        st0, sc0 = e.all_status(NETOVERHEAD), e.all_scores(NETOVERHEAD)
        o = osnap_of(oracle, snap)
        assert np.array_equal(st0, o.filter_rows(NETOVERHEAD)) and np.array_equal(sc0.astype(np.int64), o.score_rows(NETOVERHEAD)[1])
        e.upload_network(dict(f, rcost=f["rcost"].astype(np.int64), zcost=f["zcost"].astype(np.int64)))
        assert e.kernel_path(NETOVERHEAD) == 2
        e.eval(mask_of(NETOVERHEAD))
        e.sync()
        assert np.array_equal(e.all_status(NETOVERHEAD), st0) and np.array_equal(e.all_scores(NETOVERHEAD), sc0)
        e.upload_network(f)
        assert e.kernel_path(NETOVERHEAD) == 1
        e.eval(mask_of(NETOVERHEAD))
        e.sync()
        assert np.array_equal(e.all_status(NETOVERHEAD), st0) and np.array_equal(e.all_scores(NETOVERHEAD), sc0)


def test_narrow_tables_are_widened_when_the_bound_asks_for_it(gpu_required, hdr, oracle):
    """entries that fit int32 but whose sum over a workload's pairs may not: uploaded through the 32-bit tables, evaluated by the 64-bit
    sweep"""
    shape = (257, 200, 5, 200)
    snap = synth.network_snapshot(hdr, *shape[:2], seed=shape[2], pods_per_group=shape[3])
    for col in ("rc_cost", "zc_cost"):
        c = snap["nettopo"].array(col)
        c[:] = (c << 23) + c % 7   # below 2^31 each
    d = snap["appgroups"].array("dep_max_cost")
    d[:] = (d << 23) + 6
    o = osnap_of(oracle, snap)
    w = dict(status=o.filter_rows(NETOVERHEAD), norm=o.score_rows(NETOVERHEAD)[1])
    with Engine(0) as e:
        f = e.flatten_network(snap["nodes"], snap["pods"], snap["appgroups"], snap["nettopo"])
        assert f["rcost"].dtype == np.int32 and int(max(f["rcost"].max(), f["zcost"].max())) < 2**31
        e.upload_network(f)
        assert e.kernel_path(NETOVERHEAD) == 2
        e.eval(mask_of(NETOVERHEAD))
        e.sync()
        check_tables(e, w)
        assert max(int(e.raw(NETOVERHEAD, r, 0).max()) for r in range(0, shape[1], 5)) >= 2**31


@pytest.mark.parametrize("case", GN.SCORE_CASES, ids=lambda c: f"L{c['line']}")
def test_score_golden_through_the_wide_tables(gpu_required, hdr, case):
    """the reference's Score / NormalizeScore table with the cost matrices uploaded as int64 (unchanged values)"""
    nodes, pods, ag, nt = build(hdr, GN.SCORE_PLACED, [(case["appgroup"], case["selector"])])
    with Engine(0) as e:
        f = e.flatten_network(nodes, pods, ag, nt)
        rg, zc = nt.struct.n_regions, nt.struct.n_zones
        rcost, zcost = np.full(max(rg * rg, 1), -1, np.int64), np.full(max(zc * zc, 1), -1, np.int64)
        e._ck(e._lib.spx_flatten_net_topo_wide(nt.ref(), rcost.ctypes.data_as(I64P), zcost.ctypes.data_as(I64P)))
        assert np.array_equal(rcost, f["rcost"]) and np.array_equal(zcost, f["zcost"])
        e.upload_network(dict(f, rcost=rcost, zcost=zcost))
        assert e.kernel_path(NETOVERHEAD) == 2
        e.eval(mask_of(NETOVERHEAD))
        e.sync()
        assert e.raw(NETOVERHEAD, 0, 0).tolist() == case["before"]
        if not e.status(NETOVERHEAD, 0).any():
            assert e.scores(NETOVERHEAD, 0).tolist() == case["after"]


def test_sequential_commit_on_a_wide_snapshot(gpu_required, hdr, oracle):
    """NetworkOverhead scheduled one pod at a time on a shifted snapshot: the cooperative kernel declines (int cost matrices in LDS),
    the per-pod graph replay runs the 64-bit sweep's single-row launch on the growing pair lists; node, weighted score, tie count and
    unschedulable verdict per pod equal the oracle's cycle"""
    n_nodes, n_pods = 300, 96
    snap = shifted(hdr, n_nodes, n_pods, 7, 12, 40)
    mask = mask_of(NETOVERHEAD)
    with Engine(0) as e:
        load(e, snap)
        assert e.kernel_path(NETOVERHEAD) == 2
        node, score, ties, _ = e.commit_sequential(mask)
        assert e.commit_path() == 2
        e.eval(mask)  # the snapshot is intact afterwards
        e.sync()
        o = osnap_of(oracle, snap)
        assert np.array_equal(e.all_status(NETOVERHEAD), o.filter_rows(NETOVERHEAD))
        assert np.array_equal(e.all_scores(NETOVERHEAD).astype(np.int64), o.score_rows(NETOVERHEAD)[1])
    want_ = oracle.commit_sequential(osnap_of(oracle, snap), mask)
    placed = want_["node"] >= 0
    assert np.array_equal(node, want_["node"]), np.flatnonzero(node != want_["node"])[:5]
    assert np.array_equal(ties, want_["ties"])
    assert np.array_equal(score[placed], want_["score"][placed])
    assert placed.any() and len(set(node[placed].tolist())) > 3


def test_bound_of_2_63_is_refused_and_the_engine_stays_usable(gpu_required, hdr, oracle):
    snap = shifted(hdr, 64, 40, 2, 5, 55)  # entries up to 95 << 55 < 2^62, 11 pairs on a workload key: the bound passes 2^63
    with Engine(0) as e:
        load(e, snap)
        with pytest.raises(SpxError) as err:
            e.eval(mask_of(NETOVERHEAD))
        assert err.value.code == -1 and "2^63" in err.value.msg and "int64 sum would wrap" in err.value.msg
        with pytest.raises(SpxError):
            e.raw(NETOVERHEAD, 0, 0)
        w = want(hdr, oracle, SHAPES[0])
        load(e, w["snap"])
        e.eval(mask_of(NETOVERHEAD))
        e.sync()
        check_tables(e, w)
