"""The host flatteners for nodes with 9 to 64 NUMA zones: the placeholder row and its marker in the dense table, the side table
(spx_flatten_nrt_tall_nodes: count-then-fill with exact caps, padding, assumed pods, the distance minima), the refusals, and the
dense rows of nodes with up to 8 zones, which stay byte for byte what they were.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import nrt_tall_cases as TC
from scheduler_plugins_amd import SpxError
from scheduler_plugins_amd import objects as O
from scheduler_plugins_amd import synth
from test_flatten_nrt_rows import HostOnly


def _flatten(hdr, c, strategy="LeastNUMANodes", assumed=None):
    res = O.Resources()
    pods = O.build_pod_objects(hdr, res, c["pods"])
    nrts = O.build_nrt_objects(hdr, res, c["nrts"], fresh=c["fresh"], assumed=assumed)
    nodes = O.build_node_objects(hdr, res, c["nodes"])
    e = HostOnly()
    return e, nodes, nrts, e.flatten_nrt(nodes, nrts, res.table(hdr), pods, O.nrt_params(hdr, res, strategy)), res


def _one_pod():
    return [O.pod([TC.g(1, "64Mi", {TC.DEV: "1"})])]


def test_placeholder_row_marker_and_side_table(hdr):
    """node 0: 9 zones, sparse ids, pod scope, stale; node 1: dense, 3 zones; node 2: 12 zones (so node 0 is padded to 12)"""
    ids9, ids12 = TC.ids_sparse(9), TC.ids_permuted(12)
    extras = [({TC.DEV: str(p)} if p % 3 == 0 else {}) for p in range(9)]
    nrts = [TC.tall_nrt(ids9, [str(p + 1) for p in range(9)], extras=extras, policy=TC.POD, attrs={"topologyManagerMaxNUMANodes": "16"}),
            TC.tall_nrt([0, 1, 2], ["4", "2", "1"]), TC.tall_nrt(ids12, ["2"] * 12, costs=TC.cost_rows(ids12, drop=((1, 2), (11, 0))))]
    c = TC.case(nrts, _one_pod(), fresh=[False, True, True])
    _, _, _, f, _ = _flatten(hdr, c)
    nc, tt, R = f["nodes"], f["tall"], f["R"]
    assert R == 3    # cpu, memory, the device
    HAS, FRESH, SINGLE, PODSCOPE = 1, 2, 4, 8
    assert nc["n_zones"].tolist() == [255, 3, 255]
    assert nc["flags"].tolist() == [SINGLE | PODSCOPE, HAS | FRESH | SINGLE, FRESH | SINGLE]   # a tall row: as without an NRT object
    assert nc["max_numa"].tolist() == [16, 8, 8]
    for k in (0, 2):   # every zone column of a placeholder zero; cost and distance as for a node without zones
        assert not nc["zone_id"].reshape(3, 8)[k].any() and not nc["zone_present"].reshape(3, 8)[k].any()
        assert not nc["zone_avail"].reshape(3, 8 * R)[k].any()
        assert (nc["zone_cost"].reshape(3, 64)[k] == 255).all() and (nc["min_avg_dist"].reshape(3, 8)[k] == 255.0).all()
    assert tt["n_tall"] == 2 and tt["zone_stride"] == 12 and tt["node_idx"].tolist() == [0, 2]
    assert tt["flags"].tolist() == [HAS | SINGLE | PODSCOPE, HAS | FRESH | SINGLE] and tt["max_numa"].tolist() == [16, 8]
    assert tt["n_zones"].tolist() == [9, 12] and tt["node_present"].tolist() == [7, 7]
    zid, zp = tt["zone_id"].reshape(2, 12), tt["zone_present"].reshape(2, 12)
    av, cost = tt["zone_avail"].reshape(2, 12, R), tt["zone_cost"].reshape(2, 12, 12)
    assert zid[0].tolist() == ids9 + [0, 0, 0] and zid[1].tolist() == ids12
    assert zp[0].tolist() == [7 if p % 3 == 0 else 3 for p in range(9)] + [0, 0, 0]
    assert av[0, :9, 0].tolist() == [1000 * (p + 1) for p in range(9)] and av[0, :9, 2].tolist() == [p if p % 3 == 0 else 0 for p in range(9)]
    assert not av[0, 9:].any() and (cost[0, 9:] == 255).all() and (cost[0, :, 9:] == 255).all()   # padding
    assert (np.diag(cost[0])[:9] == 10).all() and cost[0, 0, 1] == 20
    assert cost[1, 1, 2] == 255 and cost[1, 11, 0] == 255 and cost[1, 2, 1] == 20    # no Costs entry -> 255
    assert (tt["min_avg_dist"].reshape(2, 12)[0, 9:] == 255.0).all()


def test_count_then_fill_with_exact_caps(hdr):
    c = TC.case([TC.tall_nrt(TC.ids_equal(9), ["2"] * 9), TC.tall_nrt(TC.ids_equal(10), ["2"] * 10)], _one_pod())
    e, nodes, nrts, f, _ = _flatten(hdr, c)
    L, slots, R = e._lib, f["slots"], f["R"]
    n_tall, zs = C.c_int64(), C.c_int32()
    args = (nodes.ref(), nrts.ref(), slots.ref())
    assert L.spx_flatten_nrt_tall_nodes(*args, 0, 0, C.byref(n_tall), C.byref(zs), *([None] * 10)) == 0
    assert (n_tall.value, zs.value) == (2, 10)
    fn = L.spx_flatten_nrt_tall_nodes

    def fill(tall_cap, stride_cap):
        tt = dict(node_idx=np.zeros(2, np.int32), flags=np.zeros(2, np.uint8), max_numa=np.zeros(2, np.int32), node_present=np.zeros(2, np.uint8),
                  n_zones=np.zeros(2, np.uint8), zone_id=np.zeros(20, np.uint8), zone_present=np.zeros(20, np.uint8), zone_avail=np.zeros(20 * R, np.int64),
                  zone_cost=np.zeros(200, np.int32), min_avg_dist=np.zeros(20, np.float32))
        rc = fn(*args, tall_cap, stride_cap, C.byref(n_tall), C.byref(zs), *[tt[k].ctypes.data_as(t) for k, t in zip(e.TALL_COLS, fn.argtypes[7:])])
        return rc, tt

    assert fill(1, 10)[0] == -1 and fill(2, 9)[0] == -1     # a cap too small: SPX_ERR_ARG, the counts still reported
    assert (n_tall.value, zs.value) == (2, 10)
    rc, tt = fill(2, 10)                                      # the exact caps
    assert rc == 0 and tt["n_zones"].tolist() == [9, 10]
    for k in e.TALL_COLS:
        assert np.array_equal(tt[k], f["tall"][k]), k


def test_assumed_pods_are_subtracted_in_tall_zones(hdr):
    ids = TC.ids_permuted(9)
    c = TC.case([TC.tall_nrt(ids, ["2"] * 8 + ["500m"])], _one_pod())
    _, _, _, f, _ = _flatten(hdr, c, assumed={0: [{"cpu": "750m", "memory": "1Gi"}, {"cpu": "250m"}]})
    av = f["tall"]["zone_avail"].reshape(9, f["R"])
    assert av[:8, 0].tolist() == [1000] * 8 and av[8, 0] == 0     # every zone charged with every assumed pod; floor at zero
    assert av[:, 1].tolist() == [3 << 30] * 9


def _brute_min_avg(cost, nz):
    """minAvgDistanceInCombinations by enumeration, float32 as the reference: float32(sum over ordered pairs) / float32(k * k)"""
    out = np.full(nz, 255.0, np.float32)
    for k in range(1, nz + 1):
        best = None
        for comb in itertools.combinations(range(nz), k):
            ix = np.array(comb)
            s = int(cost[np.ix_(ix, ix)].sum())
            best = s if best is None or s < best else best
        d = np.float32(best) / np.float32(k * k)
        if d < out[k - 1]:
            out[k - 1] = d
    return out


@pytest.mark.parametrize("nz", [9, 12, 16])
def test_min_avg_dist_against_enumeration(hdr, nz):
    """missing cost entries and an id carried by two zones; the second node has the first one's matrix (the memoised result), the
    third another one"""
    rng = np.random.default_rng(nz)
    ids = TC.ids_permuted(nz)
    ids[3] = ids[5]                                         # a duplicate id: both zones take a Costs entry that names it
    special = {(a, b): int(rng.integers(11, 40)) for a in range(nz) for b in range(a + 1, nz)}
    drop = ((0, 2), (4, 4), (nz - 1, 1))
    rows = TC.cost_rows(ids, special=special, drop=drop)
    other = TC.cost_rows(TC.ids_equal(nz), off=31)
    nrts = [TC.tall_nrt(ids, ["2"] * nz, costs=rows), TC.tall_nrt(ids, ["3"] * nz, costs=rows), TC.tall_nrt(TC.ids_equal(nz), ["2"] * nz, costs=other)]
    _, _, _, f, _ = _flatten(hdr, TC.case(nrts, _one_pod()))
    tt = f["tall"]
    cost = tt["zone_cost"].reshape(3, nz, nz)
    assert (cost[0] == 255).any() and np.array_equal(cost[0], cost[1])
    got = tt["min_avg_dist"].reshape(3, nz)
    want0, want2 = _brute_min_avg(cost[0], nz), _brute_min_avg(cost[2], nz)
    assert np.array_equal(got[0], want0) and np.array_equal(got[2], want2)
    assert np.array_equal(got[1], got[0])                   # memoised == fresh
    assert got[2, 0] == 10.0 and not np.array_equal(got[0], got[2])


def test_min_avg_dist_unused_above_16_zones(hdr):
    _, _, _, f, _ = _flatten(hdr, TC.case([TC.tall_nrt(TC.ids_equal(17), ["2"] * 17)], _one_pod()), "LeastAllocated")
    assert (f["tall"]["min_avg_dist"] == 255.0).all() and f["tall"]["n_zones"].tolist() == [17]


def test_refusals(hdr):
    for zones, what in ((TC.ids_equal(64) + [64], "node 1 lists 65"), ([64] + list(range(9)), "node 1 lists 10")):
        c = TC.case([TC.tall_nrt([0, 1], ["2", "2"]), TC.tall_nrt(zones, ["2"] * len(zones))], _one_pod())
        with pytest.raises(SpxError) as err:
            _flatten(hdr, c)
        assert err.value.code == -1 and what in err.value.msg
    # 64 zones with ids 0..63 are taken
    _, _, _, f, _ = _flatten(hdr, TC.case([TC.tall_nrt(TC.ids_permuted(64), ["2"] * 64)], _one_pod()), "LeastAllocated")
    assert f["tall"]["n_zones"].tolist() == [64] and f["tall"]["zone_id"].tolist() == TC.ids_permuted(64)
    # a wide snapshot (more than 8 slots) with a tall node: spx_flatten_nrt_nodes_wide keeps its refusal, and the wrapper names the node
    many = {f"example.com/r{k}": "1" for k in range(8)}
    c = TC.case([TC.tall_nrt([0, 1], ["2", "2"]), TC.tall_nrt(TC.ids_equal(9), ["2"] * 9, extras=[many] * 9)], _one_pod())
    with pytest.raises(SpxError) as err:
        _flatten(hdr, c)
    assert err.value.code == -1 and "node 1 lists 9" in err.value.msg and "wide" in err.value.msg


def test_eight_zones_is_not_tall_and_its_row_is_unchanged(hdr):
    """a node of exactly 8 zones next to a tall one: its dense row, literally"""
    ids = [3, 1, 0, 2, 7, 6, 5, 4]
    special = {(0, 1): 12, (2, 3): 15}
    nrts = [TC.tall_nrt(ids, ["1", "2", "3", "4", "5", "6", "7", "8"], costs=TC.cost_rows(ids, special=special, drop=((0, 7),))),
            TC.tall_nrt(TC.ids_equal(9), ["2"] * 9)]
    _, _, _, f, _ = _flatten(hdr, TC.case(nrts, [O.pod([TC.g(1)])]))
    nc = f["nodes"]
    assert f["R"] == 2 and nc["n_zones"].tolist() == [8, 255] and nc["flags"][0] == 7 and nc["max_numa"][0] == 8 and nc["node_present"][0] == 3
    assert nc["zone_id"][:8].tolist() == ids and nc["zone_present"][:8].tolist() == [3] * 8
    assert nc["zone_avail"][:16].tolist() == [x for p in range(8) for x in (1000 * (p + 1), 4 << 30)]
    cost = nc["zone_cost"][:64].reshape(8, 8)
    want = np.full((8, 8), 20)
    np.fill_diagonal(want, 10)
    want[0, 1] = want[1, 0] = 12
    want[2, 3] = want[3, 2] = 15
    want[0, 7] = 255
    assert np.array_equal(cost, want)
    # the smallest pair sum of each subset size over its square, in float32 (the bit patterns the flattener wrote before tall nodes existed)
    sums = (10, 44, 134, 254, 424, 634, 884, 1409)
    assert nc["min_avg_dist"][:8].tolist() == [float(np.float32(s) / np.float32((k + 1) * (k + 1))) for k, s in enumerate(sums)]
    assert nc["min_avg_dist"][:8].view(np.uint32).tolist() == [1092616192, 1093664768, 1097742564, 1098776576, 1099410964, 1099752334, 1099977624, 1102061568]
    assert f["tall"]["n_tall"] == 1


def test_synth_default_has_no_tall_nodes_and_keeps_its_arrays(hdr):
    a = synth.nrt_snapshot(hdr, 400, 50, seed=9)
    b = synth.nrt_snapshot(hdr, 400, 50, seed=9, tall_frac=0.1, tall_zones=(9, 16))
    za, zb = a["nrt"].array("zone_ptr"), b["nrt"].array("zone_ptr")
    ca, cb = za[1:] - za[:-1], zb[1:] - zb[:-1]
    tall = cb > 8
    assert ca.max() <= 8 and 20 < tall.sum() < 70 and np.array_equal(ca[~tall], cb[~tall]) and cb[tall].min() >= 9 and cb[tall].max() <= 16
    e = HostOnly()
    params = O.nrt_params(hdr, O.Resources(), "LeastAllocated")
    fa = e.flatten_nrt(a["nodes"], a["nrt"], a["rc"], a["pods"], params)
    fb = e.flatten_nrt(b["nodes"], b["nrt"], b["rc"], b["pods"], params)
    assert fa["tall"]["n_tall"] == 0 and fb["tall"]["n_tall"] == tall.sum()
    for k, w in {"flags": 1, "n_zones": 1, "zone_id": 8, "zone_avail": 8 * fa["R"], "zone_cost": 64, "min_avg_dist": 8}.items():
        assert np.array_equal(fa["nodes"][k].reshape(400, w)[~tall], fb["nodes"][k].reshape(400, w)[~tall]), k
    for k in ("req_qty", "ctr_ptr"):
        assert np.array_equal(a["pods"].array(k), b["pods"].array(k))
