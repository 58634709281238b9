"""NodeResourceTopologyMatch's wide tables on the host side (more than eight resource slots): the slot numbering of
spx_flatten_nrt_slots_wide, the dense flattener's unchanged refusal, and the wide node and pod tables against a restatement built from
the object tables.  No device needed."""
import ctypes as C

import numpy as np
import pytest

from scheduler_plugins_amd import objects as O
from scheduler_plugins_amd import synth
from scheduler_plugins_amd.engine import wide_rows_slice
from test_flatten_nrt_long import _effective_request
from test_flatten_nrt_rows import HostOnly

U8P, I32P, I64P = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
AFFINE, HOST_LEVEL, CPU = 1, 2, 4
FIXED_NATIVE = (0, 1, 2, 3, 4)


def _params(hdr):
    return O.nrt_params(hdr, O.Resources(), "LeastAllocated")


def _rc_flags(rc):
    return rc.array("flags")


def _native(rcf, r):
    return r in FIXED_NATIVE or (r < len(rcf) and bool(rcf[r] & 2))


def _expected_slots(s):
    ids = set(s["pods"].array("req_res").tolist()) | set(s["pods"].array("ovh_res").tolist()) | set(s["nrt"].array("zres_res").tolist())
    rcf = _rc_flags(s["rc"])
    out = []
    for r in sorted(ids):
        f = 0
        if r in (0, 1) or (r >= 5 and r < len(rcf) and rcf[r] & 1):
            f |= AFFINE
        if r in (2, 4) or not _native(rcf, r):
            f |= HOST_LEVEL
        if r == 0:
            f |= CPU
        out.append((r, f))
    return out


@pytest.mark.parametrize("extra,n_res", [(5, 9), (8, 12), (28, 32)])
def test_slot_numbering_wide(hdr, extra, n_res):
    s = synth.nrt_snapshot(hdr, 80, 300, seed=11, extra_res=extra)
    R, st, slot_res, slot_flags, slot_weight = HostOnly().nrt_slots_wide(s["nrt"], s["rc"], s["pods"], _params(hdr))
    assert st == 0 and R == n_res
    want = _expected_slots(s)
    assert [(int(slot_res[i]), int(slot_flags[i])) for i in range(R)] == want
    assert (slot_weight[:R] == 1).all()
    assert (slot_res[R:] == 0).all()


def test_slot_weights_beyond_slot_eight(hdr):
    res = O.Resources()
    names = [f"example.com/pool{k}" for k in range(9)]
    pods = O.build_pod_objects(hdr, res, [O.pod([O.container({n: "1" for n in names}, {n: "1" for n in names})])])
    nrts = O.build_nrt_objects(hdr, res, [O.nrt([{"name": "node-0", "type": "Node", "resources": {"cpu": "4", "memory": "4Gi"}}])])
    params = O.nrt_params(hdr, res, "LeastAllocated", weights={names[8]: 7, names[0]: 0, "cpu": 3})
    R, st, slot_res, _, slot_weight = HostOnly().nrt_slots_wide(nrts, res.table(hdr), pods, params)
    assert st == 0 and R == 11
    w = dict(zip(slot_res[:R].tolist(), slot_weight[:R].tolist()))
    assert w[res.id(names[8])] == 7 and w[res.id(names[0])] == 1 and w[res.id("cpu")] == 3 and w[res.id("memory")] == 1


def test_thirty_three_slots_refused(hdr):
    s = synth.nrt_snapshot(hdr, 50, 200, seed=12, extra_res=29)
    R, st, slot_res, _, _ = HostOnly().nrt_slots_wide(s["nrt"], s["rc"], s["pods"], _params(hdr))
    assert st == -1 and R == 33
    R, st, _, _, _ = HostOnly().nrt_slots_wide(s["nrt"], s["rc"], s["pods"], _params(hdr), cap=33)
    assert st == -1  # (cap above SPX_NRT_MAX_RES_WIDE)


def test_dense_slot_flatten_still_refuses_nine(hdr):
    """spx_flatten_nrt_slots: SPX_ERR_ARG beyond 8 slots, nothing written past entry 8 (callers size its arrays by SPX_NRT_MAX_RES)"""
    s = synth.nrt_snapshot(hdr, 50, 200, seed=13, extra_res=5)
    e = HostOnly()
    n_res = C.c_int32(-7)
    sr, sf, sw = np.full(16, -5, np.int32), np.full(16, 99, np.uint8), np.full(16, -9, np.int64)
    rc = e._lib.spx_flatten_nrt_slots(s["pods"].ref(), s["nrt"].ref(), s["rc"].ref(), _params(hdr).ref(), C.byref(n_res),
                                      sr.ctypes.data_as(I32P), sf.ctypes.data_as(U8P), sw.ctypes.data_as(I64P))
    assert rc == -1 and n_res.value == -7
    assert (sr[8:] == -5).all() and (sf[8:] == 99).all() and (sw[8:] == -9).all()
    # the Python flatten takes the wide form by itself
    f = e.flatten_nrt(s["nodes"], s["nrt"], s["rc"], s["pods"], _params(hdr))
    assert f["wide"] and f["R"] == 9


@pytest.fixture(scope="module")
def wide_flat(hdr):
    s = synth.nrt_snapshot(hdr, 120, 400, seed=14, extra_res=20, extra_req_frac=0.5, long_frac=0.05, long_ctrs=(9, 14))
    return s, HostOnly().flatten_nrt(s["nodes"], s["nrt"], s["rc"], s["pods"], _params(hdr))


def test_wide_node_table_restated(hdr, wide_flat):
    """presence masks with bits 8..31, node-level keys, zone quantities less the assumed pods (OverReserve)"""
    s, f = wide_flat
    assert f["wide"] and f["R"] == 24
    R = f["R"]
    slot_of = {int(r): i for i, r in enumerate(f["slots"].array("slot_res")[:R])}
    nodes, nrt, nc = s["nodes"], s["nrt"], f["nodes"]
    sp, sr = nodes.array("scalar_ptr"), nodes.array("scalar_res")
    zp_, isn, zid = nrt.array("zone_ptr"), nrt.array("zone_is_node"), nrt.array("zone_numa_id")
    rp, rr, ra = nrt.array("zres_ptr"), nrt.array("zres_res"), nrt.array("zres_avail")
    ap, alp, alr, alq = nrt.array("assumed_ptr"), nrt.array("arl_ptr"), nrt.array("arl_res"), nrt.array("arl_qty")
    has = nrt.array("has_nrt")
    high_bits = 0
    n_assumed = 0
    for i in range(int(nodes.struct.n_nodes)):
        keys = {0, 1, 2, 3} | set(sr[sp[i]:sp[i + 1]].tolist())
        assert int(nc["node_present"][i]) == sum(1 << s_ for r, s_ in slot_of.items() if r in keys), i
        zones = [z for z in range(zp_[i], zp_[i + 1]) if isn[z] and 0 <= zid[z] <= 63] if has[i] else []
        assert nc["n_zones"][i] == len(zones)
        n_assumed += ap[i + 1] - ap[i]
        for pos, z in enumerate(zones):
            assert nc["zone_id"][i * 8 + pos] == zid[z]
            present, avail = 0, np.zeros(R, np.int64)
            for k in range(rp[z], rp[z + 1]):
                s_ = slot_of[int(rr[k])]
                q = int(ra[k])
                for a in range(ap[i], ap[i + 1]):
                    for m in range(alp[a], alp[a + 1]):
                        if alr[m] == rr[k]:
                            q = 0 if q < alq[m] else q - int(alq[m])
                present |= 1 << s_
                avail[s_] = q
            assert int(nc["zone_present"][i * 8 + pos]) == present, (i, pos)
            assert np.array_equal(nc["zone_avail"][(i * 8 + pos) * R:(i * 8 + pos + 1) * R], avail), (i, pos)
            high_bits |= present >> 8
    assert nc["zone_present"].dtype == np.uint32 and nc["node_present"].dtype == np.uint32
    assert high_bits >> 15 and n_assumed > 0  # presence beyond bit 23 and OverReserve exercised


def test_wide_pod_table_restated(hdr, wide_flat):
    """CSR lists in ascending slot order, zero quantities kept; the pod-level list is GetPodEffectiveRequest with init / sidecar
    containers and overhead"""
    s, f = wide_flat
    R = f["R"]
    res_of_slot = [int(r) for r in f["slots"].array("slot_res")[:R]]
    slot_of = {r: i for i, r in enumerate(res_of_slot)}
    pods, pw = s["pods"], f["pods"]
    cp, kind = pods.array("ctr_ptr"), pods.array("ctr_kind")
    rp, rr, rq = pods.array("req_ptr"), pods.array("req_res"), pods.array("req_qty")
    rcf = _rc_flags(s["rc"])
    assert np.array_equal(pw["ctr_ptr"], cp) and np.array_equal(pw["ctr_kind"], kind)
    seen = dict(zero=0, high=0, init=0, ovh=0, long=0)
    for i in range(int(pods.struct.n_pods)):
        nn = False
        for c in range(cp[i], cp[i + 1]):
            want = {}
            for k in range(rp[c], rp[c + 1]):
                want[slot_of[int(rr[k])]] = int(rq[k])
                nn |= not _native(rcf, int(rr[k]))
            lst = sorted(want.items())
            e0, e1 = pw["ent_ptr"][c], pw["ent_ptr"][c + 1]
            assert pw["ent_slot"][e0:e1].tolist() == [x for x, _ in lst] and pw["ent_qty"][e0:e1].tolist() == [q for _, q in lst], (i, c)
            seen["zero"] += sum(q == 0 for _, q in lst)
            seen["high"] += sum(x >= 8 for x, _ in lst)
            seen["init"] += kind[c] != 0
        assert pw["non_native"][i] == nn
        present, req = _effective_request(pods, i, res_of_slot)
        slots = [x for x in range(R) if (present >> x) & 1]
        r0, r1 = pw["req_ptr"][i], pw["req_ptr"][i + 1]
        assert pw["req_slot"][r0:r1].tolist() == slots and pw["req_qty"][r0:r1].tolist() == [int(req[x]) for x in slots], i
        seen["long"] += cp[i + 1] - cp[i] > 8
    seen["ovh"] = int(pods.array("ovh_ptr")[-1])
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("rows", [(0, 400), (0, 1), (137, 263), (399, 400), (50, 50)])
def test_wide_pod_table_row_slice(hdr, wide_flat, rows):
    """a MultiEngine shard's slice equals the flatten of that shard's pods alone"""
    s, f = wide_flat
    got = wide_rows_slice(f["pods"], rows)
    want = HostOnly().flatten_nrt_pods_wide(synth.take_pods(hdr, s["pods"], np.arange(*rows)), s["rc"], f["slots"])
    for k in want:
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("rows", [(0, 200), (200, 400), (57, 331)])
def test_wide_pod_table_of_a_view(hdr, wide_flat, rows):
    """a pod table that is a view into a larger one (MultiEngine's per-rank pods: container offsets not starting at 0) flattens to
    lists starting at 0, equal to the slice of the whole table"""
    from scheduler_plugins_amd.multi import pod_rows
    s, f = wide_flat
    got = HostOnly().flatten_nrt_pods_wide(pod_rows(hdr, s["pods"], *rows), s["rc"], f["slots"])
    want = wide_rows_slice(f["pods"], rows)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
