"""NodeResourceTopologyMatch pods with more than eight containers ("long rows") on the host side: spx_flatten_nrt_pods marks them
(n_ctr = SPX_NRT_CTRS_LONG) with their pod-level columns filled, spx_flatten_nrt_long_pods lays their containers out in CSR, and the
pod-class builder keeps every long row in a class of its own.  No device needed."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from scheduler_plugins_amd import objects as O
from scheduler_plugins_amd import synth
from test_flatten_nrt_rows import HostOnly

U8P, I32P, I64P = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def _mixed_pods(hdr, res, counts):
    """one pod per entry of `counts`: that many containers, the first three init containers (the second a sidecar), requests
    that vary by container so that the CSR order is checkable"""
    pods = []
    for p, n in enumerate(counts):
        ctrs = []
        for c in range(n):
            rl = {"cpu": f"{100 + 7 * c + p}m", "memory": f"{64 + c}Mi"}
            if c % 5 == 2:
                rl["hugepages-2Mi"] = f"{2 * (c % 3)}Mi"   # includes explicit zero-quantity requests
            if c % 7 == 3:
                rl["vendor.io/gpu"] = str(1 + c % 2)
            ctrs.append(O.container(rl, dict(rl)))
        n_init = min(3, max(0, n - 1))
        init = [dict(ctrs[i], sidecar=(i == 1)) for i in range(n_init)]
        pods.append(O.pod(ctrs[n_init:], init, overhead={"cpu": "50m"} if p % 2 else None))
    return O.build_pod_objects(hdr, res, pods)


def _flatten(hdr, res, pods):
    nodes = O.build_node_objects(hdr, res, [O.node({"cpu": "64", "memory": "256Gi", "hugepages-2Mi": "1Gi", "vendor.io/gpu": "8"})])
    nrts = O.build_nrt_objects(hdr, res, [O.nrt([{"name": "node-0", "type": "Node", "resources": {"cpu": "32", "memory": "128Gi"}}],
                                                ["SingleNUMANodeContainerLevel"])])
    return HostOnly().flatten_nrt(nodes, nrts, res.table(hdr), pods, O.nrt_params(hdr, res, "LeastAllocated"))


def _effective_request(pods, i, res_of_slot):
    """GetPodEffectiveRequest (pkg/util/resource.go:51-85) from the object tables: max over init / sidecar containers, sum over
    app containers, the larger of the two per resource, plus the overhead; keys present even with a zero quantity"""
    cp, kind = pods.array("ctr_ptr"), pods.array("ctr_kind")
    rp, rr, rq = pods.array("req_ptr"), pods.array("req_res"), pods.array("req_qty")
    init, app = {}, {}
    for c in range(cp[i], cp[i + 1]):
        for k in range(rp[c], rp[c + 1]):
            r, q = int(rr[k]), int(rq[k])
            if kind[c] == 0:
                app[r] = app.get(r, 0) + q
            elif r not in init or q > init[r]:
                init[r] = q
    out = dict(app)
    for r, q in init.items():
        if r not in out or q > out[r]:
            out[r] = q
    op, orr, oq = pods.array("ovh_ptr"), pods.array("ovh_res"), pods.array("ovh_qty")
    for k in range(op[i], op[i + 1]):
        out[int(orr[k])] = out.get(int(orr[k]), 0) + int(oq[k])
    present, req = 0, np.zeros(len(res_of_slot), np.int64)
    for s, r in enumerate(res_of_slot):
        if r in out:
            present |= 1 << s
            req[s] = out[r]
    return present, req


@pytest.mark.parametrize("counts", [[9], [3, 12, 8, 40], [200, 1, 9], [8, 8, 8]])
def test_long_rows_flatten_to_csr(hdr, counts):
    res = O.Resources()
    res.id("vendor.io/gpu")
    pods = _mixed_pods(hdr, res, counts)
    f = _flatten(hdr, res, pods)
    R = f["R"]
    slot_res = [int(x) for x in f["slots"].array("slot_res")[:R]]
    pc, lt = f["pods"], f["long"]
    assert lt is pc.long
    long_rows = [i for i, n in enumerate(counts) if n > 8]
    assert lt["n_long"] == len(long_rows) and lt["pod_row"].tolist() == long_rows
    cp, kind = pods.array("ctr_ptr"), pods.array("ctr_kind")
    rp, rr, rq = pods.array("req_ptr"), pods.array("req_res"), pods.array("req_qty")
    for i, n in enumerate(counts):
        present, req = _effective_request(pods, i, slot_res)
        assert pc["pod_present"][i] == present and np.array_equal(pc["pod_req"].reshape(len(counts), R)[i], req), i
        if n <= 8:
            assert pc["n_ctr"][i] == n
            continue
        assert pc["n_ctr"][i] == 255
        # the dense per-container columns of a long row stay zero
        assert not pc["ctr_kind"].reshape(-1, 8)[i].any() and not pc["ctr_present"].reshape(-1, 8)[i].any()
        assert not pc["ctr_req"].reshape(len(counts), 8, R)[i].any()
        k = long_rows.index(i)
        c0, c1 = int(lt["ctr_ptr"][k]), int(lt["ctr_ptr"][k + 1])
        assert c1 - c0 == n
        for j in range(n):
            c = cp[i] + j
            assert lt["ctr_kind"][c0 + j] == kind[c]
            want_p, want_q = 0, np.zeros(R, np.int64)
            for q in range(rp[c], rp[c + 1]):
                s = slot_res.index(int(rr[q]))
                want_p |= 1 << s
                want_q[s] = rq[q]
            assert lt["ctr_present"][c0 + j] == want_p, (i, j)
            assert np.array_equal(lt["ctr_req"].reshape(-1, R)[c0 + j], want_q), (i, j)
    assert lt["ctr_ptr"][0] == 0 and len(lt["ctr_kind"]) == int(lt["ctr_ptr"][-1])


def test_batch_without_long_rows_flattens_as_before(hdr):
    """a batch without long rows: the dense columns are byte for byte what the flattener wrote before long rows existed (digest
    recorded from that build), and the long table is empty"""
    want = {False: "9a55553248070e7d1810b2a9c18b01f1", True: "74d0d72e2822458ce712b70d88741584"}
    for wide, digest in want.items():
        snap = synth.nrt_snapshot(hdr, 50, 3000, seed=11, wide=wide)
        f = HostOnly().flatten_nrt(snap["nodes"], snap["nrt"], snap["rc"], snap["pods"], O.nrt_params(hdr, O.Resources(), "LeastAllocated"))
        h = hashlib.sha256()
        for k in ("qos", "non_native", "n_ctr", "ctr_kind", "ctr_present", "ctr_req", "pod_present", "pod_req"):
            h.update(k.encode())
            h.update(np.ascontiguousarray(f["pods"][k]).tobytes())
        assert h.hexdigest()[:32] == digest, wide
        assert f["long"]["n_long"] == 0 and len(f["long"]["ctr_kind"]) == 0


def test_short_rows_unchanged_by_long_rows_in_the_batch(hdr):
    """the short rows of a batch with long rows flatten exactly as the same pods without the long ones"""
    snap = synth.nrt_snapshot(hdr, 60, 1500, seed=12, long_frac=0.05)
    params = O.nrt_params(hdr, O.Resources(), "LeastAllocated")
    f = HostOnly().flatten_nrt(snap["nodes"], snap["nrt"], snap["rc"], snap["pods"], params)
    n_ctr = f["pods"]["n_ctr"]
    short = np.flatnonzero(n_ctr != 255)
    assert 30 < len(short) < 1500
    g = HostOnly().flatten_nrt(snap["nodes"], snap["nrt"], snap["rc"], synth.take_pods(hdr, snap["pods"], short), params)
    per = {"qos": 1, "non_native": 1, "n_ctr": 1, "ctr_kind": 8, "ctr_present": 8, "ctr_req": 8 * f["R"], "pod_present": 1, "pod_req": f["R"]}
    for k, w in per.items():
        assert np.array_equal(f["pods"][k].reshape(1500, w)[short], g["pods"][k].reshape(len(short), w)), k
    assert g["long"]["n_long"] == 0 and f["long"]["n_long"] == 1500 - len(short)


def test_long_table_rejects_null_columns_and_small_buffers(hdr):
    import scheduler_plugins_amd as spx
    lib = spx.lib()
    res = O.Resources()
    res.id("vendor.io/gpu")
    pods = _mixed_pods(hdr, res, [12, 3, 40])
    f = _flatten(hdr, res, pods)
    slots, R = f["slots"], f["R"]
    fn = lib.spx_flatten_nrt_long_pods
    ERR = hdr.consts["SPX_ERR_ARG"]
    nl, nc = C.c_int64(), C.c_int64()
    assert fn(pods.ref(), None, slots.ref(), 0, 0, C.byref(nl), C.byref(nc), None, None, None, None, None) == 0
    assert (nl.value, nc.value) == (2, 52)
    bufs = [np.zeros(2, np.int32), np.zeros(3, np.int32), np.zeros(52, np.uint8), np.zeros(52, np.uint8), np.zeros(52 * R, np.int64)]
    ptrs = [b.ctypes.data_as(t) for b, t in zip(bufs, (I32P, I32P, U8P, U8P, I64P))]
    assert fn(pods.ref(), None, slots.ref(), 2, 52, C.byref(nl), C.byref(nc), *ptrs) == 0
    assert bufs[0].tolist() == [0, 2] and bufs[1].tolist() == [0, 12, 52]
    for i in range(5):  # any one output column NULL while the others are given
        assert fn(pods.ref(), None, slots.ref(), 2, 52, C.byref(nl), C.byref(nc), *[None if j == i else p for j, p in enumerate(ptrs)]) == ERR, i
    assert fn(pods.ref(), None, slots.ref(), 1, 52, C.byref(nl), C.byref(nc), *ptrs) == ERR   # room for one long row only
    assert fn(pods.ref(), None, slots.ref(), 2, 51, C.byref(nl), C.byref(nc), *ptrs) == ERR   # one container short
    assert (nl.value, nc.value) == (2, 52)  # the counts come back even then
    assert fn(None, None, slots.ref(), 2, 52, C.byref(nl), C.byref(nc), *ptrs) == ERR
    assert fn(pods.ref(), None, None, 2, 52, C.byref(nl), C.byref(nc), *ptrs) == ERR
    assert fn(pods.ref(), None, slots.ref(), 2, 52, None, C.byref(nc), *ptrs) == ERR


def test_long_rows_form_classes_of_their_own(hdr):
    """pod equivalence classes (spx_internal_nrt_pod_classes): a long row's record carries its pod-level request only, so two long
    rows with equal pod-level columns would look alike; each must stay its own representative, and no row may copy one"""
    import scheduler_plugins_amd as spx
    lib = spx.lib()
    snap = synth.nrt_snapshot(hdr, 40, 300, seed=13)
    pods = synth.take_pods(hdr, snap["pods"], np.tile(np.arange(30), 10))   # ten replicas of 30 templates
    pods = synth.lengthen_pods(hdr, pods, rows=np.arange(0, 300, 7), seed=13)  # some replicas long, in a pattern crossing templates
    f = HostOnly().flatten_nrt(snap["nodes"], snap["nrt"], snap["rc"], pods, O.nrt_params(hdr, O.Resources(), "LeastAllocated"))
    from scheduler_plugins_amd.engine import Table
    t = Table(hdr, "spx_nrt_pods_soa", n_pods=300, n_res=f["R"], **f["pods"])
    rep = np.zeros(300, np.int32)
    ok = C.c_int32()
    assert lib.spx_internal_nrt_pod_classes(f["slots"].ref(), t.ref(), rep.ctypes.data_as(I32P), C.byref(ok)) == 0
    assert ok.value == 1
    is_long = f["pods"]["n_ctr"] == 255
    assert is_long.sum() == len(range(0, 300, 7))
    assert (rep[is_long] == np.flatnonzero(is_long)).all()
    assert not is_long[rep[~is_long]].any()
    assert (rep != np.arange(300)).sum() > 150   # the short replicas still collapse
