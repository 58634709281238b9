"""The NRT side table of the preemption tables, host side (no GPU): spx_flatten_preempt_nrt's additivity claim against the product's
eviction simulation (spx_nrt_post_eviction, itself pinned to the reference's table by tests/test_nrt_preemption.py), and the refusals."""
import copy
import ctypes as C

import numpy as np
import pytest

import ptol_nrt_cases as NC
import ptol_nrt_oracle as NO
import scheduler_plugins_amd as spx
from scheduler_plugins_amd import SpxError, objects
from scheduler_plugins_amd.engine import Engine

HDR = spx.header()
K = HDR.consts
QOS = {NO.GUARANTEED: K["SPX_QOS_GUARANTEED"], NO.BURSTABLE: K["SPX_QOS_BURSTABLE"], NO.BESTEFFORT: K["SPX_QOS_BESTEFFORT"]}
HAS_NRT, PLACEMENT = K["SPX_NRT_F_HAS_NRT"], K["SPX_PNRT_F_PLACEMENT"]


class _Host:
    """the flatteners are host code and need no engine (no GPU here)"""
    _lib = spx.lib()
    _hdr = HDR
    _err = SpxError
    _h = None
    _ck_static = staticmethod(Engine._ck_static)
    _PNRT_NODE_COLS, _PNRT_POD_COLS = Engine._PNRT_NODE_COLS, Engine._PNRT_POD_COLS

    def _ck(self, rc):
        if rc != 0:
            raise SpxError(rc, "")

    flatten_quota = Engine.flatten_quota
    flatten_preempt_nodes = Engine.flatten_preempt_nodes
    flatten_nrt_pods = Engine.flatten_nrt_pods
    flatten_nrt_long_pods = Engine.flatten_nrt_long_pods
    flatten_preempt_nrt = Engine.flatten_preempt_nrt
    preempt_nrt_table = Engine.preempt_nrt_table
    preempt_nrt_check = Engine.preempt_nrt_check


def flatten(kw):
    t, h = NC.tables(**kw), _Host()
    f = h.flatten_preempt_nodes(t["nodes"], t["rc"], t["quota"], t["preempt"])
    return t, f, NC.flatten_nrt(h, t, f)


def test_the_flattened_pods_are_the_models():
    """the containers the decoration gave the pods add up to the model's request vectors: NodeResourcesFit sees what it saw before"""
    for name in ("64x64", "one-slot"):
        kw = NC.SHAPES[name]
        m = NC.model(**kw)
        t, f, g = flatten(kw)
        for j, src in enumerate(f["pod_src"]):
            node, k = t["assigned_at"][int(src)]
            assert f["pod_fit_req"][j].tolist() == m["nodes"][node]["pods"][k]["fit"]
        fq = _Host().flatten_quota(t["pods"], t["rc"], t["quota"])["cols"]["pod_req"].reshape(-1, 8)
        assert [r[:3] + r[4:] for r in fq.tolist()] == [p["fit"][:3] + p["fit"][4:] for p in m["pending"]]
        assert g["R"] == (1 if name == "one-slot" else 8)
        assert g["pods"]["qos"].tolist() == [QOS[NO.pod_qos(p)] for p in m["pending"]]


def post_eviction(t, m, n, victims):
    """spx_nrt_post_eviction for the pods at the positions `victims` of node n's list in the model: (code, zres_avail_out)"""
    node = m["nodes"][n]
    res = objects.Resources()
    for name in objects.PREEMPT_SCALARS + (NC.EXTRA,):
        res.id(name)
    pods = [node["pods"][k] for k in victims]
    vt = objects.build_pod_objects(HDR, res, [objects._preempt_pod(p) for p in pods]) if pods else None
    qos = np.array([QOS[NO.pod_qos(p)] for p in pods] + [0], dtype=np.uint8)
    numa = np.array([(node["placement"] or {}).get((p["key"], c["name"]), NC.UNKNOWN) for p in pods for c in p["containers"]] + [0], dtype=np.int32)
    s = t["nrt"].struct
    e0, e1 = s.zres_ptr[s.zone_ptr[n]], s.zres_ptr[s.zone_ptr[n + 1]]
    out, code = np.zeros(max(e1 - e0, 1), np.int64), C.c_int32(-1)
    assert spx.lib().spx_nrt_post_eviction(t["nrt"].ref(), t["nrt_rc"].ref(), n, vt.ref() if vt else None, qos.ctypes.data_as(C.POINTER(C.c_uint8)),
                                           numa.ctypes.data_as(C.POINTER(C.c_int32)), int(t["placement_present"][n]), int(t["placement_containers"][n]),
                                           out.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(code)) == 0
    return code.value, out[:e1 - e0].tolist()


def from_table(t, f, g, n, table_positions):
    """what the device concludes from the side table for the stack `table_positions` (positions in the flattened list of node n):
    (code, available + releases in the order of the NRT's zone resources)"""
    R, flags = g["R"], int(g["node_flags"][n])
    s = t["nrt"].struct
    slot_of = {int(r): k for k, r in enumerate(g["slots"].array("slot_res")[:R])}
    live = [int(g["zone_avail"][n, z - s.zone_ptr[n], slot_of[s.zres_res[e]]]) for z in range(s.zone_ptr[n], s.zone_ptr[n + 1]) for e in range(s.zres_ptr[z], s.zres_ptr[z + 1])]
    if not flags & HAS_NRT:
        return K["SPX_EVICT_NO_NRT"], live
    if not table_positions:
        return K["SPX_EVICT_NO_VICTIMS"], live
    if not flags & PLACEMENT:
        return (K["SPX_EVICT_NO_CONTAINERS"] if t["placement_present"][n] else K["SPX_EVICT_NO_PLACEMENT"]), live
    sums = np.zeros((8, max(R, 1)), np.int64)
    contributing = 0
    for pos in table_positions:
        j = int(f["pod_ptr"][n]) + pos
        contributing += int(g["pod_contributes"][j])
        for k in range(g["rel_ptr"][j], g["rel_ptr"][j + 1]):
            assert g["rel_qty"][k] > 0
            sums[g["rel_zone"][k], g["rel_slot"][k]] += g["rel_qty"][k]
    if contributing == 0:
        return K["SPX_EVICT_NOTHING_TO_ADD"], live
    if (sums > g["zone_headroom"][n]).any():
        return K["SPX_EVICT_EXCEEDS_ALLOCATABLE"], live
    after = g["zone_avail"][n] + sums
    return K["SPX_EVICT_OK"], [int(after[z - s.zone_ptr[n], slot_of[s.zres_res[e]]]) for z in range(s.zone_ptr[n], s.zone_ptr[n + 1]) for e in range(s.zres_ptr[z], s.zres_ptr[z + 1])]


@pytest.mark.parametrize("name", ["64x64", "63x65", "one-slot"])
def test_sums_of_releases_are_the_eviction_simulation(name):
    """for random stacks of every node: available + the sum of the stack's releases, and which of the verdicts applies, are what
    spx_nrt_post_eviction gives for those victims, entry for entry"""
    kw = NC.SHAPES[name]
    m = NC.model(**kw)
    t, f, g = flatten(kw)
    rng = np.random.default_rng(17)
    seen = set()
    for n, node in enumerate(m["nodes"]):
        L = int(f["pod_ptr"][n + 1] - f["pod_ptr"][n])
        assert L == (len(node["pods"]) if node["present"] else 0)  # (the node table holds no pods of an absent node)
        model_pos = [t["assigned_at"][int(f["pod_src"][f["pod_ptr"][n] + pos])][1] for pos in range(L)]
        stacks = [[], list(range(L))] + [[p] for p in range(min(L, 4))] + [sorted(rng.choice(L, size=int(rng.integers(1, L + 1)), replace=False).tolist()) for _ in range(6 if L else 0)]
        for stack in stacks:
            want = post_eviction(t, m, n, [model_pos[p] for p in stack])
            assert from_table(t, f, g, n, stack) == want, (n, stack)
            seen.add(want[0])
    assert seen >= ({K["SPX_EVICT_OK"], K["SPX_EVICT_NO_VICTIMS"], K["SPX_EVICT_EXCEEDS_ALLOCATABLE"]} if name == "one-slot" else set(range(7)))


# ---------------------------------------------------------------------------------------------------------------- refusals
def raises_arg(fn, *names):
    with pytest.raises(SpxError) as err:
        fn()
    assert err.value.code == K["SPX_ERR_ARG"]
    for name in names:
        assert name in err.value.msg, err.value.msg


KW = NC.SHAPES["63x65"]


def tampered(change):
    """the flattener on the 63x65 model after change(model): the node table's pod order (pod_src) is the untouched model's"""
    t, f, _ = flatten(KW)
    m = copy.deepcopy(NC.model(**KW))
    change(m)
    return lambda: NC.flatten_nrt(_Host(), NC.build_tables(m), f)


def node_with(m, pred):
    return next(n for n, node in enumerate(m["nodes"]) if node["nrt"] is not None and pred(node))


def test_flattener_refuses_what_the_device_cannot_take_and_names_it():
    m0 = NC.model(**KW)
    n = node_with(m0, lambda node: len(node["pods"]) >= 2 and node["placement"])
    first = sum(len(x["pods"]) for x in m0["nodes"][:n])  # object index of the node's first pod

    def nine_zones(m):
        z = m["nodes"][n]["nrt"]["zones"]
        m["nodes"][n]["nrt"]["zones"] = [dict(z[0], name=f"node-{k}") for k in range(9)]
    raises_arg(tampered(nine_zones), f"node {n}")

    def over_allocatable(m):
        z = m["nodes"][n]["nrt"]["zones"][0]
        name, alloc, _ = z["resources"][0]
        z["resources"][0] = (name, alloc, alloc + 1)
    raises_arg(tampered(over_allocatable), f"node {n}")

    def listed_twice(m):
        z = m["nodes"][n]["nrt"]["zones"][0]
        z["resources"].append(z["resources"][0])
    raises_arg(tampered(listed_twice), f"node {n}")

    def extended(m, quantities):
        """the node's first pods request an extended resource its first zone reports, and sit on that zone"""
        node = m["nodes"][n]
        z = node["nrt"]["zones"][0]
        z["resources"].append((NC.EXTRA, (1 << 62) + 5, 0))
        for p, q in zip(node["pods"], quantities):
            p["containers"][0]["requests"][NC.EXTRA] = q
            node["placement"][(p["key"], "c0")] = NO.numa_id(z["name"])
    raises_arg(tampered(lambda m: extended(m, [-1])), f"assigned pod {first}")
    raises_arg(tampered(lambda m: extended(m, [1 << 61, 1 << 61])), f"node {n}")
    tampered(lambda m: extended(m, [1 << 60, 1 << 60]))()  # within the limit

    def more_than_eight_slots(m):
        m["nodes"][n]["nrt"]["zones"][0]["resources"] += [(f"example.com/more{k}", 4, 4) for k in range(7)]
    raises_arg(tampered(more_than_eight_slots), "SPX_NRT_MAX_RES")


def test_flattener_refuses_a_zone_the_filter_does_not_list():
    """a zone whose name parses to a NUMA id but is not of type Node: the simulation would add to it, the Filter never reads it"""
    t, f, _ = flatten(KW)
    m = NC.model(**KW)
    n = node_with(m, lambda node: True)
    nrt = t["nrt"]
    is_node = nrt.array("zone_is_node")
    z = int(nrt.struct.zone_ptr[n])
    is_node[z] = 0
    try:
        raises_arg(lambda: NC.flatten_nrt(_Host(), t, f), f"node {n}")
    finally:
        is_node[z] = 1


def test_check_names_the_node_the_pod_and_the_row():
    t, f, g = flatten(KW)
    h = _Host()
    assert h.preempt_nrt_check(g) == (0, -1)
    n = int(np.flatnonzero(g["n_zones"])[3])
    j = int(np.flatnonzero(np.diff(g["rel_ptr"]))[2])
    k = int(g["rel_ptr"][j])

    def with_(**cols):
        return dict(g, **cols)

    def poke(name, at, value):
        col = g[name].copy()
        col[at] = value
        return with_(**{name: col})

    assert h.preempt_nrt_check(poke("n_zones", n, 9)) == (1, n)
    assert h.preempt_nrt_check(poke("zone_headroom", (n, 0, 0), -1)) == (1, n)  # available > allocatable
    assert h.preempt_nrt_check(poke("zone_id", (n, 0), 64)) == (1, n)
    assert h.preempt_nrt_check(poke("rel_qty", k, -1)) == (2, j)
    assert h.preempt_nrt_check(poke("rel_qty", k, 1 << 62)) == (2, j)
    assert h.preempt_nrt_check(poke("rel_slot", k, g["R"])) == (2, j)
    assert h.preempt_nrt_check(poke("rel_zone", k, 8)) == (2, j)
    pods = objects_long_row(g["pods"], 5)
    assert h.preempt_nrt_check(with_(pods=pods)) == (3, 5)  # more than 8 containers: a long row
    assert h.preempt_nrt_check(with_(R=g["R"] + 1))[0] == 4  # the pods' n_res is not the slots'
    kind, bad = C.c_int32(), C.c_int64()
    assert spx.lib().spx_flatten_preempt_nrt_check(None, C.byref(kind), C.byref(bad)) == K["SPX_ERR_ARG"] and kind.value == 4


def objects_long_row(pods, row):
    out = type(pods)({k: v.copy() for k, v in pods.items()})
    out["n_ctr"][row] = K["SPX_NRT_CTRS_LONG"]
    return out
