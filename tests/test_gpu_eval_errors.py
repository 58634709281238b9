"""Which error a bad spx_eval gets, and what such a call leaves behind.

The table: one entry per fault, and per pair of faults whose order decides the answer.  Code and text are literals, copied from
the source as it stood before spx_eval was split into eval_check / prepare_* / launch_* (csrc/spx_engine.hip); they are not obtained
from the engine.  Snapshots are 70 nodes x 8 pods: one full wave of nodes plus a tail; the pods do not matter to the checks.

The last two tests pin that a call eval_check refuses changes nothing a later call can observe.  Before the split the stride test of
a bound NRT table sat behind the quota launch and Coscheduling's gate, so both tests failed there: the refused call had built the
gate (spx_fetch_cosched_gap answered) and had rewritten the quota status bytes.
(Coscheduling: after a refused spx_eval the plugin is in no state in which spx_eval_best could reach its own "gate has not been
evaluated for these rows" text — the bit is not in `evaluated`, and the argmax says so first, before and after the split.  What does
tell the two apart is the gate itself: spx_fetch_cosched_gap, which asks for nothing but a valid gate.)"""
import functools

import numpy as np
import pytest

import cosched_cases as CC
import scheduler_plugins_amd as spx
from scheduler_plugins_amd import SpxError, synth
from scheduler_plugins_amd import objects as O
from scheduler_plugins_amd.engine import ALLOCATABLE, CAPACITY, COSCHED, LROC, LVRB, NETOVERHEAD, NRT, PEAKS, SYSCHED, TLP, Engine, mask_of

pytestmark = pytest.mark.gpu

N_NODES, N_PODS = 70, 8
ARG, STATE = "SPX_ERR_ARG", "SPX_ERR_STATE"
STRIDE = "bound score table must use the engine row stride (spx_score_table reports it)"


@functools.lru_cache(maxsize=None)
def tables():
    """the flat tables of one seeded 70 x 8 snapshot, every plugin family, computed once"""
    hdr = spx.header()
    s = synth.full_snapshot(hdr, N_NODES, N_PODS, seed=7, pods_per_group=4, n_namespaces=2)
    s["node_pods"] = synth.synth_node_pods(hdr, N_NODES, 7)
    s["power_models"] = synth.synth_power_models(hdr, N_NODES, 7)
    params = O.nrt_params(hdr, O.Resources(), "LeastAllocated")
    cs = CC.build(hdr, CC.draw_snapshot(seed=11, n_nodes=N_NODES, n_groups=2, n_walk=1, n_pending=N_PODS))
    with Engine(0) as e:
        t = {"alloc": e.flatten_alloc_nodes(s["nodes"], s["rc"]),
             "tri_nodes": e.flatten_trimaran_nodes(s["nodes"], s["metrics"], s["assigned"]),
             "tri_pods": e.flatten_trimaran_pods(s["pods"]),
             "lroc_nodes": e.flatten_lroc_nodes(s["nodes"], s["node_pods"]),
             "lroc_pods": e.flatten_lroc_pods(s["pods"]),
             "peaks": e.flatten_peaks(s["nodes"], s["metrics"], s["power_models"], s["pods"]),
             "nrt": e.flatten_nrt(s["nodes"], s["nrt"], s["rc"], s["pods"], params),
             "net": e.flatten_network(s["nodes"], s["pods"], s["appgroups"], s["nettopo"]),
             "quota": e.flatten_quota(s["pods"], s["rc"], s["quota"]),
             "sysched": e.flatten_sysched(synth.sysched_snapshot(hdr, N_NODES, N_PODS, seed=7)["objects"]),
             "cosched": e.flatten_cosched(cs[1], cs[2])}
        e.set_option("NRT_WIDE", 1)
        t["nrt_wide"] = e.flatten_nrt(s["nodes"], s["nrt"], s["rc"], s["pods"], params)
    assert t["nrt_wide"].get("wide") and not t["nrt"].get("wide")
    assert (t["sysched"]["N"], t["sysched"]["P"], t["cosched"]["N"], t["cosched"]["P"]) == (N_NODES, N_PODS, N_NODES, N_PODS)
    return t


# ------------------------------------------------------------------ engine states, named by what has been uploaded
def up_fresh(e, t):
    pass


def up_alloc(e, t):  # a node table, no pod table
    e.upload_alloc_nodes(t["alloc"])


def up_tri(e, t):  # nodes and pods known; trimaran and Allocatable only
    up_alloc(e, t)
    e.upload_trimaran_nodes(t["tri_nodes"])
    e.upload_trimaran_pods(t["tri_pods"])


def up_full(e, t):
    up_tri(e, t)
    e.upload_lroc_nodes(t["lroc_nodes"])
    e.upload_lroc_pods(t["lroc_pods"])
    e.upload_peaks(t["peaks"])
    e.upload_nrt(t["nrt"])
    e.upload_network(t["net"])
    e.upload_quota(t["quota"])


def up_wide_slots(e, t):  # the wide NRT slot table alone: the engine's NRT state is the wide one, without nodes and pods
    up_tri(e, t)
    e._ck(e._lib.spx_upload_nrt_slots_wide(e._h, t["nrt_wide"]["slots"].ref()))


def up_sysched(e, t):
    e.upload_sysched_nodes(t["sysched"]["nodes"])
    e.upload_sysched_pods(t["sysched"]["pods"])


def up_sysched_words(e, t):  # the pods' sets one word wider than the nodes'
    pods = t["sysched"]["pods"]
    e.upload_sysched_nodes(t["sysched"]["nodes"])
    e.upload_sysched_pods(dict(pods, set_bits=np.ascontiguousarray(np.pad(pods["set_bits"], ((0, 0), (0, 1))))))


ALL = mask_of(ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD, CAPACITY, LROC, PEAKS)

# (id, uploads, a plugin whose score table is bound with a foreign stride or None, mask, rows or None = all, code, text)
CASES = [
    ("mask_zero", up_full, None, 0, None, ARG, "plugin mask has unsupported bits"),
    ("mask_unknown_bit", up_full, None, ALL | (1 << 20), None, ARG, "plugin mask has unsupported bits"),
    ("lroc_missing", up_tri, None, mask_of(LROC), None, STATE, "LowRiskOverCommitment node/pod tables not uploaded"),
    ("peaks_missing", up_tri, None, mask_of(PEAKS), None, STATE, "Peaks node/pod tables not uploaded"),
    ("sysched_missing", up_tri, None, mask_of(SYSCHED), None, STATE, "SySched node/pod tables not uploaded"),
    ("cosched_missing", up_tri, None, mask_of(COSCHED), None, STATE, "Coscheduling tables not uploaded"),
    ("capacity_missing", up_tri, None, mask_of(CAPACITY), None, STATE, "CapacityScheduling quota tables not uploaded"),
    ("trimaran_missing", up_alloc, None, mask_of(TLP), None, STATE, "trimaran node/pod tables not uploaded"),
    ("nrt_dense_missing", up_tri, None, mask_of(NRT), None, STATE, "NRT slot/node/pod tables not uploaded"),
    ("nrt_wide_missing", up_wide_slots, None, mask_of(NRT), None, STATE, "NRT wide slot/node/pod tables not uploaded"),
    ("net_missing", up_tri, None, mask_of(NETOVERHEAD), None, STATE, "NetworkOverhead node/topology/pod tables not uploaded"),
    ("no_node_table", up_fresh, None, mask_of(ALLOCATABLE), None, STATE, "no node table uploaded"),
    ("n_pods_unknown", up_alloc, None, mask_of(ALLOCATABLE), (0, 0), STATE, "n_pods unknown: upload a pod table first"),
    ("rows_past_the_end", up_full, None, ALL, (0, N_PODS + 1), ARG, "row range out of bounds"),
    ("rows_negative", up_full, None, ALL, (-1, 2), ARG, "row range out of bounds"),
    ("rows_reversed", up_full, None, ALL, (5, 4), ARG, "row range out of bounds"),
    ("sysched_n_words", up_sysched_words, None, mask_of(SYSCHED), None, STATE, "SySched: the node and pod tables differ in n_words"),
    ("stride_tlp", up_full, TLP, ALL, None, STATE, STRIDE),
    ("stride_lroc", up_full, LROC, ALL, None, STATE, STRIDE),
    ("stride_peaks", up_full, PEAKS, ALL, None, STATE, STRIDE),
    ("stride_sysched", up_sysched, SYSCHED, mask_of(SYSCHED), None, STATE, STRIDE),
    ("stride_nrt", up_full, NRT, ALL, None, STATE, STRIDE),
    ("stride_net", up_full, NETOVERHEAD, ALL, None, STATE, STRIDE),
    # two faults at once: the order of the checks decides
    ("lroc_missing_before_bad_rows", up_tri, None, mask_of(LROC), (0, 99), STATE, "LowRiskOverCommitment node/pod tables not uploaded"),
    ("peaks_missing_before_no_node_table", up_fresh, None, mask_of(PEAKS), None, STATE, "Peaks node/pod tables not uploaded"),
    ("bad_rows_before_nrt_missing", up_tri, None, mask_of(NRT), (0, 99), ARG, "row range out of bounds"),
    ("trimaran_missing_before_nrt_missing", up_alloc, None, mask_of(TLP, NRT), None, STATE, "trimaran node/pod tables not uploaded"),
]


def bind_foreign_stride(e, plugin):
    """binds `plugin`'s score table to caller memory of n_pods rows whose stride is 16 bytes more than the engine's; returns the slab"""
    import torch
    _, stride, rows = e.score_table(plugin)
    slab = torch.zeros(rows * (stride + 16), dtype=torch.uint8, device="cuda:0")
    e.bind_score_table(plugin, slab.data_ptr(), stride + 16, rows)
    return slab


def expect(e, hdr, code, text, call):
    with pytest.raises(SpxError) as err:
        call()
    assert (err.value.code, err.value.msg) == (hdr.consts[code], text)
    assert e._lib.spx_last_error(e._h).decode() == text


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_error_table(gpu_required, hdr, case):
    _, uploads, bound, mask, rows, code, text = case
    t = tables()
    with Engine(0) as e:
        uploads(e, t)
        slab = bind_foreign_stride(e, bound) if bound is not None else None
        b, end = rows if rows is not None else (0, N_PODS)
        expect(e, hdr, code, text, lambda: e._ck(e._lib.spx_eval(e._h, mask, b, end)))
        if slab is not None:  # and the same call goes through once the table is the engine's own again
            e.bind_score_table(bound, 0, 0, 0)
            e.eval(mask, b, end)
            e.sync()
        del slab


def test_refused_call_leaves_coscheduling_gate_unbuilt(gpu_required, hdr):
    t = tables()
    f = t["cosched"]
    assert int((np.diff(f["step_ptr"]) > 0).sum()) > 0  # a gate with a walk: kernel_path(COSCHED) moves when it is built
    with Engine(0) as e:
        e.upload_cosched(f)
        e.upload_nrt(t["nrt"])
        slab = bind_foreign_stride(e, NRT)
        expect(e, hdr, STATE, STRIDE, lambda: e.eval(mask_of(COSCHED, NRT)))
        # no gate, no walk, no rows: what every reader of the gate says of an engine whose gate was never evaluated
        with pytest.raises(SpxError) as err:
            e.eval_best(mask_of(COSCHED))
        assert err.value.code == hdr.consts[STATE] and "has not been evaluated" in err.value.msg
        expect(e, hdr, STATE, "Coscheduling's gate has not been evaluated since its last upload", e.cosched_gap)
        expect(e, hdr, STATE, "Coscheduling's PreFilter has not been evaluated since its last upload", lambda: e.prefilter(COSCHED))
        assert e.kernel_path(COSCHED) == 0 and e.nrt_filter_path() == 0
        e.bind_score_table(NRT, 0, 0, 0)  # the same engine evaluates the same mask once the table is its own
        e.eval(mask_of(COSCHED, NRT))
        e.sync()
        with Engine(0) as fresh:
            fresh.upload_cosched(f)
            fresh.eval(mask_of(COSCHED))
            assert np.array_equal(e.prefilter(COSCHED), fresh.prefilter(COSCHED))
        del slab


def test_refused_call_leaves_quota_status_bytes(gpu_required, hdr):
    t = tables()
    q = t["quota"]
    ns = q["ns"]
    # two quota tables over the same pods: without any ElasticQuota every pod passes; with every namespace at its Max none with a request does
    open_q = dict(q, ns=dict(ns, has_quota=np.zeros_like(ns["has_quota"])))
    full_max, full_used = ns["max"].copy().reshape(-1, 8), ns["used"].copy().reshape(-1, 8)
    full_max[:, :3], full_used[:, :3] = 1, 1
    shut_q = dict(q, ns=dict(ns, has_quota=np.ones_like(ns["has_quota"]), max=full_max.reshape(-1), used=full_used.reshape(-1)))
    with Engine(0) as e, Engine(0) as other:
        up_full(e, t)
        e.upload_quota(open_q)
        e.eval(mask_of(CAPACITY, TLP))
        e.eval_best(mask_of(CAPACITY, TLP))
        e.sync()  # (spx_fetch_prefilter copies CapacityScheduling's bytes without waiting for the engine stream)
        good, good_best = e.prefilter(CAPACITY).copy(), e.best()
        e.upload_quota(shut_q)  # what the next evaluation would write ...
        up_full(other, t)
        other.upload_quota(shut_q)
        other.eval(mask_of(CAPACITY, TLP))
        other.eval_best(mask_of(CAPACITY, TLP))
        other.sync()
        assert (other.prefilter(CAPACITY) != good).any()  # ... differs from what the good call left, and so would the argmax over it
        assert any(not np.array_equal(x, y) for x, y in zip(other.best(), good_best))
        slab = bind_foreign_stride(e, NRT)
        expect(e, hdr, STATE, STRIDE, lambda: e.eval(mask_of(CAPACITY, NRT)))
        e.sync()
        assert np.array_equal(e.prefilter(CAPACITY), good)
        e.eval_best(mask_of(CAPACITY, TLP))
        for x, y in zip(e.best(), good_best):
            assert np.array_equal(x, y)
        del slab
