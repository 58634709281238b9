"""NodeMetadata (plugin 11) and PodState (plugin 12) on the GPU: the raw int64 node column, NormalizeScore over each pod's feasible
nodes (kernels_node_columns.hip), against the plain-Python reference (tests/node_columns_ref.py; tests/test_node_columns_host.py
holds that reference to its edges on the CPU) on CONSTRUCTED columns and feasible sets.  Engine.upload_nodemeta / upload_podstate
take the raw column and Engine.upload_feasible_mask gives the feasible sets: no flattener stands between the test and the kernels.
Every byte of a feasible node is compared at tolerance 0, and (NodeMetadata) every invalid node's byte must be 0."""
import numpy as np
import pytest

import node_columns_ref as R
from helpers import ALLOCATABLE, LVRB, NETOVERHEAD, NRT, TLP, lvrb_params, tlp_params
from scheduler_plugins_amd import SpxError
from scheduler_plugins_amd import objects as O
from scheduler_plugins_amd import synth
from scheduler_plugins_amd.engine import NODEMETA, NUM_PLUGINS, PODSTATE, Engine, mask_of

pytestmark = pytest.mark.gpu

PLUGIN = {R.META: NODEMETA, R.PODSTATE: PODSTATE}
ERR_ARG, ERR_STATE = -1, -3


def upload(e, kind, raw):
    (e.upload_nodemeta if kind == R.META else e.upload_podstate)(raw)


def spans_for(kind, n):
    if kind == R.PODSTATE:
        return (R.podstate_span(n), 100)
    k = R.NODES.index(n)  # three of the ten ranges per node count; test_every_range runs them all
    return tuple(R.RANGES[(k + j * 3) % len(R.RANGES)] for j in range(3))


def row_ranges(p):
    return sorted({(0, p), (min(1, p - 1), min(2, p)), (p - 1, p)})


def check_table(e, t, failures, tag):
    """both regimes on one engine: the rows under the table's masks (every row range), then without a mask (every row the same)"""
    plugin = PLUGIN[t.kind]
    upload(e, t.kind, t.raw)
    e.upload_feasible_mask(t.masks)
    assert np.array_equal(e.raw(plugin, 0), np.array(t.raw, dtype=np.int64))  # INT64_MIN kept
    for rb, re in row_ranges(t.n_rows):
        e.eval(mask_of(plugin), rb, re)
        e.sync()
        failures += t.mismatches(e.all_scores(plugin, rb, re), rb, re, f"{tag} masked [{rb},{re})")
    e.upload_feasible_mask(None)
    for rb, re in row_ranges(t.n_rows):
        e.eval(mask_of(plugin), rb, re)
        e.sync()
        got = e.all_scores(plugin, rb, re)
        for r in np.flatnonzero((got != t.unmasked).any(axis=1))[:2]:
            n = int(np.flatnonzero(got[r] != t.unmasked)[0])
            failures.append(f"{tag} {t.label}: broadcast [{rb},{re}) row {rb + r} node {n} (raw {t.raw[n]}): got {got[r, n]} want {t.unmasked[n]}")


@pytest.mark.parametrize("n_nodes", R.NODES)
@pytest.mark.parametrize("kind", [R.META, R.PODSTATE])
def test_rows_on_constructed_columns(gpu_required, kind, n_nodes):
    """node counts around the 64-lane wave and the 256-node tile, 1, 2 and 65 pod rows (one workgroup on a single row, a wave per row
    in a batch, a batch whose count is no multiple of 4), row ranges [0, P), [1, 2) and the last row, rows padded to 128 and to 16 bytes"""
    failures = []
    for p in R.PODS:
        for align in ((128, 16) if p == 65 else (128,)):
            for span in spans_for(kind, n_nodes):
                for place in R.placements(n_nodes):
                    t = R.table(kind, n_nodes, p, span, place)
                    with Engine(0) as e:
                        e.set_option("ROW_ALIGN", align)
                        check_table(e, t, failures, f"align {align}")
    assert not failures, "\n".join([f"{len(failures)} cells"] + failures[:10])


@pytest.mark.parametrize("span", R.RANGES)
def test_every_range(gpu_required, span):
    """max - min from 1 to 2^64 - 2: the float64-reciprocal quotient below 2^40, the plain int64 sequence above, the wrapping product
    from floor(2^63 / 99) + 1 on, the range that is itself negative from 2^63 on; also with a whole workgroup per row"""
    failures = []
    for place in R.placements(257):
        t = R.table(R.META, 257, 65, span, place)
        for opt in (0, 1):
            with Engine(0) as e:
                e.set_option("ROW_WORKGROUP", opt)
                check_table(e, t, failures, f"row_workgroup {opt}")
    assert not failures, "\n".join([f"{len(failures)} cells"] + failures[:10])


def test_podstate_limits(gpu_required):
    lim = (1 << 31) - 1
    t = R.table(R.PODSTATE, 257, 65, 2 * lim, (255, 256))
    assert min(t.raw) == -lim and max(t.raw) == lim
    with Engine(0) as e:
        for bad in (1 << 31, -(1 << 31), R.INT64_MIN, R.INT64_MAX):
            with pytest.raises(SpxError) as ei:
                e.upload_podstate([0, bad, 1])
            assert ei.value.code == ERR_ARG and "2^31" in ei.value.msg
        failures = []
        check_table(e, t, failures, "limits")
        assert not failures, "\n".join(failures[:10])


@pytest.mark.parametrize("kind", [R.META, R.PODSTATE])
def test_bound_table_and_rows_outside_the_range(gpu_required, kind):
    """a table the caller bound: the same bytes, and no byte of a row outside [row_begin, row_end) is touched, in either regime"""
    import torch
    plugin = PLUGIN[kind]
    t = R.table(kind, 257, 65, spans_for(kind, 257)[0], (255, 256))
    with Engine(0) as e:
        upload(e, kind, t.raw)
        e.upload_feasible_mask(t.masks)
        _, stride, rows = e.score_table(ALLOCATABLE)  # the engine's row stride
        assert stride == 384 and rows == 65
        slab = torch.full((rows, stride), 0xAB, dtype=torch.uint8, device="cuda:0")
        e.bind_score_table(plugin, slab.data_ptr(), stride, rows)
        for masked in (True, False):
            e.upload_feasible_mask(t.masks if masked else None)
            for rb, re in ((1, 2), (64, 65), (3, 41), (0, 65)):
                slab.fill_(0xAB)
                torch.cuda.synchronize()
                e.eval(mask_of(plugin), rb, re)
                e.sync()
                got = slab.cpu().numpy()
                outside = np.ones(rows, bool)
                outside[rb:re] = False
                assert (got[outside] == 0xAB).all(), (masked, rb, re)
                if masked:
                    assert not t.mismatches(got[rb:re, :257], rb, re)
                else:
                    assert (got[rb:re, :257] == t.unmasked).all()
                assert np.array_equal(e.all_scores(plugin, rb, re), got[rb:re, :257])
        e.bind_score_table(plugin, 0, 0, 0)


def best_reference(tables, weights, feasible):
    """numpy: per row the weighted total's maximum over feasible nodes, its lowest node, the number of nodes that reach it, the feasible count"""
    total = sum(int(w) * tables[p].astype(np.int64) for p, w in weights.items())
    node, score, ties, feas = [], [], [], []
    for r in range(feasible.shape[0]):
        idx = np.flatnonzero(feasible[r])
        if len(idx) == 0:
            node.append(-1), score.append(0), ties.append(0), feas.append(0)
            continue
        m = total[r, idx].max()
        node.append(int(idx[np.flatnonzero(total[r, idx] == m)[0]])), score.append(int(m)), ties.append(int((total[r, idx] == m).sum())), feas.append(len(idx))
    return np.array(node), np.array(score), np.array(ties), np.array(feas)


def load_alloc(e, raw):
    e.set_allocatable("Most", {1: 1})
    e.upload_alloc_nodes(np.array([raw], dtype=np.int64))


@pytest.mark.parametrize("unfused", [0, 1])
def test_eval_best_and_decide_next_to_allocatable(gpu_required, unfused):
    """spx_eval + spx_eval_best and spx_decide with weights on the new plugins, next to Allocatable under the same caller mask, against
    a numpy sum of the reference tables: score, node, ties, feasible"""
    tm = R.table(R.META, 257, 65, 1 << 32, (255, 256))
    tp = R.table(R.PODSTATE, 257, 65, 100, (0, 256), seed=3)
    rng = np.random.default_rng(5)
    alloc_raw = [int(v) for v in rng.integers(0, 1000, 257)]
    masks = tm.masks
    feasible = masks != 0
    want = {NODEMETA: tm.want, PODSTATE: R.rows(R.PODSTATE, tp.raw, masks), ALLOCATABLE: R.rows(R.PODSTATE, alloc_raw, masks)}  # (Allocatable's rule is PodState's)
    for weights in ({ALLOCATABLE: 1, NODEMETA: 1, PODSTATE: 1}, {ALLOCATABLE: 3, NODEMETA: 2, PODSTATE: 5}, {ALLOCATABLE: 0, NODEMETA: 1, PODSTATE: 0}):
        ref = best_reference(want, weights, feasible)
        with Engine(0) as e:
            e.set_option("DECIDE_UNFUSED", unfused)
            load_alloc(e, alloc_raw)
            e.upload_nodemeta(tm.raw)
            e.upload_podstate(tp.raw)
            e.upload_feasible_mask(masks)
            e.set_plugin_weights(weights)
            m = mask_of(ALLOCATABLE, NODEMETA, PODSTATE)
            e.eval(m)
            e.eval_best(m)
            e.sync()
            for p in (ALLOCATABLE, PODSTATE):
                assert ((e.all_scores(p) == want[p]) | ~feasible).all(), p
            got = e.best()
            for g, w, name in zip(got, ref, ("node", "score", "ties", "feasible")):
                assert np.array_equal(g, w), (weights, name, np.flatnonzero(g != w)[:5])
            # the mask changed: the tables were normalised under another feasible set
            flipped = masks.copy()
            flipped[:, 0] ^= 1
            e.upload_feasible_mask(flipped)
            with pytest.raises(SpxError) as ei:
                e.eval_best(m)
            assert ei.value.code == ERR_STATE and "NodeMetadata / PodState" in ei.value.msg
            e.upload_feasible_mask(masks)
            e.decide(m)
            e.sync()
            for g, w, name in zip(e.best(), ref, ("node", "score", "ties", "feasible")):
                assert np.array_equal(g, w), ("decide", weights, name, np.flatnonzero(g != w)[:5])


def test_one_byte_of_the_new_table_decides_the_winner(gpu_required):
    """node 10 wins by exactly one weighted point that NodeMetadata's table supplies: one byte off there and the winner is node 20"""
    n = 65
    meta = [0] * n
    meta[10], meta[20], meta[64] = 6400, 6336, R.INVALID   # bytes 100 and 99 over the range [0, 6400]; node 64 has no valid metadata: 0
    alloc = [0] * n
    alloc[64], alloc[20] = 100, 1     # Allocatable bytes: node 64 -> 100, node 20 -> 1, node 10 -> 0
    mask = np.ones((2, n), np.uint8)
    mask[1, 10] = 0                   # second row: without node 10 the winner is node 64 under weight 1, node 20 under weight 2
    want = {NODEMETA: R.rows(R.META, meta, mask), ALLOCATABLE: R.rows(R.PODSTATE, alloc, mask)}
    assert want[NODEMETA][0, 10] == 100 and want[NODEMETA][0, 20] == 99 and want[ALLOCATABLE][0, 20] == 1 and want[ALLOCATABLE][0, 10] == 0
    for w_meta, first in ((2, (10, 200, 1)), (1, (10, 100, 3))):
        weights = {ALLOCATABLE: 1, NODEMETA: w_meta}
        ref = best_reference(want, weights, mask != 0)
        assert (ref[0][0], ref[1][0], ref[2][0]) == first
        if w_meta == 2:  # the margin is one point: the reference with node 20's byte one higher picks node 20
            off = {NODEMETA: want[NODEMETA].copy(), ALLOCATABLE: want[ALLOCATABLE]}
            off[NODEMETA][0, 20] += 1
            assert best_reference(off, weights, mask != 0)[0][0] == 20
        with Engine(0) as e:
            load_alloc(e, alloc)
            e.upload_nodemeta(meta)
            e.upload_feasible_mask(mask)
            e.set_plugin_weights(weights)
            m = mask_of(ALLOCATABLE, NODEMETA)
            e.eval(m)
            e.eval_best(m)
            e.sync()
            a = e.best()
            e.decide(m)
            e.sync()
            b = e.best()
            for g, h, w in zip(a, b, ref):
                assert np.array_equal(g, w) and np.array_equal(h, w)


def test_full_profile_with_filter_plugins(gpu_required, hdr, oracle):
    """one seeded profile, 70 nodes x 20 pods: NRT and NetworkOverhead supply the feasible sets, their and the trimaran plugins'
    tables come from the oracle, the new plugins' from the Python reference"""
    n_nodes, n_pods = 70, 20
    snap = synth.full_snapshot(hdr, n_nodes, n_pods, seed=4, pods_per_group=20, n_namespaces=20)
    cols = synth.node_column_snapshot(n_nodes, seed=4)
    weights = {ALLOCATABLE: 1, TLP: 2, LVRB: 1, NRT: 3, NETOVERHEAD: 2, NODEMETA: 2, PODSTATE: 1}
    allp = tuple(weights)
    with Engine(0) as e:
        params = O.nrt_params(hdr, O.Resources(), "LeastAllocated")
        e.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])
        e.load_nrt_objects(snap["nodes"], snap["nrt"], snap["rc"], snap["pods"], params)
        e.load_network_objects(snap["nodes"], snap["pods"], snap["appgroups"], snap["nettopo"])
        e.upload_nodemeta(cols["nodemeta"])
        e.upload_podstate(cols["podstate"])
        e.set_plugin_weights(weights)
        e.eval(mask_of(*allp))
        e.eval_best(mask_of(*allp))
        e.sync()
        osnap = oracle.Snapshot(snap["nodes"], snap["pods"], rc=snap["rc"], metrics=snap["metrics"], assigned=snap["assigned"],
                                alloc_params=e.alloc_params, tlp_params=tlp_params(hdr), lvrb_params=lvrb_params(hdr),
                                nrt=snap["nrt"], nrt_params=params, appgroups=snap["appgroups"], nettopo=snap["nettopo"])
        nrt_status, net_status = osnap.filter_rows(NRT), osnap.filter_rows(NETOVERHEAD)
        feasible = (nrt_status == 0) & (net_status == 0)
        assert feasible.any() and not feasible.all()
        want = {p: osnap.score_rows(p, want_norm=False)[0].clip(0, 255) for p in (TLP, LVRB, NRT)}
        want[NETOVERHEAD] = osnap.score_rows(NETOVERHEAD, mask=(nrt_status == 0).astype(np.uint8))[1]
        want[ALLOCATABLE] = osnap.score_rows(ALLOCATABLE, mask=feasible.astype(np.uint8))[1]
        want[NODEMETA] = R.rows(R.META, [int(v) for v in cols["nodemeta"]], feasible)
        want[PODSTATE] = R.rows(R.PODSTATE, [int(v) for v in cols["podstate"]], feasible)
        for p in (NODEMETA, PODSTATE):
            assert ((e.all_scores(p) == want[p]) | ~feasible).all(), p
        assert len({tuple(r) for r in e.all_scores(NODEMETA)}) > 1  # rows are no longer identical
        ref = best_reference(want, weights, feasible)
        for g, w, name in zip(e.best(), ref, ("node", "score", "ties", "feasible")):
            assert np.array_equal(g, w), name
        e.decide(mask_of(*allp))
        e.sync()
        for g, w, name in zip(e.best(), ref, ("node", "score", "ties", "feasible")):
            assert np.array_equal(g, w), ("decide", name)


def test_state(gpu_required):
    t = R.table(R.META, 65, 2, 100, (0, 64))
    tp = R.table(R.PODSTATE, 65, 2, 100, (0, 64))
    with Engine(0) as e:
        e.upload_feasible_mask(t.masks)
        for plugin, text in ((NODEMETA, "NodeMetadata node column not uploaded"), (PODSTATE, "PodState node column not uploaded")):
            with pytest.raises(SpxError) as ei:  # an evaluation before the upload
                e.eval(mask_of(plugin))
            assert ei.value.code == ERR_STATE and text in ei.value.msg
            with pytest.raises(SpxError) as ei:
                e.raw(plugin, 0)
            assert ei.value.code == ERR_STATE
        e.upload_nodemeta(t.raw)
        e.upload_podstate(tp.raw)
        m = mask_of(NODEMETA, PODSTATE)
        e.eval(m)
        e.sync()
        assert not t.mismatches(e.all_scores(NODEMETA), 0, 2) and not tp.mismatches(e.all_scores(PODSTATE), 0, 2)
        # uploading a column again invalidates "evaluated" — of that plugin alone
        other = [v if v == R.INVALID else v // 2 for v in t.raw]
        e.upload_nodemeta(other)
        with pytest.raises(SpxError) as ei:
            e.scores(NODEMETA, 0)
        assert ei.value.code == ERR_STATE
        assert not tp.mismatches(e.all_scores(PODSTATE), 0, 2)
        with pytest.raises(SpxError) as ei:
            e.eval_best(m)
        assert ei.value.code == ERR_STATE
        e.eval(mask_of(NODEMETA))
        e.sync()
        assert ((e.all_scores(NODEMETA) == R.rows(R.META, other, t.masks)) | (t.masks == 0)).all()
        # a reload with another node count: one snapshot shape per engine
        for up in (e.upload_nodemeta, e.upload_podstate):
            with pytest.raises(SpxError) as ei:
                up([1, 2, 3])
            assert ei.value.code == ERR_STATE and "n_nodes differs" in ei.value.msg
        e.n_nodes = 65
        assert ((e.all_scores(NODEMETA) == R.rows(R.META, other, t.masks)) | (t.masks == 0)).all()  # the refused upload changed nothing
        # the gate's id (10) lies inside the per-plugin arrays now and still owns no table
        with pytest.raises(SpxError):
            e.scores(10, 0)
        with pytest.raises(SpxError):
            e.score_table(10)
        assert NUM_PLUGINS == 13


def test_commit_sequential_declines_both(gpu_required, hdr):
    snap = synth.trimaran_snapshot(hdr, 64, 8, seed=2)
    cols = synth.node_column_snapshot(64, seed=2)
    with Engine(0) as e:
        e.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])
        e.upload_nodemeta(cols["nodemeta"])
        e.upload_podstate(cols["podstate"])
        m = mask_of(ALLOCATABLE, TLP, NODEMETA, PODSTATE)
        e.eval(m)
        e.sync()
        before = {p: e.all_scores(p).copy() for p in (ALLOCATABLE, TLP, NODEMETA, PODSTATE)}
        for extra in (NODEMETA, PODSTATE):
            with pytest.raises(SpxError) as ei:
                e.commit_sequential(mask_of(ALLOCATABLE, TLP, extra))
            assert ei.value.code == ERR_ARG and "spx_commit_sequential supports Allocatable / TargetLoadPacking" in ei.value.msg
        for p, w in before.items():
            assert np.array_equal(e.all_scores(p), w), p
