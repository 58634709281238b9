"""NodeResourceTopologyMatch's long-row and wide kernels (kernels_nrt_long.hip, kernels_nrt_wide.hip) at their edges: NUMA ids that
are not list positions (permuted; sparse in 0..63), extra resources in later, init and sidecar containers, zone quantities decided
by the charges of the containers before, more non-zero slots than the wide kernel caches, pods of exactly 8 / 9 / 63 / 64 (wide) and
8 / 9 / 64 / 65 / 200 (dense long rows) containers.  The examples are tests/nrt_edges.py's lists; tests/test_nrt_edges_host.py shows
with the oracle alone that every one of them holds its edge.  Every cell against the CPU oracle: status exact, uint8 score equal to
the raw score clipped to 0..255 (tolerance 0, as tests/test_gpu_nrt_long.py and tests/test_gpu_nrt_wide.py state).

Outside the tests on purpose, because the reference is undefined there: NUMA ids that are not a permutation of the positions under
LeastNUMANodes (subtractFromNUMAs panics out of range), empty request lists in Guaranteed pods, and a Guaranteed container that does
not name both cpu and memory (the single-entry and all-zero lists are containers of Burstable pods)."""
import numpy as np
import pytest
from hypothesis import given, settings
from hypothesis import strategies as st

import nrt_edges as E
from helpers import NRT
from scheduler_plugins_amd import SpxError
from scheduler_plugins_amd import objects as O
from scheduler_plugins_amd.engine import Engine, mask_of
from test_gpu_nrt_long import ALLP, WEIGHTS, _full_long, _load_full, _osnap
from test_gpu_nrt_wide import POOLS
from test_gpu_property import COMMON

pytestmark = pytest.mark.gpu

STRATEGIES = E.STRATEGIES
CONTAINER_FAILS = 4


def _want(oracle, snap, params):
    osnap = oracle.Snapshot(snap["nodes"], snap["pods"], rc=snap["rc"], nrt=snap["nrt"], nrt_params=params)
    th = oracle.usable_cpus()
    return osnap.filter_rows(NRT, threads=th), osnap.score_rows(NRT, want_norm=False, threads=th)[0]


def _every_cell(e, want_st, want_raw, tag):
    got_st, got_sc = e.all_status(NRT), e.all_scores(NRT)
    bad = np.argwhere(got_st != want_st)
    assert bad.size == 0, ("status", tag, len(bad), [(int(p), int(n), int(got_st[p, n]), int(want_st[p, n])) for p, n in bad[:5]])
    bad = np.argwhere(got_sc.astype(np.int64) != want_raw.clip(0, 255))
    assert bad.size == 0, ("score", tag, len(bad), [(int(p), int(n), int(got_sc[p, n]), int(want_raw[p, n])) for p, n in bad[:5]])
    return got_st, got_sc


def _raw_rows(e, edges, want_raw, tag):
    for r in edges["rows"][:8]:
        assert np.array_equal(e.raw(NRT, r), want_raw[r]), (tag, r)


# ------------------------------------------------------------------ property tests over nrt_edges' example lists
@settings(max_examples=len(E.EXAMPLES_LONG), **COMMON)
@given(ex=st.sampled_from(E.EXAMPLES_LONG))
def test_long_rows_at_their_edges(gpu_required, hdr, oracle, ex):
    """the dense tables with k_nrt_long on the rows of more than eight containers; also in two row ranges that split a run of long
    rows and with the reference-arithmetic kernels, byte-equal"""
    snap, edges = E.build(hdr, ex)
    params = O.nrt_params(hdr, O.Resources(), ex.strategy)
    want_st, want_raw = _want(oracle, snap, params)
    n_ctr = np.diff(snap["pods"].array("ctr_ptr"))
    n_long, P = int((n_ctr > 8).sum()), len(n_ctr)
    with Engine(0) as e:
        e.load_nrt_objects(snap["nodes"], snap["nrt"], snap["rc"], snap["pods"], params)
        assert not e.nrt_wide()
        if ex.numa_ids != "position":
            assert e.kernel_path(NRT) == 0
        e.eval(mask_of(NRT))
        e.sync()
        assert e.nrt_long_rows() == n_long and n_long >= 5
        got_st, got_sc = _every_cell(e, want_st, want_raw, ex)
        _raw_rows(e, edges, want_raw, ex)
        cut = edges["charge"]["ok"]  # rows cut - 1 and cut are both long
        assert n_ctr[cut - 1] > 8 and n_ctr[cut] > 8
        e.eval(mask_of(NRT), cut, P)
        assert e.nrt_long_rows() == int((n_ctr[cut:] > 8).sum())
        e.eval(mask_of(NRT), 0, cut)
        assert e.nrt_long_rows() == int((n_ctr[:cut] > 8).sum())
        e.sync()
        assert np.array_equal(e.all_status(NRT), got_st) and np.array_equal(e.all_scores(NRT), got_sc)
        e.force_reference_kernels(NRT)
        e.eval(mask_of(NRT))
        e.sync()
        assert e.nrt_long_rows() == n_long
        assert np.array_equal(e.all_status(NRT), got_st) and np.array_equal(e.all_scores(NRT), got_sc)


@settings(max_examples=len(E.EXAMPLES_WIDE), **COMMON)
@given(ex=st.sampled_from(E.EXAMPLES_WIDE))
def test_wide_snapshot_at_its_edges(gpu_required, hdr, oracle, ex):
    """k_nrt_wide on snapshots of 9, 12 and 32 slots, and through SPX_OPT_NRT_WIDE on 4 and 6 slots: there also byte-equal to the dense
    route (the dense sweeps + k_nrt_long) of a fresh engine"""
    snap, edges = E.build(hdr, ex)
    params = O.nrt_params(hdr, O.Resources(), ex.strategy)
    want_st, want_raw = _want(oracle, snap, params)
    P = int(snap["pods"].struct.n_pods)
    with Engine(0) as e:
        if ex.slots <= 6:
            e.set_option("NRT_WIDE", 1)
        e.load_nrt_objects(snap["nodes"], snap["nrt"], snap["rc"], snap["pods"], params)
        assert e.nrt_wide()
        e.eval(mask_of(NRT))
        e.sync()
        assert e.nrt_filter_path() == 4 and e.nrt_long_rows() == 0
        got_st, got_sc = _every_cell(e, want_st, want_raw, ex)
        _raw_rows(e, edges, want_raw, ex)
        cut = edges["charge"]["ok"]
        e.eval(mask_of(NRT), cut, P)
        e.eval(mask_of(NRT), 0, cut)
        e.sync()
        assert np.array_equal(e.all_status(NRT), got_st) and np.array_equal(e.all_scores(NRT), got_sc)
    if ex.slots <= 6:
        with Engine(0) as e:
            e.load_nrt_objects(snap["nodes"], snap["nrt"], snap["rc"], snap["pods"], params)
            assert not e.nrt_wide()
            e.eval(mask_of(NRT))
            e.sync()
            assert e.nrt_long_rows() == int((np.diff(snap["pods"].array("ctr_ptr")) > 8).sum())
            assert np.array_equal(e.all_status(NRT), got_st) and np.array_equal(e.all_scores(NRT), got_sc)


# ------------------------------------------------------------------ hand-built cases
def _zone(zid, cpu, all_ids, pools=None, mem="64Gi"):
    r = {"cpu": str(cpu), "memory": mem}
    r.update({name: str(q) for name, q in zip(POOLS, pools or [])})
    return {"name": f"node-{zid}", "type": "Node", "resources": r, "costs": {f"node-{j}": (10 if j == zid else 20) for j in all_ids}}


def _g(cpu, extra=None, mem="1Mi"):  # a Guaranteed container
    rl = {"cpu": cpu, "memory": mem}
    rl.update(extra or {})
    return O.container(rl, dict(rl))


def _tables(hdr, pods_spec, zones_per_node, policy, strategy, wide):
    res = O.Resources()
    if wide:
        for name in POOLS:
            res.id(name)
    pods = O.build_pod_objects(hdr, res, pods_spec)
    nrts = O.build_nrt_objects(hdr, res, [O.nrt(z, [policy]) for z in zones_per_node])
    tot = {"cpu": "64", "memory": "512Gi"}
    if wide:
        tot.update({name: "256" for name in POOLS})
    nodes = O.build_node_objects(hdr, res, [O.node(tot, tot) for _ in zones_per_node])
    return dict(nodes=nodes, pods=pods, nrt=nrts, rc=res.table(hdr)), O.nrt_params(hdr, res, strategy)


def _hand(hdr, oracle, pods_spec, zones_per_node, strategy, wide, policy="SingleNUMANodeContainerLevel"):
    """-> (status, raw) [pods][nodes] of the oracle, after the GPU's tables were found equal to them.  wide: the zones carry nine more
    resources (11 slots), so the wide tables and k_nrt_wide run; else the dense tables and, for rows above eight containers, k_nrt_long"""
    snap, params = _tables(hdr, pods_spec, zones_per_node, policy, strategy, wide)
    want_st, want_raw = _want(oracle, snap, params)
    with Engine(0) as e:
        e.load_nrt_objects(snap["nodes"], snap["nrt"], snap["rc"], snap["pods"], params)
        assert e.nrt_wide() == wide
        e.eval(mask_of(NRT))
        e.sync()
        n_long = sum(len(p["containers"]) + len(p["init_containers"]) > 8 for p in pods_spec)
        assert e.nrt_long_rows() == (0 if wide else n_long)
        assert (e.nrt_filter_path() == 4) == wide
        _every_cell(e, want_st, want_raw, (strategy, wide))
        for r in range(len(pods_spec)):
            assert np.array_equal(e.raw(NRT, r), want_raw[r]), r
    return want_st, want_raw


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_sixty_four_containers_in_a_wide_snapshot(gpu_required, hdr, oracle, strategy):
    """SPX_NRT_WIDE_MAX_CTRS app containers of one pool8 unit each (the last row of the kernel's record table): node 0 holds 32 + 31,
    so container 64 is the one that fails there; node 1 holds 32 + 32"""
    ids = (0, 1)
    node0 = [_zone(0, 8, ids, [4] * 8 + [32]), _zone(1, 8, ids, [4] * 8 + [31])]
    node1 = [_zone(0, 8, ids, [4] * 8 + [32]), _zone(1, 8, ids, [4] * 8 + [32])]
    ctr = _g("100m", {POOLS[8]: "1"})
    st_, raw = _hand(hdr, oracle, [O.pod([ctr] * 64), O.pod([ctr] * 63)], [node0, node1], strategy, wide=True)
    assert st_.tolist() == [[CONTAINER_FAILS, 0], [0, 0]]
    assert raw[0, 1] > 0


def test_sixty_five_containers_refused_on_a_wide_snapshot(gpu_required, hdr, oracle):
    """one container more than the record table holds: SPX_ERR_ARG naming the row; the engine takes a valid load afterwards (of as
    many rows: an engine keeps one batch size)"""
    ids = (0, 1)
    node = [_zone(0, 8, ids, [4] * 8 + [40]), _zone(1, 8, ids, [4] * 8 + [40])]
    ctr = _g("100m", {POOLS[8]: "1"})
    bad, params = _tables(hdr, [O.pod([ctr] * 3), O.pod([ctr] * 64), O.pod([ctr] * 65)], [node], "SingleNUMANodeContainerLevel", "LeastAllocated", True)
    good, _ = _tables(hdr, [O.pod([ctr] * 3), O.pod([ctr] * 64), O.pod([ctr] * 63)], [node], "SingleNUMANodeContainerLevel", "LeastAllocated", True)
    with Engine(0) as e:
        with pytest.raises(SpxError) as err:
            e.load_nrt_objects(bad["nodes"], bad["nrt"], bad["rc"], bad["pods"], params)
        assert err.value.code == -1 and "row 2 " in err.value.msg and "65" in err.value.msg
        e.load_nrt_objects(good["nodes"], good["nrt"], good["rc"], good["pods"], params)
        assert e.nrt_wide()
        e.eval(mask_of(NRT))
        e.sync()
        _every_cell(e, *_want(oracle, good, params), "after the refusal")


@pytest.mark.parametrize("strategy", ["LeastAllocated", "LeastNUMANodes"])
def test_two_hundred_containers_in_a_dense_long_row(gpu_required, hdr, oracle, strategy):
    """200 app containers of 10m fill two zones of one core; the 201st finds none"""
    ids = (0, 1)
    node = [_zone(0, 1, ids), _zone(1, 1, ids)]
    st_, raw = _hand(hdr, oracle, [O.pod([_g("10m")] * 200), O.pod([_g("10m")] * 201)], [node], strategy, wide=False)
    assert st_[:, 0].tolist() == [0, CONTAINER_FAILS]
    assert raw[0, 0] > 0


@pytest.mark.parametrize("wide", [False, True], ids=["long", "wide"])
@pytest.mark.parametrize("strategy", ["LeastAllocated", "BalancedAllocation"])
def test_charge_goes_to_numa_id_forty(gpu_required, hdr, oracle, wide, strategy):
    """zones (id 40, id 3) in that list order.  The first container (3 cores) fits id 40 only; eight containers of 1m go to the lowest
    fitting id, 3, and leave 992m there; the last container fits only if id 40's zone, charged with 3 of its 4 cores, still holds it"""
    ids = (40, 3)
    node = [_zone(40, 4, ids, [4] * 9 if wide else None), _zone(3, 1, ids, [4] * 9 if wide else None)]
    head = [_g("3")] + [_g("1m")] * 8
    st_, _ = _hand(hdr, oracle, [O.pod(head + [_g("1")]), O.pod(head + [_g("1001m")]), O.pod([_g("3"), _g("3")])], [node], strategy, wide)
    assert st_[:, 0].tolist() == [0, CONTAINER_FAILS, CONTAINER_FAILS]


@pytest.mark.parametrize("wide", [False, True], ids=["long", "wide"])
def test_least_numa_charges_the_position_an_id_names(gpu_required, hdr, oracle, wide):
    """LeastNUMANodes, container scope, zones with ids (1, 0, 2) holding 4, 1 and 0 cores.  The first container (3 cores) takes the
    zone at position 0, whose id is 1; subtractFromNUMAs uses that id as a list position and empties position 1 instead
    (numaresources.go:184-215), so the second container of 3 cores still finds 4 cores at position 0: one zone each, a score above 0.
    With ids equal to positions the second container fits no subset and the score is 0"""
    pods = [O.pod([_g("3"), _g("3")] + [_g("1m")] * 8)]
    ids = (1, 0, 2)
    pp = [4] * 9 if wide else None
    _, raw = _hand(hdr, oracle, pods, [[_zone(1, 4, ids, pp), _zone(0, 1, ids, pp), _zone(2, 0, ids, pp)]], "LeastNUMANodes", wide)
    ids = (0, 1, 2)
    _, raw0 = _hand(hdr, oracle, pods, [[_zone(0, 4, ids, pp), _zone(1, 1, ids, pp), _zone(2, 0, ids, pp)]], "LeastNUMANodes", wide)
    assert raw[0, 0] > 0 and raw0[0, 0] == 0


# ------------------------------------------------------------------ the commit loop's row_indirect mode of k_nrt_long
def test_commit_sequential_with_long_rows_and_permuted_ids(gpu_required, hdr, oracle):
    """the per-pod loop over a batch with long rows on nodes whose NUMA ids are permutations of the positions, against the oracle's
    cycle with its Reserve state"""
    snap = _full_long(hdr, 300, 160, 47)
    E.mutate_numa_ids(snap["nrt"], np.random.default_rng(47), "permuted", share=0.7)
    ids, zptr = snap["nrt"].array("zone_numa_id"), snap["nrt"].array("zone_ptr")
    assert (ids != np.arange(len(ids)) - np.repeat(zptr[:-1], np.diff(zptr))).any()
    mask = mask_of(*ALLP)
    with Engine(0) as e:
        _load_full(e, snap)
        assert e.kernel_path(NRT) == 0
        e.set_plugin_weights(WEIGHTS)
        node, score, ties, _ = e.commit_sequential(mask)
        assert e.commit_path() == 2
        alloc_params = e.alloc_params
    want = oracle.commit_sequential(_osnap(oracle, hdr, snap, alloc_params), mask, WEIGHTS, quota=snap["quota"],
                                    bind_ts=int(snap["metrics"].struct.window_end) + 1)
    placed = want["node"] >= 0
    assert np.array_equal(node, want["node"]) and np.array_equal(ties, want["ties"])
    assert np.array_equal(score[placed], want["score"][placed])
    assert 5 < placed.sum() < len(placed)
