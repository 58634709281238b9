"""NodeResourceTopologyMatch on the GPU for snapshots with more than eight resource slots (the wide tables, kernels_nrt_wide.hip).
Every cell against the CPU oracle, which takes up to 32 resources per list: status exact, raw score with tolerance 0.  With
SPX_OPT_NRT_WIDE the wide kernel also runs on snapshots of 8 or fewer slots, byte-equal to the dense sweeps."""
import numpy as np
import pytest

from helpers import ALLOCATABLE, CAPACITY, LVRB, NETOVERHEAD, NRT, TLP, lvrb_params, tlp_params
from scheduler_plugins_amd import SpxError
from scheduler_plugins_amd import objects as O
from scheduler_plugins_amd import synth
from scheduler_plugins_amd.engine import Engine, mask_of

pytestmark = pytest.mark.gpu

STRATEGIES = ["LeastAllocated", "MostAllocated", "BalancedAllocation", "LeastNUMANodes"]
ST = {"container": 4, "pod": 5}
POOLS = [f"example.com/pool{k}" for k in range(9)]  # extended resources: with cpu and memory, 11 slots; pool8 is slot 10


def _want(oracle, nodes, pods, rc, nrts, params, b=0, e=None):
    osnap = oracle.Snapshot(nodes, pods, rc=rc, nrt=nrts, nrt_params=params)
    th = oracle.usable_cpus()
    return osnap.filter_rows(NRT, b, e, threads=th), osnap.score_rows(NRT, b, e, want_norm=False, threads=th)[0]


def _check(e, oracle, nodes, pods, rc, nrts, params):
    st, raw = _want(oracle, nodes, pods, rc, nrts, params)
    assert np.array_equal(e.all_status(NRT), st)
    assert np.array_equal(e.all_scores(NRT).astype(np.int64), raw.clip(0, 255))
    return st, raw


# ------------------------------------------------------------------ hand-built cases
def _zone(i, pools, extra=None):
    r = {"cpu": "8", "memory": "64Gi"}
    r.update({name: str(q) for name, q in zip(POOLS, pools)})
    r.update(extra or {})
    return {"name": f"node-{i}", "type": "Node", "resources": r, "costs": {f"node-{j}": (10 if j == i else 20) for j in range(2)}}


def _g(extra=None, cpu="1", mem="1Gi"):  # a Guaranteed container
    rl = {"cpu": cpu, "memory": mem}
    rl.update(extra or {})
    return O.container(rl, dict(rl))


def _hand_case(hdr, oracle, pods_spec, zones_per_node, policy, strategy="LeastAllocated", alloc_extra=None, res=None):
    """one node per entry of zones_per_node; alloc_extra[i]: node i's extra allocatable (default: every pool)"""
    res = res or O.Resources()
    for name in POOLS:
        res.id(name)
    pods = O.build_pod_objects(hdr, res, pods_spec)
    nrts = O.build_nrt_objects(hdr, res, [O.nrt(z, [policy]) for z in zones_per_node])
    node_specs = []
    for i in range(len(zones_per_node)):
        tot = {"cpu": "16", "memory": "512Gi"}
        tot.update((alloc_extra[i] if alloc_extra else {name: "64" for name in POOLS}))
        node_specs.append(O.node(tot, tot))
    nodes = O.build_node_objects(hdr, res, node_specs)
    params = O.nrt_params(hdr, res, strategy)
    with Engine(0) as e:
        e.load_nrt_objects(nodes, nrts, res.table(hdr), pods, params)
        assert e.nrt_wide()
        e.eval(mask_of(NRT))
        e.sync()
        assert e.nrt_filter_path() == 4 and e.nrt_long_rows() == 0
        return _check(e, oracle, nodes, pods, res.table(hdr), nrts, params)


@pytest.mark.parametrize("policy", ["SingleNUMANodeContainerLevel", "SingleNUMANodePodLevel"])
def test_slot_ten_pool_fits_one_zone(gpu_required, hdr, oracle, policy):
    """the only unmet request is slot 10 (pool8): 3 fit zone 1 only, 4 fit no zone"""
    zones = [_zone(0, [4] * 8 + [1]), _zone(1, [4] * 8 + [3])]
    pods = [O.pod([_g({POOLS[8]: "3"})]), O.pod([_g({POOLS[8]: "4"})]), O.pod([_g({POOLS[0]: "2"})])]
    st, _ = _hand_case(hdr, oracle, pods, [zones], policy)
    fail = ST["pod"] if policy.endswith("PodLevel") else ST["container"]
    assert st[:, 0].tolist() == [0, fail, 0]


def test_slot_ten_not_reported_at_node_level(gpu_required, hdr, oracle):
    """node 1's allocatable lacks pool8: a request for it cannot be met there whatever the zones hold (filter.go:110-116)"""
    zones = [_zone(0, [4] * 9), _zone(1, [4] * 9)]
    alloc = [{name: "64" for name in POOLS}, {name: "64" for name in POOLS[:8]}]
    st, _ = _hand_case(hdr, oracle, [O.pod([_g({POOLS[8]: "1"})]), O.pod([_g({POOLS[1]: "1"})])], [zones, zones],
                       "SingleNUMANodeContainerLevel", alloc_extra=alloc)
    assert st[0].tolist() == [0, ST["container"]] and st[1].tolist() == [0, 0]


def test_host_level_slot_beyond_eight(gpu_required, hdr, oracle):
    """an extended resource no zone reports is host-level without NUMA affinity: skipped by the zone check, still checked at node level"""
    res = O.Resources()
    zones = [_zone(0, [4] * 9), _zone(1, [4] * 9)]
    for name in POOLS:
        res.id(name)
    res.id("example.com/host-only")
    alloc = [dict({name: "64" for name in POOLS}, **{"example.com/host-only": "5"}), {name: "64" for name in POOLS}]
    st, _ = _hand_case(hdr, oracle, [O.pod([_g({"example.com/host-only": "3", POOLS[8]: "1"})])], [zones, zones],
                       "SingleNUMANodeContainerLevel", alloc_extra=alloc, res=res)
    assert st[0].tolist() == [0, ST["container"]]


def test_non_guaranteed_affine_slot_beyond_eight_is_skipped(gpu_required, hdr, oracle):
    """hugepages-1Gi (slot >= 9, NUMA-affine): a Burstable pod's request is suitable in any zone (isResourceSetSuitable), a Guaranteed
    pod's must fit"""
    res = O.Resources()
    for name in POOLS:
        res.id(name)
    res.id("hugepages-1Gi")
    zones = [_zone(0, [4] * 9, {"hugepages-1Gi": "2Gi"}), _zone(1, [4] * 9, {"hugepages-1Gi": "2Gi"})]
    alloc = [dict({name: "64" for name in POOLS}, **{"hugepages-1Gi": "64Gi"})]
    burst = O.container({"cpu": "1", "memory": "1Gi", "hugepages-1Gi": "8Gi"}, {"cpu": "2", "memory": "1Gi", "hugepages-1Gi": "8Gi"})
    st, raw = _hand_case(hdr, oracle, [O.pod([burst]), O.pod([_g({"hugepages-1Gi": "8Gi"})])], [zones], "SingleNUMANodeContainerLevel",
                         alloc_extra=alloc, res=res)
    assert st[:, 0].tolist() == [0, ST["container"]] and raw[0, 0] == 100


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_twelve_containers_in_a_wide_snapshot(gpu_required, hdr, oracle, strategy):
    """twelve app containers of one pool8 unit each fill 6 + 6; a thirteenth finds no zone (container scope charges each)"""
    zones = [_zone(0, [4] * 8 + [6]), _zone(1, [4] * 8 + [6])]
    ctr = _g({POOLS[8]: "1", POOLS[3]: "0"}, cpu="500m", mem="1Gi")
    st, _ = _hand_case(hdr, oracle, [O.pod([ctr] * 12), O.pod([ctr] * 13), O.pod([ctr] * 5, [_g({POOLS[8]: "6"})])], [zones],
                       "SingleNUMANodeContainerLevel", strategy)
    assert st[:, 0].tolist() == [0, ST["container"], 0]


# ------------------------------------------------------------------ seeded snapshots
_SNAPS = {}


def _wide_snap(hdr, extra):
    if extra not in _SNAPS:
        _SNAPS[extra] = synth.nrt_snapshot(hdr, 2000, 4000, seed=50 + extra, long_frac=0.01, long_ctrs=(9, 20), extra_res=extra)
    return _SNAPS[extra]


@pytest.mark.parametrize("extra,n_res", [(5, 9), (8, 12), (28, 32)])
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_seeded_wide_snapshot_every_cell(gpu_required, hdr, oracle, extra, n_res, strategy):
    s = _wide_snap(hdr, extra)
    params = O.nrt_params(hdr, O.Resources(), strategy)
    want_st, want_raw = _want(oracle, s["nodes"], s["pods"], s["rc"], s["nrt"], params)
    with Engine(0) as e:
        e.load_c(s, params)  # spx_load_nrt: the wide route by itself
        assert e.nrt_wide()
        e.eval(mask_of(NRT))
        e.sync()
        assert e.nrt_filter_path() == 4 and e.nrt_long_rows() == 0
        assert np.array_equal(e.all_status(NRT), want_st)
        assert np.array_equal(e.all_scores(NRT).astype(np.int64), want_raw.clip(0, 255))
        # the extra slots decide cells: some pass, some fail, and requests beyond slot 8 are present
        assert (want_st != 0).any() and (want_st == 0).any()
        if strategy == "LeastAllocated":
            f = e.flatten_nrt(s["nodes"], s["nrt"], s["rc"], s["pods"], params)
            assert f["R"] == n_res and (f["pods"]["ent_slot"] >= 8).any()


def test_seeded_wide_ranges_raw_and_reference_option(gpu_required, hdr, oracle):
    s = _wide_snap(hdr, 8)
    params = O.nrt_params(hdr, O.Resources(), "BalancedAllocation")
    want_st, want_raw = _want(oracle, s["nodes"], s["pods"], s["rc"], s["nrt"], params)
    with Engine(0) as e:
        e.load_nrt_objects(s["nodes"], s["nrt"], s["rc"], s["pods"], params)
        assert e.nrt_wide()
        for b, en in [(0, 1333), (1333, 1334), (1334, 4000)]:
            e.eval(mask_of(NRT), b, en)
        e.sync()
        assert np.array_equal(e.all_status(NRT), want_st)
        assert np.array_equal(e.all_scores(NRT).astype(np.int64), want_raw.clip(0, 255))
        for r in range(0, 4000, 397):
            assert np.array_equal(e.raw(NRT, r), want_raw[r]), r
        e.force_reference_kernels(NRT)
        e.eval(mask_of(NRT))
        e.sync()
        assert np.array_equal(e.all_status(NRT), want_st)
        assert np.array_equal(e.all_scores(NRT).astype(np.int64), want_raw.clip(0, 255))


def test_too_many_slots_refused(gpu_required, hdr):
    s = synth.nrt_snapshot(hdr, 200, 300, seed=9, extra_res=29)
    with Engine(0) as e:
        with pytest.raises(SpxError) as err:
            e.load_c(s, O.nrt_params(hdr, O.Resources(), "LeastAllocated"))
        assert err.value.code == -1 and "33" in err.value.msg


# ------------------------------------------------------------------ the option on dense-sized snapshots, mode switches
@pytest.fixture(scope="module")
def dense_snaps(hdr):
    return {w: synth.nrt_snapshot(hdr, 1250, 12500, seed=61, wide=w) for w in (False, True)}


@pytest.mark.parametrize("wide6", [False, True], ids=["4slots", "6slots"])
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_wide_option_byte_equal_to_dense(gpu_required, hdr, dense_snaps, wide6, strategy):
    s = dense_snaps[wide6]
    params = O.nrt_params(hdr, O.Resources(), strategy)
    with Engine(0) as e:
        e.load_c(s, params)
        assert not e.nrt_wide()
        e.eval(mask_of(NRT))
        e.sync()
        st, sc = e.all_status(NRT), e.all_scores(NRT)
    with Engine(0) as e:
        e.set_option("NRT_WIDE", 1)
        e.load_c(s, params)
        assert e.nrt_wide()
        e.eval(mask_of(NRT))
        e.sync()
        assert e.nrt_filter_path() == 4
        assert np.array_equal(e.all_status(NRT), st) and np.array_equal(e.all_scores(NRT), sc)


def test_dense_wide_dense_on_one_engine(gpu_required, hdr, dense_snaps):
    """every step byte-equal to a fresh engine: a wide load leaves nothing of the dense state behind, nor the other way round"""
    params = O.nrt_params(hdr, O.Resources(), "LeastAllocated")
    dense, wide = dense_snaps[False], synth.nrt_snapshot(hdr, 1250, 12500, seed=61, extra_res=6)

    def fresh(s):
        with Engine(0) as f:
            f.load_c(s, params)
            f.eval(mask_of(NRT))
            f.sync()
            return f.all_status(NRT), f.all_scores(NRT)

    with Engine(0) as e:
        for s, is_wide in ((dense, False), (wide, True), (dense, False)):
            e.load_c(s, params)
            assert e.nrt_wide() == is_wide
            e.eval(mask_of(NRT))
            e.sync()
            assert (e.nrt_filter_path() == 4) == is_wide
            st, sc = fresh(s)
            assert np.array_equal(e.all_status(NRT), st) and np.array_equal(e.all_scores(NRT), sc)


def test_commit_and_delta_refused_on_a_wide_engine(gpu_required, hdr):
    s = synth.widen_snapshot(hdr, synth.full_snapshot(hdr, 300, 160, seed=71), 6, seed=71, req_frac=0.0)
    params = O.nrt_params(hdr, O.Resources(), "LeastAllocated")
    with Engine(0) as e:
        e.load_c(s, params)
        assert e.nrt_wide()
        with pytest.raises(SpxError) as err:
            e.commit_sequential(mask_of(ALLOCATABLE, NRT))
        assert err.value.code == -3 and "wide" in err.value.msg
        f = e.flatten_nrt(s["nodes"], s["nrt"], s["rc"], s["pods"], params)
        with pytest.raises(SpxError) as err:
            e.update_nrt_nodes([0], f)
        assert err.value.code == -3 and "wide" in err.value.msg
        # the rest of the commit loop is untouched
        e.commit_sequential(mask_of(ALLOCATABLE))


# ------------------------------------------------------------------ profiles: decide, load_profile, shards
ALLP = (ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD, CAPACITY)
WEIGHTS = {ALLOCATABLE: 1, TLP: 2, LVRB: 1, NRT: 3, NETOVERHEAD: 2}


def _full_wide(hdr, n_nodes, n_pods, seed):
    """the full profile with seven more resources in the zones and node allocatables (12 NRT slots).  The pods keep their requests:
    CapacityScheduling's quota table names at most four scalar resources (the every-cell tests above request the extra ones)"""
    snap = synth.widen_snapshot(hdr, synth.full_snapshot(hdr, n_nodes, n_pods, seed=seed), 7, seed=seed, req_frac=0.0)
    snap["nrt_params"] = O.nrt_params(hdr, O.Resources(), "LeastAllocated")
    return snap


@pytest.mark.parametrize("concurrent", [False, True], ids=["loaders", "load_profile"])
def test_decide_full_profile_with_wide_nrt(gpu_required, hdr, oracle, concurrent):
    """spx_decide over the full profile (NRT next to NetworkOverhead, Allocatable and CapacityScheduling): each pod's decision equals
    the oracle's cycle run for that pod alone"""
    snap = _full_wide(hdr, 400, 300, 81)
    mask = mask_of(*ALLP)
    with Engine(0) as e:
        e.load_c(snap, snap["nrt_params"], concurrent=concurrent)
        assert e.nrt_wide()
        e.set_plugin_weights(WEIGHTS)
        e.decide(mask)
        e.sync()
        got = e.best()
        alloc_params = e.alloc_params
    osnap = oracle.Snapshot(snap["nodes"], snap["pods"], rc=snap["rc"], metrics=snap["metrics"], assigned=snap["assigned"],
                            alloc_params=alloc_params, tlp_params=tlp_params(hdr), lvrb_params=lvrb_params(hdr), nrt=snap["nrt"],
                            nrt_params=snap["nrt_params"], appgroups=snap["appgroups"], nettopo=snap["nettopo"])
    placed = 0
    for r in range(0, 300, 3):
        want = oracle.commit_sequential(osnap, mask, WEIGHTS, quota=snap["quota"], row_begin=r, row_end=r + 1,
                                        bind_ts=int(snap["metrics"].struct.window_end) + 1)
        assert got[0][r] == want["node"][0], r
        if want["node"][0] >= 0:
            placed += 1
            assert got[1][r] == want["score"][0] and got[2][r] == want["ties"][0], r
    assert placed > 5


def test_multi_engine_shards_wide(gpu_required, hdr):
    """two shards on one device: the gathered NRT tables equal the unsharded run"""
    from scheduler_plugins_amd.multi import PEER_COPY, MultiEngine
    snap = synth.nrt_snapshot(hdr, 700, 600, seed=45, extra_res=7, long_frac=0.02, long_ctrs=(9, 12))
    params = O.nrt_params(hdr, O.Resources(), "MostAllocated")
    with Engine(0) as e:
        e.load_nrt_objects(snap["nodes"], snap["nrt"], snap["rc"], snap["pods"], params)
        assert e.nrt_wide()
        e.eval(mask_of(NRT))
        e.sync()
        want_st, want_sc = e.all_status(NRT), e.all_scores(NRT)
    with MultiEngine([0, 0], PEER_COPY) as m:
        m.load_nrt_objects(snap["nodes"], snap["nrt"], snap["rc"], snap["pods"], params)
        assert all(x.nrt_wide() for x in m.engines)
        m.bind_global_table(NRT)
        m.bind_global_table(NRT, status=True)
        m.eval(mask_of(NRT))
        m.allgather_table(NRT)
        m.allgather_table(NRT, status=True)
        m.sync()
        for rank in range(2):
            assert np.array_equal(m.global_rows(NRT, rank, status=True), want_st), rank
            assert np.array_equal(m.global_rows(NRT, rank), want_sc), rank
