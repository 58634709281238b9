"""The dense NodeResourceTopologyMatch kernels (k_nrt, k_nrt_long) and the wide one (k_nrt_wide) on nodes of at most eight zones that
list one NUMA id twice or more: the charge to every carrier of the id, its undo, the fwk.Error of uneven twins as status 255
(SPX_NRT_ST_ERROR), LeastNUMANodes' count of distinct ids and its subtraction by list position, ids packed across positions 3 and 4.
Every cell against the CPU oracle at tolerance 0: status exact, the score table equal to raw.clip(0, 255), spx_fetch_raw rows equal.
The examples are tests/nrt_dense_twin_cases.py's, shown to hold their edges in tests/test_nrt_dense_twins_host.py (where the oracle
is itself compared with two plain Python readings of the Go source).  The oracle's answer for an example is computed once and shared.

The float64, rank-space and fused launches require ids equal to positions; what is asserted about them here is that the engine does
not run them on such a snapshot."""
import numpy as np
import pytest

import nrt_dense_twin_cases as DC
import nrt_tall_cases as TC
from helpers import ALLOCATABLE, NRT
from scheduler_plugins_amd.engine import Engine, mask_of
from test_gpu_nrt_long import ALLP, WEIGHTS, _load_full, _osnap

pytestmark = pytest.mark.gpu

ERROR = DC.ERROR
_REF = {}
EXAMPLES = DC.examples()


def _ref(hdr, oracle, name, strategy, slots=4, longest=65):
    """(case, tables, oracle status, oracle raw scores), built and evaluated once per session; never written to"""
    key = (name, strategy, slots, longest)
    if key not in _REF:
        if name.startswith("uneven") and longest != 65:
            c = DC.uneven_case(int(name.rsplit("-", 1)[1]), sparse="sparse" in name, longest=longest)
        else:
            c = EXAMPLES[name][0]()
        c = DC.with_slots(c, slots)
        s = TC.build(hdr, c, strategy)
        o = oracle.Snapshot(s["nodes"], s["pods"], rc=s["rc"], nrt=s["nrt"], nrt_params=s["params"])
        th = oracle.usable_cpus()
        st, raw = o.filter_rows(NRT, threads=th), o.score_rows(NRT, want_norm=False, threads=th)[0]
        st.setflags(write=False), raw.setflags(write=False)
        _REF[key] = (c, s, st, raw)
    return _REF[key]


def _load(e, s):
    e.load_nrt_objects(s["nodes"], s["nrt"], s["rc"], s["pods"], s["params"])


def _equal(e, st, raw, tag, b=0, en=None):
    got_st, got_sc = e.all_status(NRT, b, en), e.all_scores(NRT, b, en).astype(np.int64)
    bad = np.argwhere(got_st != st[b:en])
    assert bad.size == 0, ("status", tag, len(bad), [(int(p) + b, int(n), int(got_st[p, n]), int(st[b:en][p, n])) for p, n in bad[:6]])
    bad = np.argwhere(got_sc != raw[b:en].clip(0, 255))
    assert bad.size == 0, ("score", tag, len(bad), [(int(p) + b, int(n), int(got_sc[p, n]), int(raw[b:en][p, n])) for p, n in bad[:6]])


def _sweep(e, c, st, raw, tag, wide):
    """the whole batch, spx_fetch_raw of every row, two row ranges whose cut follows an Error row, the reference kernels"""
    P = len(c["pods"])
    n_long = 0 if wide else sum(len(p["containers"]) + len(p["init_containers"]) > 8 for p in c["pods"])
    e.eval(mask_of(NRT))
    e.sync()
    assert e.nrt_wide() == wide and e.nrt_filter_path() == (4 if wide else 1) and e.nrt_long_rows() == n_long, tag
    if not wide:
        assert e.kernel_path(NRT) == 0, tag          # ids are not positions: the reference-arithmetic sweep, not a fast form
    _equal(e, st, raw, tag)
    for r in range(P):
        assert np.array_equal(e.raw(NRT, r), raw[r]), (tag, r)
    cut = 1 if P < 3 else P // 3 | 1                 # odd: in the uneven examples the upper range starts at a reader
    for b, en in ((cut, P), (0, cut)):
        e.eval(mask_of(NRT), b, en)
        e.sync()
        _equal(e, st, raw, (tag, b, en), b, en)
    _equal(e, st, raw, (tag, "ranges"))
    if not wide:
        e.force_reference_kernels(NRT)
        e.eval(mask_of(NRT))
        e.sync()
        _equal(e, st, raw, (tag, "reference kernels"))
        e.force_reference_kernels()


# ------------------------------------------------------------------ the dense route: k_nrt, and k_nrt_long on rows of 9 and 65 containers
@pytest.mark.parametrize("name", sorted(EXAMPLES))
def test_dense_route(gpu_required, hdr, oracle, name):
    with Engine(0) as e:
        for strategy in EXAMPLES[name][1]:
            c, s, st, raw = _ref(hdr, oracle, name, strategy)
            _load(e, s)
            _sweep(e, c, st, raw, (name, strategy), wide=False)
    if name.startswith("uneven"):
        assert (st == ERROR).any() and sum(len(p["containers"]) in (9, 65) for p in c["pods"]) == 2


SIX = ["uneven-sparse-5", "uneven-8", "even-sparse-8", "quiet-4", "least-numa-container-5"]


@pytest.mark.parametrize("name", SIX)
def test_dense_route_six_slots(gpu_required, hdr, oracle, name):
    with Engine(0) as e:
        for strategy in EXAMPLES[name][1]:
            c, s, st, raw = _ref(hdr, oracle, name, strategy, slots=6)
            _load(e, s)
            assert e.flatten_nrt(s["nodes"], s["nrt"], s["rc"], s["pods"], s["params"])["R"] == 6
            _sweep(e, c, st, raw, (name, strategy, 6), wide=False)


@pytest.mark.parametrize("option", ["NRT_RANK_FILTER", "NRT_FUSED"])
@pytest.mark.parametrize("strategy", ["LeastAllocated", "BalancedAllocation"])
def test_one_twin_node_keeps_the_batch_off_the_rank_space_launches(gpu_required, hdr, oracle, option, strategy):
    """70 nodes of one shape, one of them with paired ids: with the rank-space Filter asked for, alone and inside the fused launch,
    the sweep reports the float64-compare path (1), runs the reference-arithmetic kernel, and the twin column holds the oracle's
    cells, the Error among them"""
    c, s, st, raw = _ref(hdr, oracle, "mixed", strategy)
    with Engine(0) as e:
        e.set_option("NRT_RANK_FILTER", 1)
        e.set_option("NRT_FUSED", 1 if option == "NRT_FUSED" else 0)
        _load(e, s)
        e.eval(mask_of(NRT))
        e.sync()
        assert e.nrt_filter_path() == 1 and e.kernel_path(NRT) == 0
        _equal(e, st, raw, (option, strategy))
        assert (e.all_status(NRT)[:, c["twin_col"]] == ERROR).any()


# ------------------------------------------------------------------ the wide route: k_nrt_wide
WIDE = ["uneven-sparse-5", "uneven-sparse-8", "uneven-8", "even-sparse-4", "quiet-3", "least-numa-container-5", "least-numa-8"]


@pytest.mark.parametrize("slots", [9, 12])
@pytest.mark.parametrize("name", WIDE)
def test_wide_route(gpu_required, hdr, oracle, name, slots):
    with Engine(0) as e:
        for strategy in EXAMPLES[name][1]:
            c, s, st, raw = _ref(hdr, oracle, name, strategy, slots=slots, longest=64)
            _load(e, s)
            _sweep(e, c, st, raw, (name, strategy, slots), wide=True)
    if name.startswith("uneven"):
        assert (st == ERROR).any() and max(len(p["containers"]) for p in c["pods"]) == 64


@pytest.mark.parametrize("slots", [4, 6])
@pytest.mark.parametrize("name", ["uneven-sparse-5", "uneven-4", "quiet-8"])
def test_wide_tables_on_few_slots_equal_the_dense_route(gpu_required, hdr, oracle, name, slots):
    for strategy in EXAMPLES[name][1]:
        c, s, st, raw = _ref(hdr, oracle, name, strategy, slots=slots, longest=64)
        with Engine(0) as e:
            _load(e, s)
            e.eval(mask_of(NRT))
            e.sync()
            assert not e.nrt_wide() and e.nrt_long_rows() == 2 * name.startswith("uneven")
            dense = e.all_status(NRT), e.all_scores(NRT)
            _equal(e, st, raw, (name, strategy, slots, "dense"))
        with Engine(0) as e:
            e.set_option("NRT_WIDE", 1)
            _load(e, s)
            _sweep(e, c, st, raw, (name, strategy, slots, "wide"), wide=True)
            assert np.array_equal(e.all_status(NRT), dense[0]) and np.array_equal(e.all_scores(NRT), dense[1])


# ------------------------------------------------------------------ state: a row delta that makes twins, and one that takes them back
def test_node_update_to_uneven_twins_and_back(gpu_required, hdr, oracle):
    """the mixed example without its twin (every node position ids), then spx_update_nrt_nodes of the one column to paired ids, then
    back: each equal to a full upload of that snapshot, and to the oracle"""
    c, s, st, raw = _ref(hdr, oracle, "mixed", "LeastAllocated")
    col = c["twin_col"]
    plain = dict(c, nrts=[c["nrts"][0] if i == col else t for i, t in enumerate(c["nrts"])])
    sp = TC.build(hdr, plain, "LeastAllocated")
    o = oracle.Snapshot(sp["nodes"], sp["pods"], rc=sp["rc"], nrt=sp["nrt"], nrt_params=sp["params"])
    st0, raw0 = o.filter_rows(NRT), o.score_rows(NRT, want_norm=False)[0]
    assert not (st0 == ERROR).any() and (st[:, col] == ERROR).any()
    with Engine(0) as e:
        f0 = e.flatten_nrt(sp["nodes"], sp["nrt"], sp["rc"], sp["pods"], sp["params"])
        f1 = e.flatten_nrt(s["nodes"], s["nrt"], s["rc"], s["pods"], s["params"])
        e.upload_nrt(f0)
        for f, want_st, want_raw, tag in ((f0, st0, raw0, "uploaded"), (f1, st, raw, "to twins"), (f0, st0, raw0, "back"), (f1, st, raw, "again")):
            if tag != "uploaded":
                e.update_nrt_nodes([col], f)
            e.eval(mask_of(NRT))
            e.sync()
            _equal(e, want_st, want_raw, tag)
            delta = e.all_status(NRT), e.all_scores(NRT)
            with Engine(0) as full:
                full.upload_nrt(f)
                full.eval(mask_of(NRT))
                full.sync()
                assert np.array_equal(full.all_status(NRT), delta[0]) and np.array_equal(full.all_scores(NRT), delta[1]), tag


# ------------------------------------------------------------------ downstream of the status table
@pytest.fixture(scope="module")
def profile(hdr):
    snap, twins = DC.twin_profile(hdr, 130, 60, seed=1, share=0.9)
    return snap, twins


def _would_win(o, st):
    """rows whose best weighted score sits on an Error node when the Error is read as a pass: every Score plugin normalised over
    the nodes that pass or raise the Error"""
    from helpers import LVRB, NETOVERHEAD, TLP
    net = o.filter_rows(NETOVERHEAD)
    soft = ((st == 0) | (st == ERROR)) & (net == 0)
    tot = sum(WEIGHTS[p] * o.score_rows(p, want_norm=False)[0].clip(0, 255) for p in (TLP, LVRB, NRT)).astype(np.int64)
    tot += WEIGHTS[NETOVERHEAD] * o.score_rows(NETOVERHEAD, mask=((st == 0) | (st == ERROR)).astype(np.uint8), want_raw=False)[1]
    tot += WEIGHTS[ALLOCATABLE] * o.score_rows(ALLOCATABLE, mask=soft.astype(np.uint8), want_raw=False)[1]
    tot[~soft] = -1
    best = tot.argmax(axis=1)
    return [r for r in range(len(best)) if st[r, best[r]] == ERROR]


def test_decide_does_not_choose_an_error_node(gpu_required, hdr, oracle, profile):
    snap, twins = profile
    mask = mask_of(*ALLP)
    with Engine(0) as e:
        _load_full(e, snap)
        e.set_plugin_weights(WEIGHTS)
        assert e.kernel_path(NRT) == 0
        e.decide(mask)
        e.sync()
        got = e.best()
        e.eval(mask)
        e.sync()
        status = e.all_status(NRT)
        alloc_params = e.alloc_params
    osnap = _osnap(oracle, hdr, snap, alloc_params)
    st = osnap.filter_rows(NRT)
    assert np.array_equal(status, st) and (st == ERROR).sum() > 100
    tempted, placed = _would_win(osnap, st), 0
    for r in range(60):
        want = oracle.commit_sequential(osnap, mask, WEIGHTS, quota=snap["quota"], row_begin=r, row_end=r + 1,
                                        bind_ts=int(snap["metrics"].struct.window_end) + 1)
        assert got[0][r] == want["node"][0], r
        if want["node"][0] >= 0:
            assert got[1][r] == want["score"][0] and got[2][r] == want["ties"][0], r
            assert st[r, got[0][r]] == 0, r
            placed += r in tempted
    assert placed >= 3, (tempted, placed)    # rows that are decided, and on which reading 255 as a pass would have chosen an Error node


def test_allocatable_normalises_without_the_error_nodes(gpu_required, hdr, oracle, profile):
    """spx_eval of Allocatable with NRT: the feasible set NormalizeScore takes lo and hi over leaves the Error cells out"""
    snap, _ = profile
    with Engine(0) as e:
        e.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])
        e.load_nrt_objects(snap["nodes"], snap["nrt"], snap["rc"], snap["pods"], snap["nrt_params"])
        e.eval(mask_of(ALLOCATABLE, NRT))
        e.sync()
        got, status = e.all_scores(ALLOCATABLE).astype(np.int64), e.all_status(NRT)
        alloc_params = e.alloc_params
    osnap = _osnap(oracle, hdr, snap, alloc_params)
    st = osnap.filter_rows(NRT)
    assert np.array_equal(status, st)
    want = osnap.score_rows(ALLOCATABLE, mask=(st == 0).astype(np.uint8), want_raw=False)[1]
    soft = osnap.score_rows(ALLOCATABLE, mask=((st == 0) | (st == ERROR)).astype(np.uint8), want_raw=False)[1]
    feasible = st == 0
    assert np.array_equal(got[feasible], want[feasible])
    assert (want[feasible] != soft[feasible]).any()      # reading the Error as a pass moves lo or hi of some row


def test_commit_sequential_on_a_snapshot_with_error_cells(gpu_required, hdr, oracle, profile):
    """the per-pod loop (k_nrt on one row at a time) against the oracle's cycle with its Reserve state"""
    snap, twins = profile
    mask = mask_of(*ALLP)
    with Engine(0) as e:
        _load_full(e, snap)
        e.set_plugin_weights(WEIGHTS)
        node, score, ties, _ = e.commit_sequential(mask)
        assert e.commit_path() == 2
        alloc_params = e.alloc_params
    osnap = _osnap(oracle, hdr, snap, alloc_params)
    want = oracle.commit_sequential(osnap, mask, WEIGHTS, quota=snap["quota"], bind_ts=int(snap["metrics"].struct.window_end) + 1)
    placed = want["node"] >= 0
    assert np.array_equal(node, want["node"]) and np.array_equal(ties, want["ties"])
    assert np.array_equal(score[placed], want["score"][placed])
    assert placed.sum() > 5 and np.isin(want["node"][placed], twins).any()


def test_one_device_multi_engine(gpu_required, hdr, oracle):
    from scheduler_plugins_amd.multi import PEER_COPY, MultiEngine
    c, s, st, raw = _ref(hdr, oracle, "uneven-sparse-5", "LeastAllocated")
    with MultiEngine([0], PEER_COPY) as m:
        m.load_nrt_objects(s["nodes"], s["nrt"], s["rc"], s["pods"], s["params"])
        m.bind_global_table(NRT)
        m.bind_global_table(NRT, status=True)
        m.eval(mask_of(NRT))
        m.allgather_table(NRT)
        m.allgather_table(NRT, status=True)
        m.sync()
        assert np.array_equal(m.global_rows(NRT, 0, status=True), st)
        assert np.array_equal(m.global_rows(NRT, 0).astype(np.int64), raw.clip(0, 255))
