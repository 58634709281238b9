"""kernels_nrt_tall.hip where tests/test_gpu_nrt_tall.py does not reach: a wave that walks several (row, tile) items on one working
copy, zones that share a NUMA id, the subset search's two short cuts, and both forms of the per-container request column.  Every cell
against the CPU oracle at tolerance 0, as tests/test_gpu_nrt_tall.py's _check does: status exact, the score table equal to
raw.clip(0, 255), spx_fetch_raw rows equal, two row ranges, the reference kernels.  The examples are tests/nrt_tall_edge_cases.py's,
shown to hold their edges in tests/test_nrt_tall_edges_host.py (where the oracle's subset search is itself compared with a plain
Python reading of the Go source).  The oracle's answer for an example is computed once and shared by the tests that use it."""
import numpy as np
import pytest

import nrt_tall_cases as TC
import nrt_tall_edge_cases as EC
from helpers import NRT
from scheduler_plugins_amd.engine import Engine, mask_of

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(hdr, oracle, key, make, strategy):
    """(case, tables, oracle status, oracle raw scores) of an example, built and evaluated once per session; never written to"""
    if (key, strategy) not in _REF:
        c = make()
        s = TC.build(hdr, c, strategy)
        o = oracle.Snapshot(s["nodes"], s["pods"], rc=s["rc"], nrt=s["nrt"], nrt_params=s["params"])
        th = oracle.usable_cpus()
        st, raw = o.filter_rows(NRT, threads=th), o.score_rows(NRT, want_norm=False, threads=th)[0]
        st.setflags(write=False), raw.setflags(write=False)
        _REF[(key, strategy)] = (c, s, st, raw)
    return _REF[(key, strategy)]


def _check(hdr, oracle, key, make, strategy, raw_rows=None, copies=None):
    """tests/test_gpu_nrt_tall.py's _check on a shared reference: the whole batch, two row ranges that split it, and the reference
    kernels — all equal to the oracle; spx_fetch_raw of some rows; the tall-node count.  `copies`: whether the engine must report
    class copies for the batch (True: the record stream carries it, False: it does not)"""
    c, s, st, raw = _ref(hdr, oracle, key, make, strategy)
    sc = raw.clip(0, 255)
    P, n_tall = len(c["pods"]), TC.n_tall(c)
    with Engine(0) as e:
        e.load_nrt_objects(s["nodes"], s["nrt"], s["rc"], s["pods"], s["params"])
        assert int((e.nrt_soa["nodes"]["n_zones"] == 255).sum()) == n_tall
        if copies is not None:
            assert (e.nrt_pod_classes()[1] > 0) == copies
        e.eval(mask_of(NRT))
        e.sync()
        assert e.nrt_tall_nodes() == n_tall
        assert np.array_equal(e.all_status(NRT), st)
        assert np.array_equal(e.all_scores(NRT).astype(np.int64), sc)
        for r in (range(P) if raw_rows is None else raw_rows):
            assert np.array_equal(e.raw(NRT, int(r) % P), raw[r]), r
        cut = max(1, P // 3)
        for b, en in ((cut, P), (0, cut)):
            e.eval(mask_of(NRT), b, en)
            assert e.nrt_tall_nodes() == n_tall
        e.sync()
        assert np.array_equal(e.all_status(NRT), st) and np.array_equal(e.all_scores(NRT).astype(np.int64), sc)
        e.force_reference_kernels(NRT)
        e.eval(mask_of(NRT))
        e.sync()
        assert e.nrt_tall_nodes() == n_tall
        assert np.array_equal(e.all_status(NRT), st) and np.array_equal(e.all_scores(NRT).astype(np.int64), sc)
    return c, st, raw


# ------------------------------------------------------------------ A. a wave takes a second and a third item
def _assert_reuse(hdr, c, strategy, sharp, begin=0):
    """before anything runs on the GPU: rows x tiles >= 2 x waves + tiles, and every wave has its writer -> reader pair"""
    from test_flatten_nrt_rows import HostOnly
    s = TC.build(hdr, c, strategy)
    f = HostOnly().flatten_nrt(s["nodes"], s["nrt"], s["rc"], s["pods"], s["params"])
    P, n_tall, tiles = len(c["pods"]), int(f["tall"]["n_tall"]), EC.tall_tiles(int(f["tall"]["n_tall"]))
    waves = EC.tall_waves(P - begin, n_tall, int(f["tall"]["zone_stride"]), int(f["R"]))
    assert (P - begin) * tiles >= 2 * waves + tiles, "no wave would take a second item: the constants changed, resize the example"
    pairs = EC.reuse_pairs(c["kinds"], sharp, begin, P, n_tall, waves)
    assert all(pairs)
    return n_tall, tiles, waves, pairs


@pytest.mark.parametrize("strategy", ["LeastAllocated", "BalancedAllocation"])
def test_filter_charges_on_a_reused_copy(gpu_required, hdr, oracle, strategy):
    """about 530 rows x 2 tiles on the 512 waves a 64-zone stride and 4 slots allow: every wave charges its copy for one row and
    must start the next from the table as uploaded"""
    c = _ref(hdr, oracle, "filter-reuse", EC.filter_reuse_case, strategy)[0]
    *_, pairs = _assert_reuse(hdr, c, strategy, EC.FILTER_SHARP)
    _, st, _ = _check(hdr, oracle, "filter-reuse", EC.filter_reuse_case, strategy, raw_rows=pairs[0][0] + pairs[-1][0])
    assert (st == 0).all()


def test_least_numa_subtraction_on_a_reused_copy(gpu_required, hdr, oracle):
    """about 2060 rows x 2 tiles on 2048 waves (a 16-zone stride, 4 slots): LeastNUMANodes' greedy subtraction empties the closest
    pair on a wave's copy, and the next row of that wave needs the pair untouched"""
    c = _ref(hdr, oracle, "ln-reuse", EC.ln_reuse_case, "LeastNUMANodes")[0]
    *_, pairs = _assert_reuse(hdr, c, "LeastNUMANodes", EC.LN_SHARP)
    _, _, raw = _check(hdr, oracle, "ln-reuse", EC.ln_reuse_case, "LeastNUMANodes", raw_rows=pairs[0][0] + pairs[-1][0])
    kinds = np.array(c["kinds"])
    assert (raw[kinds == "emptier"] == 76).all() and (raw[kinds == "reader"] == 82).all()


@pytest.mark.parametrize("key,make,strategy,sharp", [("filter-reuse", EC.filter_reuse_case, "LeastAllocated", EC.FILTER_SHARP),
                                                     ("ln-reuse", EC.ln_reuse_case, "LeastNUMANodes", EC.LN_SHARP)], ids=["filter", "least-numa"])
def test_reuse_under_row_ranges(gpu_required, hdr, oracle, key, make, strategy, sharp):
    """a range that starts at row 3 and still gives every wave two items; eight of its rows alone, one item per wave (no reuse): the
    same bytes; the working-copy buffer sized by the short range and then used by the long one, and the other way round"""
    c, s, st, raw = _ref(hdr, oracle, key, make, strategy)
    sc = raw.clip(0, 255)
    P, begin = len(c["pods"]), 3
    n_tall, tiles, waves, pairs = _assert_reuse(hdr, c, strategy, sharp, begin)
    lo = begin + waves // tiles          # the rows that are second on their wave in the long range
    assert lo + 8 <= P
    with Engine(0) as e:
        f = e.flatten_nrt(s["nodes"], s["nrt"], s["rc"], s["pods"], s["params"])
        e.upload_nrt(f)
        stride, R = int(f["tall"]["zone_stride"]), int(f["R"])   # the grids, from the tables this engine holds
        assert EC.tall_waves(P - begin, n_tall, stride, R) == waves and EC.tall_waves(8, n_tall, stride, R) == 8 * tiles
        for b, en in ((lo, lo + 8), (begin, P), (lo, lo + 8), (0, P)):
            e.eval(mask_of(NRT), b, en)
            e.sync()
            assert e.nrt_tall_nodes() == n_tall
            assert np.array_equal(e.all_status(NRT, b, en), st[b:en]), (b, en)
            assert np.array_equal(e.all_scores(NRT, b, en).astype(np.int64), sc[b:en]), (b, en)
        writer, reader = pairs[5][0]
        assert np.array_equal(e.raw(NRT, writer), raw[writer]) and np.array_equal(e.raw(NRT, reader), raw[reader])


# ------------------------------------------------------------------ B. zones that share a NUMA id
@pytest.mark.parametrize("strategy", TC.NOT_LEAST_NUMA)
@pytest.mark.parametrize("nz", EC.SHARED_ZONES)
def test_shared_ids_filter_and_scores(gpu_required, hdr, oracle, nz, strategy):
    _, st, _ = _check(hdr, oracle, f"shared-filter-{nz}", lambda: EC.shared_filter_case(nz), strategy)
    C = TC.ST["container"]
    assert st[:5, :3].tolist() == [[0, 0, 0], [C, 0, 0], [C, 0, 0], [C, C, 0], [0, 0, 0]]
    assert (st[:5, 3] == 255).all()    # uneven twins: one of them is charged below zero, the reference's fwk.Error


@pytest.mark.parametrize("nz", [9, 16])
def test_shared_ids_filter_least_numa(gpu_required, hdr, oracle, nz):
    _, st, _ = _check(hdr, oracle, f"shared-filter-{nz}", lambda: EC.shared_filter_case(nz), "LeastNUMANodes")
    assert np.array_equal(st, _ref(hdr, oracle, f"shared-filter-{nz}", lambda: EC.shared_filter_case(nz), "LeastAllocated")[2])


@pytest.mark.parametrize("policy", [TC.POD, TC.CONTAINER], ids=["pod-scope", "container-scope"])
@pytest.mark.parametrize("nz", [9, 16])
def test_shared_ids_least_numa(gpu_required, hdr, oracle, nz, policy):
    """the count is of distinct ids: a pair of twins scores as one NUMA node; in container scope the subtraction takes ids as positions"""
    _, _, raw = _check(hdr, oracle, f"shared-ln-{nz}-{policy}", lambda: EC.shared_ln_pod_case(nz, policy), "LeastNUMANodes")
    assert raw[1, 0] == 94 and raw[1, 1] == 82
    if policy == TC.CONTAINER:
        assert raw[6, 0] > 0 and raw[6, 1] == 0


# ------------------------------------------------------------------ C. the subset search's short cuts
def test_subset_search_pod_scope(gpu_required, hdr, oracle):
    c, _, raw = _check(hdr, oracle, "subset", EC.subset_case, "LeastNUMANodes", raw_rows=range(0, 130, 9))
    assert (raw[:, c["negative_node"]] > 0).any()


def test_subset_search_container_scope(gpu_required, hdr, oracle):
    _check(hdr, oracle, "subset-container", lambda: EC.two_container_pods(EC.subset_case(policy=TC.CONTAINER)), "LeastNUMANodes",
           raw_rows=range(0, 130, 9))


# ------------------------------------------------------------------ D. both forms of the per-container request column
@pytest.mark.parametrize("name", sorted(EC.FORMS))
def test_request_column_rebuilt_and_shipped(gpu_required, hdr, oracle, name):
    """the kernel reads the dense per-container request column.  A batch the record stream carries does not ship it: the engine
    rebuilds it from the stream's doubles (and reports class copies for the repeated row).  One more row with a quantity the stream
    refuses, and the column is shipped as flattened (and no copies are reported).  Both against the oracle, the extra row's cells too"""
    make, strategy = EC.FORMS[name]
    rows = (0, -2, -1)
    c, st, raw = _check(hdr, oracle, f"form-stream-{name}", lambda: EC.with_copy_row(make()), strategy, raw_rows=rows, copies=True)
    c2, st2, raw2 = _check(hdr, oracle, f"form-column-{name}", lambda: EC.with_unstreamable_row(EC.with_copy_row(make())), strategy, raw_rows=rows,
                           copies=False)
    assert np.array_equal(st2[:-1], st) and np.array_equal(raw2[:-1], raw) and (st2[-1] != 0).any()
