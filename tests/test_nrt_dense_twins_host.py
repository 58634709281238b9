"""The examples of tests/nrt_dense_twin_cases.py hold the edges they are built for — shown with the CPU oracle alone, with
tests/nrt_filter_ref.py (a plain Python reading of filter.go and numaresources.go the oracle's status is compared with on every cell)
and with tests/nrt_tall_ref.py (LeastNUMANodes' subset search, compared with the oracle's raw scores) — so that
tests/test_gpu_nrt_dense_twins.py compares the GPU against cells that really are at those edges.  No GPU."""
import numpy as np
import pytest

import nrt_dense_twin_cases as DC
import nrt_filter_ref as FREF
import nrt_tall_cases as TC
import nrt_tall_edge_cases as EC
import nrt_tall_ref as REF
from helpers import NRT
from scheduler_plugins_amd import objects as O

ERROR = DC.ERROR
CTR = TC.ST["container"]
_ORC = {}


def _oracle(oracle, hdr, name, strategy="LeastAllocated"):
    if (name, strategy) not in _ORC:
        c = DC.examples()[name][0]()
        s = TC.build(hdr, c, strategy)
        o = oracle.Snapshot(s["nodes"], s["pods"], rc=s["rc"], nrt=s["nrt"], nrt_params=s["params"])
        th = oracle.usable_cpus()
        _ORC[(name, strategy)] = (c, o.filter_rows(NRT, threads=th), o.score_rows(NRT, want_norm=False, threads=th)[0])
    return _ORC[(name, strategy)]


def _ref_pod(pod):
    res = O.Resources()

    def ctr(c):
        return {"requests": {k: res.canonical(k, v) for k, v in c["requests"].items()},
                "limits": {k: res.canonical(k, v) for k, v in c["limits"].items()}, "sidecar": bool(c.get("sidecar"))}
    return {"containers": [ctr(c) for c in pod["containers"]], "init_containers": [ctr(c) for c in pod["init_containers"]]}


def _policy(t):
    return {TC.CONTAINER: "container", TC.POD: "pod"}.get(t["policies"][0])


def _twin_container_cols(c):
    return [n for n, t in enumerate(c["nrts"]) if c["fresh"][n] and _policy(t) == "container" and DC.is_twin_node(t)]


# ------------------------------------------------------------------ the generators themselves
def test_id_patterns():
    for n in DC.ZONE_COUNTS:
        for sparse in (False, True):
            for name, ids in DC.patterns(n, sparse).items():
                assert len(ids) == n and len(set(ids)) < n, (n, name)
                assert (max(ids) < n) == (name != "sparse")      # LeastNUMANodes' container scope indexes the list by id
        if n >= 5:
            ids = DC.ids_lo_hi(n)
            assert ids[3] == ids[4] == min(ids) and DC.twin_positions(ids) == [3, 4]
        if n >= 3:
            ids = DC.ids_high(n)
            assert len(ids) == n and min(ids) == 0 and ids.count(0) == 1 and ids.count(1) == 2
    assert DC.ids_sparse(3) == [63, 63, 5]
    for name, (make, _) in DC.examples().items():
        c = make()
        assert len(c["nrts"]) <= 70 and len(c["pods"]) <= 40, name
        assert all(len(t["zones"]) <= 8 for t in c["nrts"])


# ------------------------------------------------------------------ even twins
@pytest.mark.parametrize("sparse", [False, True], ids=["dense-ids", "sparse-ids"])
@pytest.mark.parametrize("n", DC.ZONE_COUNTS)
def test_even_twins_hold_one_container_per_distinct_id(hdr, oracle, n, sparse):
    c, st, _ = _oracle(oracle, hdr, f"even-sparse-{n}" if sparse else f"even-{n}")
    for col, (name, ids) in enumerate(zip(c["names"], c["ids"])):
        want = [0 if k <= len(set(ids)) else CTR for k in range(1, n + 1)]
        assert st[:, col].tolist() == want, (name, ids)
    names = c["names"]
    assert len(set(c["ids"][names.index("paired")])) == (n + 1) // 2
    if "ends" in names:
        assert len(set(c["ids"][names.index("ends")])) == n - 1
    free = st[:, names.index("free")]
    assert (free == 0).all()
    for col, name in enumerate(names):                       # the duplicate-free twin of the same sizes decides differently
        if "free" not in name:
            assert (st[:, col] != free).any(), name


# ------------------------------------------------------------------ uneven twins
@pytest.mark.parametrize("sparse", [False, True], ids=["dense-ids", "sparse-ids"])
@pytest.mark.parametrize("n", DC.ZONE_COUNTS)
def test_uneven_twins_raise_the_error_where_planted(hdr, oracle, n, sparse):
    c, st, _ = _oracle(oracle, hdr, f"uneven-sparse-{n}" if sparse else f"uneven-{n}")
    free = {kind: col for col, (_, kind, what) in enumerate(c["plan"]) if what == "free"}
    for col, (name, kind, what) in enumerate(c["plan"]):
        for r, want in enumerate(c["want"]):
            got, tag = int(st[r, col]), (c["rows"][r], name, kind, what)
            if what == "twin":
                assert got == want[kind], tag
                if want[kind] == ERROR:                      # ... and the duplicate-free twin of the same sizes decides differently
                    assert st[r, free[kind]] == (CTR if c["rows"][r] == "error-then-unfit" else 0), tag
                    assert st[r + 1, col] == 0 and c["rows"][r + 1].startswith("reader"), tag
            elif what == "stale":
                assert got == TC.ST["invalid"], tag
            elif what == "not-single":
                assert got == 0, tag
            else:                                            # pod scope, and the duplicate-free twin: never an Error
                assert got != ERROR, tag
    # the Error is raised by the container it is planted on: the same row one container shorter passes
    rows = c["rows"]
    assert rows.index("eighth") >= 0 and len(c["pods"][rows.index("eighth")]["containers"]) == 8
    assert len(c["pods"][rows.index("ninth")]["containers"]) == 9 and len(c["pods"][rows.index("longest")]["containers"]) == 65
    twin_cols = [col for col, p in enumerate(c["plan"]) if p[2] == "twin"]
    assert (st[rows.index("seven-tiny"), twin_cols] == 0).all()
    assert (st[rows.index("init-first"), twin_cols] == TC.ST["init"]).all() and (st[rows.index("sidecar-first"), twin_cols] == TC.ST["sidecar"]).all()
    assert (st[rows.index("unfit-then-error"), twin_cols] == CTR).all() and (st[rows.index("error-then-unfit"), twin_cols] == ERROR).all()


@pytest.mark.parametrize("n", DC.ZONE_COUNTS)
def test_quiet_twins_never_raise_it(hdr, oracle, n):
    c, st, _ = _oracle(oracle, hdr, f"quiet-{n}")
    assert not (st == ERROR).any()
    assert (st[:-1] == 0).all()
    to_zero = c["plan"].index(("paired", "to-zero", "twin"))
    assert st[-1, to_zero] == CTR and (np.delete(st[-1], to_zero) == 0).all()


def test_mixed_case_has_one_error_column(hdr, oracle):
    c, st, _ = _oracle(oracle, hdr, "mixed")
    cols = np.flatnonzero((st == ERROR).any(axis=0))
    assert cols.tolist() == [c["twin_col"]] and len(c["nrts"]) > 64
    assert (st[:, c["twin_col"] - 1] == st[:, 0]).all() and not (st[:, 0] == ERROR).any()


# ------------------------------------------------------------------ two more readings of the Go source
def test_status_equals_the_python_reading_of_the_filter(hdr, oracle):
    """every cell of every example, and the share of Error and of passing cells among the container-scope cells on twin nodes"""
    cells = errors = passes = 0
    for name in DC.examples():
        c, st, _ = _oracle(oracle, hdr, name)
        zones = EC.ref_nodes(c)
        pods = [_ref_pod(p) for p in c["pods"]]
        for col, t in enumerate(c["nrts"]):
            alloc = set(c["nodes"][col]["allocatable"])
            for r, pod in enumerate(pods):
                assert FREF.filter_status(zones[col], pod, c["fresh"][col], _policy(t), alloc) == st[r, col], (name, r, col)
        cols = _twin_container_cols(c)
        cells += st[:, cols].size
        errors += int((st[:, cols] == ERROR).sum())
        passes += int((st[:, cols] == 0).sum())
    print(f"container-scope cells on twin nodes: {cells}, Error {errors}, pass {passes}")
    assert cells > 1000 and 4 * errors >= cells and 4 * passes >= cells


def test_status_is_the_same_for_every_strategy(hdr, oracle):
    for name in ("uneven-5", "quiet-4", "even-8"):
        st = _oracle(oracle, hdr, name)[1]
        for strategy in TC.STRATEGIES[1:]:
            assert np.array_equal(_oracle(oracle, hdr, name, strategy)[1], st), (name, strategy)


def test_least_numa_raw_scores_equal_the_python_reading_of_the_search(hdr, oracle):
    """pod scope: tests/nrt_tall_ref.py runs unchanged on nodes of at most eight zones; Guaranteed pods without init containers (its
    request is the containers' sum).  The count is of distinct ids: twins score as one NUMA node"""
    compared = 0
    for name, (_, strategies) in DC.examples().items():
        if "LeastNUMANodes" not in strategies:
            continue
        c, _, raw = _oracle(oracle, hdr, name, "LeastNUMANodes")
        zones = EC.ref_nodes(c)
        for col, t in enumerate(c["nrts"]):
            if _policy(t) != "pod" or not c["fresh"][col]:
                continue
            node = REF.Node(zones[col])
            max_numa = 8
            for r, p in enumerate(c["pods"]):
                pod = _ref_pod(p)
                if FREF.pod_qos(pod) != FREF.GUARANTEED or pod["init_containers"]:
                    continue
                assert REF.pod_scope_score(node, EC.ref_request(p), max_numa) == raw[r, col], (name, r, col)
                compared += 1
    assert compared > 300
    c, _, raw = _oracle(oracle, hdr, "least-numa-8", "LeastNUMANodes")
    assert raw[1, 0] > raw[1, 1]                 # four cores: the twins at positions 0 and 1 count one NUMA node, the free pair two
    _, _, rawc = _oracle(oracle, hdr, "least-numa-container-8", "LeastNUMANodes")
    assert rawc[6, 0] > 0 and rawc[6, 1] == 0    # container scope: ids taken as list positions leave the twins' second zone alone
