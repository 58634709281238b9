"""tests/alloc_norm_cases.py on the CPU: the constructed rows hold what their names say, the plain-integer reference equals the
oracle's orc_allocatable_normalize on every row (the wrap rows included: that agreement is what gives the wrap convention its
authority), and the case set bites — host models of three wrong kernels each disagree with the reference on a constructed cell,
the right model on none — before tests/test_gpu_alloc_norm_edges.py holds the kernels to the same reference."""
import ctypes as C

import numpy as np
import pytest

import alloc_norm_cases as ac
from helpers import NETOVERHEAD

SHAPES = (17, 1025, 16385)
_tables = {}


def tables(name, n_nodes, seed=0):
    key = (name, n_nodes, seed)
    if key not in _tables:
        _tables[key] = ac.build(name, n_nodes, seed)
    return _tables[key]


def cells(t, r):
    """(node, d, R) for the feasible nodes of row r, d and R taken from the row's own lo and hi"""
    idx = np.flatnonzero(t.masks[r])
    vals = [t.raw[i] for i in idx]
    lo, hi = min(vals), max(vals)
    return [(int(n), v - lo, hi - lo) for n, v in zip(idx, vals)]


@pytest.mark.parametrize("n_nodes", SHAPES)
@pytest.mark.parametrize("name", list(ac.CLASSES))
def test_rows_hold_what_they_name(name, n_nodes):
    klass = ac.CLASSES[name]
    assert klass.copy == (ac.COMPACT if name == "A" else ac.GENERAL)
    parts = tables(name, n_nodes)
    assert [g for t in parts for g in t.groups] == list(klass.groups)
    assert len({t.n_rows for t in parts}) == 1 and parts[0].n_rows >= 8
    branches, pinned_last = set(), False
    for t in parts:
        N = t.n_nodes
        assert N == n_nodes and len(t.raw) == N and t.masks.shape == t.want.shape == (t.n_rows, N)
        assert t.masks.dtype == t.want.dtype == np.uint8
        assert min(t.raw) == klass.glo and max(t.raw) - min(t.raw) == klass.grange      # the range that picks the copy, in every part
        assert all(-(1 << 63) < v < (1 << 63) for v in t.raw)
        names = [r.name for r in t.rows if r is not None]
        assert len(set(names)) == len(names) and sum(r is None for r in t.rows) >= ac.N_PLACEHOLDERS
        row = {r.name: (i, r) for i, r in enumerate(t.rows) if r is not None}
        for want in ("all nodes feasible", "all feasible values equal", "no feasible node", "only node 0", f"only node {N - 1}"):
            assert want in row
        i, r = row["all nodes feasible"]
        assert t.masks[i].all() and (r.lo, r.R) == (klass.glo, klass.grange)
        i, r = row["all feasible values equal"]
        assert t.masks[i].any() and r.R == 0 and r.lo != klass.glo and not t.want[i].any()
        i, r = row["no feasible node"]
        assert not t.masks[i].any() and r.lo is None and not t.want[i].any()
        for k in (0, N - 1):
            i, r = row[f"only node {k}"]
            assert np.flatnonzero(t.masks[i]).tolist() == [k] and r.R == 0 and not t.want[i].any()
        for g, grp in enumerate(t.groups):
            i, r = row[f"every cell of group {g}"]
            assert (r.lo, r.R) == (grp.lo, grp.R) and np.array_equal(t.masks[i] != 0, t.group_of == g)
            ds = {d for _, d, _ in cells(t, i)}
            assert {0, 1, grp.R - 1, grp.R} <= ds and set(grp.extra) <= ds
            for q in ac.Q_ALWAYS:
                c = ac.c_of(q, grp.R)
                assert {d for d in (c - 1, c, c + 1) if 0 <= d <= grp.R} <= ds
            if n_nodes == 16385:
                assert set(ac.family(grp.R)) <= ds
            branches.add(ac.branch(grp.R))
            if ac.branch(grp.R) != ac.WRAP:     # below the wrap the bytes are the plain quotient: 0 at lo, 100 at hi
                for n, d, R in cells(t, i):
                    assert t.want[i, n] == d * 100 // R
            assert not t.want[i][t.masks[i] == 0].any()
        assert t.pinned
        for g, a, b, adv in t.pinned:
            i, r = row[f"only lo and hi of group {g}, at nodes {(a, b)}"]
            assert np.flatnonzero(t.masks[i]).tolist() == sorted((a, b)) and (r.lo, r.R) == (t.groups[g].lo, t.groups[g].R)
            assert t.raw[a] == r.lo and t.raw[b] == r.lo + r.R
            assert (min(a, b), max(a, b)) in [(x % N, y % N) if y >= 0 else (x, N - 1) for x, y in ac.PIN_PAIRS]
            if adv is not None:
                assert t.group_of[adv] == g and t.d_of[adv] == ac.c_of(50, r.R) - 1
            pinned_last |= a == N - 1     # a feasible set whose minimum sits on the last node
        two = [r for r in t.rows if r is not None and len(r.groups) == 2]
        assert two or len(t.groups) == 1
        for r in two:
            i, j = r.groups
            assert r.lo == t.groups[i].lo and r.lo + r.R == t.groups[j].lo + t.groups[j].R and r.R > max(t.groups[i].R, t.groups[j].R)
    assert pinned_last
    if name == "A":   # offsets fit 32 bits; a lo above 2^31; exact-integer quotients exist
        assert branches == {ac.SMALL} and any(g.lo - klass.glo > 1 << 31 for g in klass.groups) and any(g.R % 100 == 0 for g in klass.groups)
    if name == "B2":  # cells whose offset from the row's lo needs more than 32 bits: the two-halves fma
        assert branches == {ac.SMALL} and any(g.R >= 1 << 32 for g in klass.groups)
    if name == "C":
        assert branches == {ac.SMALL, ac.WIDE, ac.WRAP}
        assert any(g.R >= 1 << 63 and g.lo < 0 < g.lo + g.R for g in klass.groups)
        assert {R for R, _ in ac.SEARCHED_RANGES} <= {g.R for g in klass.groups}
        assert any(g.lo < 0 and g.lo - klass.glo > 1 << 60 and ac.branch(g.R) == ac.SMALL for g in klass.groups)


@pytest.mark.parametrize("name", list(ac.CLASSES))
def test_another_seed_moves_the_nodes_and_no_answer(name):
    """the byte of a cell depends on (group, d) alone: another permutation seed, the same byte for the same raw value in every group
    row; the engine owns all padding, so the reference has none to read"""
    for ta, tb in zip(tables(name, 1025, 0), tables(name, 1025, 3)):
        assert ta.raw != tb.raw and {ta.raw[i] for i in np.flatnonzero(ta.group_of >= 0) if ta.d_of[i] in (0, 1)} == \
            {tb.raw[i] for i in np.flatnonzero(tb.group_of >= 0) if tb.d_of[i] in (0, 1)}
        assert [p[0] for p in ta.pinned] != [p[0] for p in tb.pinned]     # the seed rotates which groups are pinned
        for g in range(len(ta.groups)):
            ia = next(i for i, r in enumerate(ta.rows) if r is not None and r.name == f"every cell of group {g}")
            ib = next(i for i, r in enumerate(tb.rows) if r is not None and r.name == f"every cell of group {g}")
            byte_a = {ta.raw[n]: int(ta.want[ia, n]) for n in np.flatnonzero(ta.masks[ia])}
            byte_b = {tb.raw[n]: int(tb.want[ib, n]) for n in np.flatnonzero(tb.masks[ib])}
            common = set(byte_a) & set(byte_b)
            assert len(common) >= min(13, ta.groups[g].R + 1) and all(byte_a[v] == byte_b[v] for v in common)


@pytest.mark.parametrize("n_nodes", SHAPES)
@pytest.mark.parametrize("name", list(ac.CLASSES))
def test_reference_equals_the_oracle(oracle, name, n_nodes):
    """every row, placeholders included: orc_allocatable_normalize over the row's feasible list, clamped to the byte"""
    normalize = oracle.lib().orc_allocatable_normalize
    wrapped = 0
    for t in tables(name, n_nodes):
        for r in range(t.n_rows):
            idx = np.flatnonzero(t.masks[r])
            scores = np.array([t.raw[i] for i in idx], dtype=np.int64)
            if len(idx):
                normalize(scores.ctypes.data_as(C.POINTER(C.c_int64)), len(idx))
            want = np.zeros(t.n_nodes, dtype=np.int64)
            want[idx] = scores.clip(0, 255)
            assert np.array_equal(t.want[r].astype(np.int64), want), t.describe(r)
            wrapped += int((scores < 0).sum() + (scores > 100).sum())
    assert (wrapped > 0) == (name == "C")   # only class C leaves [0, 100] before the clamp


def search_misrounding_ranges(lo_exp, n=2, seed=42):
    """the first n ranges R, drawn uniformly from [2^lo_exp, 2^(lo_exp + 1)), with a cell of family(R) on which the single float64
    product differs from floor(d * 100 / R), each with its first such cell"""
    rng = np.random.default_rng(seed)
    found = []
    while len(found) < n:
        R = int(rng.integers(1 << lo_exp, 1 << (lo_exp + 1)))
        bad = [d for d in ac.family(R) if ac.model_single_product(d, R) != d * 100 // R]
        if bad:
            found.append((R, bad[0]))
    return tuple(found)


def test_searched_ranges_are_what_the_search_finds():
    assert search_misrounding_ranges(42) + search_misrounding_ranges(43) == ac.SEARCHED_RANGES
    for k, (R, d) in enumerate(ac.SEARCHED_RANGES):
        assert (1 << (42 + k // 2)) <= R < (1 << (43 + k // 2)) and ac.branch(R) == ac.WIDE


def search_unbiased_range(k_lo, k_hi, seed=42):
    """the first R = 100 * k, k drawn uniformly from [k_lo, k_hi), with an exact-integer cell d = q * k on which the unbiased product
    gives q - 1, with its first such cell"""
    rng = np.random.default_rng(seed)
    while True:
        k = int(rng.integers(k_lo, k_hi))
        bad = [q * k for q in range(1, 101) if ac.model_unbiased(q * k, 100 * k) != q]
        if bad:
            return 100 * k, bad[0]


def test_unbiased_ranges_are_what_the_search_finds():
    assert (search_unbiased_range(1 << 20, (1 << 32) // 100), search_unbiased_range((1 << 32) // 100 + 1, (1 << 42) // 100)) == ac.UNBIASED_RANGES
    assert ac.UNBIASED_RANGES[0][0] in {g.R for g in ac.A.groups} and ac.UNBIASED_RANGES[1][0] in {g.R for g in ac.B2.groups}


def disagreements(model, t, only=lambda R: True):
    """(row, node) of the named rows' cells on which a host model of a kernel differs from the reference"""
    out = []
    for r, row in enumerate(t.rows):
        if row is None or not row.R or not only(row.R):
            continue
        out += [(r, n) for n, d, R in cells(t, r) if model(d, R) != t.want[r, n]]
    return out


@pytest.mark.parametrize("n_nodes", SHAPES)
def test_the_case_set_catches_three_wrong_kernels_and_passes_the_right_one(n_nodes):
    below_42 = lambda R: R < (1 << 42)
    n_right = 0
    for name in ac.CLASSES:      # the right model: no disagreement on any row below 2^42, in any class
        for t in tables(name, n_nodes):
            assert disagreements(ac.model_right, t, below_42) == [], (name, t.part)
            n_right += sum(1 for r in t.rows if r is not None and r.R and below_42(r.R))
    assert n_right > 20
    # no (1 + 2^-49) bias, the multiplier one ulp down: caught by class A's exact-integer quotients (and class B's)
    for name in ("A", "B1", "B2"):
        assert any(disagreements(ac.model_no_bias, t, below_42) for t in tables(name, n_nodes)), name
    # ... and the multiplier as the division rounds it (the bias simply dropped): caught by the ranges searched for it, in A and B2
    for name, (R, d) in zip(("A", "B2"), ac.UNBIASED_RANGES):
        hit = [t.raw[n] - t.rows[r].lo for t in tables(name, n_nodes) for r, n in disagreements(ac.model_unbiased, t, lambda x: x == R)]
        assert d in hit, (name, R, d, hit)
    # the single product for every range: caught by each of class C's searched ranges, at the cell the search recorded
    for R, d in ac.SEARCHED_RANGES:
        hit = []
        for t in tables("C", n_nodes):
            for r, n in disagreements(ac.model_single_product, t, lambda x: x == R):
                hit.append(t.raw[n] - t.rows[r].lo)
        assert d in hit, (R, d, hit)
    # an unsigned quotient for every range: wrong on wrap rows only; caught at the hi node of the first wrap range and of 2^57 (the
    # product wraps negative, so does the quotient, the byte is 0 where the unsigned quotient says 100), and with the whole family
    # (16385 nodes) by every wrap row
    caught = set()
    for t in tables("C", n_nodes):
        bad_rows = {r for r, _ in disagreements(ac.model_unsigned, t)}
        for r, row in enumerate(t.rows):
            if row is None or not row.name.startswith("every cell of group"):
                continue
            assert r not in bad_rows or ac.branch(row.R) == ac.WRAP, t.describe(r)
            if r in bad_rows:
                caught.add(row.R)
            if row.R in (ac.WRAP_FROM, 1 << 57):
                hi = next(n for n, d, R in cells(t, r) if d == R)
                assert t.want[r, hi] == 0 and ac.model_unsigned(row.R, row.R) == 100 and r in bad_rows
        assert disagreements(ac.model_unsigned, t, lambda R: R < ac.WRAP_FROM) == []
    wrap_ranges = {g.R for g in ac.C.groups if ac.branch(g.R) == ac.WRAP}
    assert {ac.WRAP_FROM, 1 << 57} <= caught <= wrap_ranges and (n_nodes < 16385 or caught == wrap_ranges)


def test_tlp_utilisations_land_on_their_scores():
    """the node columns spx_decide's test uploads: the score formula gives exactly the byte asked for, for every byte 0..100, and
    is half a unit from a rounding edge (the neighbouring float64 values give the same score)"""
    for s in range(101):
        u = ac.tlp_util_for(s)
        assert 0 <= u <= 100
        for v in (u, np.nextafter(u, 0.0), np.nextafter(u, 200.0)):
            if s in (0, 100) and v != u:
                continue   # (0 and 100 sit on the clamp and on the target itself)
            assert ac.tlp_score_model(float(v), ac.TLP_CAP_MILLI) == s, (s, u, v)
    t = tables("A", 1025)[0]
    b = ac.tlp_bytes(t)
    for r, row in enumerate(t.rows):
        if row is not None and row.name.startswith("every cell of group"):
            m = t.masks[r] != 0
            assert (b[m].astype(int) + t.want[r][m] == 100).all()
    assert len(np.unique(b)) > 60


@pytest.mark.parametrize("n_nodes", sorted(ac.NET_SEEDS))
def test_network_snapshot_leaves_the_class_a_rows_usable(hdr, oracle, n_nodes):
    """the snapshot under the fused forms of k_net_cls, for the seed used on the GPU: by the oracle's NetworkOverhead Filter alone,
    ungrouped pods keep every constructed cell, no grouped row loses more than half of its group's cells, and a grouped row keeps
    a node that hosts one of its dependencies feasible"""
    parts = tables("A", n_nodes)
    snap = ac.network_snapshot(hdr, parts[0], ac.NET_SEEDS[n_nodes])
    appgroup = snap["pods"].array("appgroup")
    assert (appgroup[0::2] == -1).all() and (appgroup[1::2] >= 0).all()
    osnap = oracle.Snapshot(snap["nodes"], snap["pods"], appgroups=snap["appgroups"], nettopo=snap["nettopo"])
    status = osnap.filter_rows(NETOVERHEAD)
    assert (status != 0).any()
    for t in parts:
        assert ac.network_conditions(t, snap, status) == [], t.part
