"""The per-pod weighted argmax (k_best_fast and the general int64 k_best, kernels_profile.hip) against a numpy int64 reference on
CONSTRUCTED tables: every score table and Filter status table of the mask is bound to caller-owned memory
(spx_bind_score_table / spx_bind_status_table), spx_eval runs once so that the engine's bookkeeping says "evaluated", the rows of
tests/best_cases.py are written over what it left — whole rows, padding columns included — and spx_eval_best reads them.
The answer is tests/best_cases.py::reference; (node, score, ties, feasible) of every row is compared at tolerance 0.

Which kernel runs is launch_best's rule on the weights (best_cases.selects; stated next to each weight set in
best_cases.WEIGHT_SETS): every weight in [0, 2^23) and sum(weight * 255) < 2^31 -> k_best_fast, else k_best.

This file is the independent anchor of the tests that compare spx_decide, the multi-engine paths and the commit loops with
spx_eval + spx_eval_best."""
import numpy as np
import pytest

import best_cases as bc
from helpers import ALLOCATABLE, CAPACITY, LVRB, NETOVERHEAD, NRT, TLP
from scheduler_plugins_amd import synth
from scheduler_plugins_amd.engine import Engine, mask_of

pytestmark = pytest.mark.gpu

TRIMARAN_TABLES = (ALLOCATABLE, TLP, LVRB)
FULL_TABLES = (ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD)
RANGES = ((0, 1), (5, 6), (0, 2), (1, 4), (3, 8), (0, 5))   # single rows (16 waves on the row), counts and begins that are no multiple of 4
RANGE_SHAPES = (17, 1025, 16385)
PADS = ((255, 0), (0xAB, 0xAB))
COLUMNS = ("node", "score", "ties", "feasible")


def row_align(n: int, align: int = 128) -> int:
    return (n + align - 1) // align * align


class Bound:
    """an engine whose score tables `tables` and Filter status tables `filters` live in torch slabs"""

    def __init__(self, e, tables, filters):
        import torch
        self.torch, self.e, self.tables, self.filters = torch, e, tables, filters
        self.slabs = {}
        _, self.stride, self.rows = e.score_table(tables[0])
        for p in tables:
            _, stride, rows = e.score_table(p)
            assert (stride, rows) == (self.stride, self.rows)
            self.slabs[("score", p)] = torch.zeros((rows, stride), dtype=torch.uint8, device="cuda:0")
            e.bind_score_table(p, self.slabs[("score", p)].data_ptr(), stride, rows)
        for p in filters:
            self.slabs[("status", p)] = torch.zeros((self.rows, self.stride), dtype=torch.uint8, device="cuda:0")
            e.bind_status_table(p, self.slabs[("status", p)].data_ptr(), self.stride, self.rows)

    def bound_everywhere(self) -> bool:
        return all(self.e.score_table(p)[0] == self.slabs[("score", p)].data_ptr() for p in self.tables)

    def write(self, cases: bc.Cases) -> None:
        """whole rows, padding included"""
        arrays = [(("score", p), t) for p, t in zip(self.tables, cases.scores)] + [(("status", p), t) for p, t in zip(self.filters, cases.statuses)]
        self.torch.cuda.synchronize()
        for key, t in arrays:
            assert t.shape == (cases.n_rows, self.stride) and cases.n_rows <= self.rows
            self.slabs[key][:cases.n_rows].copy_(self.torch.from_numpy(t))
        self.torch.cuda.synchronize()

    def unbind(self) -> None:
        self.e.sync()
        for p in self.tables:
            self.e.bind_score_table(p, 0, 0, 0)
        for p in self.filters:
            self.e.bind_status_table(p, 0, 0, 0)
        self.slabs.clear()


def compare(e, mask, ranges, want, ctx, failures):
    for rb, re in ranges:
        e.eval_best(mask, rb, re)   # raises if the engine needed a table it does not have
        got = e.best(rb, re)
        for name, g, w in zip(COLUMNS, got, want):
            w = w[rb:re]
            if not np.array_equal(g.astype(np.int64), w):
                bad = np.flatnonzero(g.astype(np.int64) != w)
                failures.append((ctx, (rb, re), name, "rows", (bad[:6] + rb).tolist(), "got", g[bad[:6]].tolist(), "want", w[bad[:6]].tolist()))


def run_all(e, b, mask, tables, weight_sets, n_nodes, n_status, seed, ranges, rejected=None, ext=None):
    """every weight set x both paddings x every row range: spx_eval_best over the constructed tables against the reference"""
    failures = []
    ran = set()
    for pad in PADS:
        cases = bc.build(n_nodes, b.stride, len(tables), n_status, seed, pad=pad)
        assert cases.n_rows == e.n_pods
        if ext is not None:   # the last status table is the caller's mask as it was uploaded
            assert np.array_equal(cases.feasible_mask(n_status - 1), ext)
        b.write(cases)
        assert b.bound_everywhere()
        scores = dict(zip(tables, cases.scores))
        for w in weight_sets:
            weights = dict(zip(tables, w))
            e.set_plugin_weights(weights)
            want = bc.reference(scores, weights, cases.statuses, n_nodes, rejected)
            ran.add(bc.selects(w))
            compare(e, mask, ranges, want, (n_nodes, "pad", pad, "weights", w, bc.selects(w)), failures)
    assert ran == {bc.FAST, bc.GENERAL}
    assert not failures, (len(failures), failures[:8])


def n_case_rows(n_nodes, n_tables, n_status) -> int:
    return bc.build(n_nodes, row_align(n_nodes), n_tables, n_status, 0).n_rows   # the row list depends on the shape alone


def trimaran(hdr, n_nodes, caller_mask):
    n_status = 1 if caller_mask else 0
    n_pods = n_case_rows(n_nodes, 3, n_status)
    snap = synth.trimaran_snapshot(hdr, n_nodes, n_pods, seed=n_nodes)
    mask = mask_of(*TRIMARAN_TABLES)
    with Engine(0) as e:
        e.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])
        b = Bound(e, TRIMARAN_TABLES, ())
        assert b.stride == row_align(n_nodes)
        ext = None
        if caller_mask:   # the feasibility of the case rows (the same for both paddings: the padding is not the caller's to write)
            ext = bc.build(n_nodes, b.stride, 3, 1, seed=n_nodes).feasible_mask(0)
            e.upload_feasible_mask(ext)
        e.eval(mask)
        e.sync()
        ranges = [(0, n_pods)] + (list(RANGES) if n_nodes in RANGE_SHAPES else [])
        try:
            run_all(e, b, mask, TRIMARAN_TABLES, [w for w, _ in bc.WEIGHT_SETS], n_nodes, n_status, n_nodes, ranges, ext=ext)
        finally:
            b.unbind()


@pytest.mark.parametrize("n_nodes", [1, 16, 17, 255, 257, 1023, 1024, 1025, 4097, 16385])
def test_constructed_tables_trimaran(gpu_required, hdr, n_nodes):
    """Allocatable + TargetLoadPacking + LVRB: three score tables; the caller's feasibility mask is the one status table, uploaded
    before spx_eval and left alone afterwards (spx_eval_best checks its generation).  16385 nodes give a single-row launch of the
    fast kernel more than 16 tiles (a wave takes a second one), 4097 do the same for the general kernel."""
    trimaran(hdr, n_nodes, caller_mask=True)


@pytest.mark.parametrize("n_nodes", [17, 1025])
def test_constructed_tables_trimaran_without_a_status_table(gpu_required, hdr, n_nodes):
    """no caller mask: no status table stands between the kernels and the padding columns, which hold 255 (the engine's own copy
    of a caller mask marks its padding infeasible, so only this run has padding that looks like the best feasible node)"""
    trimaran(hdr, n_nodes, caller_mask=False)


@pytest.mark.parametrize("caller_mask", [True, False])
@pytest.mark.parametrize("n_nodes", [17, 1025])
def test_constructed_tables_full_profile(gpu_required, hdr, oracle, n_nodes, caller_mask):
    """the whole profile: five score tables, NRT's and NetworkOverhead's bound status tables and the caller's mask (three status
    tables; two without the caller's mask), and CapacityScheduling's PreFilter: the rows it rejects report (-1, 0, 0, 0)
    whatever the tables hold"""
    from test_gpu_profile import ALL, load_all
    n_status = 3 if caller_mask else 2
    n_pods = n_case_rows(n_nodes, 5, n_status)
    snap = synth.full_snapshot(hdr, n_nodes, n_pods, seed=1, pods_per_group=20, n_namespaces=20)
    # quotas for three namespaces only: in a batch this small the generator's quotas turn most pods away, and a rejected row
    # compares nothing but (-1, 0, 0, 0)
    snap["quota"].array("has_quota")[3:] = 0
    rejected = np.array([oracle.lib().orc_capacity_prefilter(snap["pods"].ref(), snap["rc"].ref(), snap["quota"].ref(), i)
                         for i in range(n_pods)], dtype=np.uint8) != 0
    assert 1 <= rejected.sum() <= n_pods // 6
    mask = mask_of(*ALL)
    weight_sets = [bc.extend(w, 5) for w, _ in bc.WEIGHT_SETS] + [bc.FIVE_TABLE_LARGEST]
    with Engine(0) as e:
        load_all(e, hdr, snap)
        b = Bound(e, FULL_TABLES, (NRT, NETOVERHEAD))
        ext = None
        if caller_mask:
            ext = bc.build(n_nodes, b.stride, 5, 3, seed=n_nodes).feasible_mask(2)
            e.upload_feasible_mask(ext)
        e.eval(mask)
        e.sync()
        assert np.array_equal(e.prefilter(CAPACITY) != 0, rejected)
        ranges = [(0, n_pods)] + list(RANGES)
        try:
            run_all(e, b, mask, FULL_TABLES, weight_sets, n_nodes, n_status, n_nodes, ranges, rejected, ext)
        finally:
            b.unbind()


def test_largest_admitted_weight_and_the_refusal(gpu_required, hdr):
    """spx_set_plugin_weights refuses weights whose totals could leave int64 (sum of |weight| * 255 over the scoring plugins above
    INT64_MAX, include/spx.h); the largest weight it admits, 36170086419038336, and its negative run through the general kernel:
    the 255 byte's total is 2^63 - 128"""
    from scheduler_plugins_amd import SpxError
    from scheduler_plugins_amd.engine import NUM_PLUGINS
    largest = (2 ** 63 - 1) // 255
    assert largest == 36170086419038336
    n_nodes = 257
    n_pods = n_case_rows(n_nodes, 3, 1)
    snap = synth.trimaran_snapshot(hdr, n_nodes, n_pods, seed=n_nodes)
    mask = mask_of(*TRIMARAN_TABLES)
    zero = {p: 0 for p in range(NUM_PLUGINS)}
    with Engine(0) as e:
        e.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])
        b = Bound(e, TRIMARAN_TABLES, ())
        cases = bc.build(n_nodes, b.stride, 3, 1, seed=n_nodes)
        e.upload_feasible_mask(cases.feasible_mask(0))
        e.eval(mask)
        e.sync()
        try:
            b.write(cases)
            scores = dict(zip(TRIMARAN_TABLES, cases.scores))
            failures = []
            for w in ((largest, 0, 0), (0, -largest, 0), (largest - 2, 1, 1), (-(largest - 2), -1, -1)):
                weights = dict(zip(TRIMARAN_TABLES, w))
                e.set_plugin_weights({**zero, **weights})
                want = bc.reference(scores, weights, cases.statuses, n_nodes)
                assert np.abs(want[1]).max() > 2 ** 53 and (w[0] <= 0 or want[1].max() == 2 ** 63 - 128)
                compare(e, mask, [(0, n_pods), (2, 3)], want, ("weights", w), failures)
            assert not failures, failures[:8]
            # one more, anywhere among the scoring plugins: refused, and the weights in place stay
            for w in ((largest + 1, 0, 0), (largest, 1, 0), (-largest, 0, -1), (2 ** 63 - 1, 0, 0), (-2 ** 63, 0, 0), (2 ** 62, 2 ** 62, 2 ** 62)):
                with pytest.raises(SpxError):
                    e.set_plugin_weights({**zero, **dict(zip(TRIMARAN_TABLES, w))})
            with pytest.raises(SpxError):   # the unnamed plugins' default weight of 1 counts
                e.set_plugin_weights({ALLOCATABLE: largest})
            e.eval_best(mask)
            for name, g, wnt in zip(COLUMNS, e.best(), want):
                assert np.array_equal(g.astype(np.int64), wnt), name
        finally:
            b.unbind()
