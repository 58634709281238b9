"""SPX_OPT_TLP_CHUNK_SCHED: the chunks of 64 positions of the class form's value-sorted order (SPX_OPT_TLP_POD_CLASSES) are launched
heaviest first — sorted, stably, by descending number of positions the sweep evaluates in them, the last, partial chunk left last — and
the build's scan runs over many blocks.  None of it may change a byte of a table or the count of evaluated rows.

Every case runs three engines on one snapshot of 1 100 nodes (two tiles, the second with 76 live nodes): chunk schedule on, chunk
schedule off (value order), class form off.  Before the compared evaluation every engine evaluates once under another target
utilisation, so a row the sweep skipped would keep other bytes.  TargetLoadPacking's and Allocatable's tables are compared byte for
byte, the rows with a non-negative value against the oracle, spx_tlp_form must say "classes", spx_tlp_pod_classes must give the numpy
count, and the order itself (spx_tlp_fetch_order) is checked against a numpy restatement of the schedule.

Values outside the table [0, 65 536) share one bin whose inner order is whatever the scatter's atomics left, so there the count of
evaluated rows is held between its two bounds (exact for the positions inside the table) and the schedule's keys are computed from the
order the engine reports."""
import numpy as np
import pytest

from helpers import ALLOCATABLE, TLP, tlp_params
from scheduler_plugins_amd import objects as O
from scheduler_plugins_amd import synth
from scheduler_plugins_amd.engine import Engine, mask_of

pytestmark = pytest.mark.gpu

N_NODES = 1_100
AMB_SIZE = 1 << 16
CHUNK = 64
PLAIN, CLASSES = 1, 2
BOTH = mask_of(ALLOCATABLE, TLP)

_snap = {}


def _snapshot(hdr):
    if "s" not in _snap:
        _snap["s"] = synth.trimaran_snapshot(hdr, N_NODES, 8, seed=77 + N_NODES, round_frac=0.0)
    return _snap["s"]


def _pods_for(hdr, values):
    """pod objects whose TargetLoadPacking value is max(v, 0): one app container with that cpu limit (targetloadpacking.go:198-205)"""
    res = O.Resources()
    return O.build_pod_objects(hdr, res, [O.pod([O.container(None, {"cpu": f"{max(int(v), 0)}m"})]) for v in values])


def _inside(v):
    return (v >= 0) & (v < AMB_SIZE)


def _evaluated_mask(vals):
    """the sweep's own test on an order's values: a position is evaluated when it starts a chunk or differs from the one before"""
    p = np.arange(len(vals))
    return (p % CHUNK == 0) | (vals != np.roll(vals, 1))


def _keys(vals):
    """per whole chunk: evaluated positions, or 64 when the chunk holds a value outside the table"""
    n_whole = len(vals) // CHUNK
    ev = _evaluated_mask(vals)[:n_whole * CHUNK].reshape(n_whole, CHUNK).sum(axis=1)
    out = (~_inside(vals[:n_whole * CHUNK])).reshape(n_whole, CHUNK).any(axis=1)
    return np.where(out, CHUNK, ev)


class _Trio:
    """three engines on one snapshot: `sched` (chunk schedule on, the default), `value` (off), `plain` (class form off)"""

    def __init__(self, hdr, cls_opt=1, target=40):
        self.hdr, self.snap, self.target = hdr, _snapshot(hdr), target
        self.sched, self.value, self.plain = Engine(0), Engine(0), Engine(0)
        assert self.sched.get_option("TLP_CHUNK_SCHED") == 1  # the default
        self.value.set_option("TLP_CHUNK_SCHED", 0)
        self.sched.set_option("TLP_POD_CLASSES", cls_opt)
        self.value.set_option("TLP_POD_CLASSES", cls_opt)
        self.plain.set_option("TLP_POD_CLASSES", 0)
        self.all = (self.sched, self.value, self.plain)
        for e in self.all:
            e.set_tlp(target_utilization=target)
            e.upload_alloc_nodes(e.flatten_alloc_nodes(self.snap["nodes"], self.snap["rc"]))
            e.upload_trimaran_nodes(e.flatten_trimaran_nodes(self.snap["nodes"], self.snap["metrics"], self.snap["assigned"]))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for e in self.all:
            e.close()

    def upload(self, values):
        values = np.asarray(values, np.int64)
        self.pods = _pods_for(self.hdr, values)
        cols = self.sched.flatten_trimaran_pods(self.pods)
        assert np.array_equal(cols["tlp_pod_milli"], np.maximum(values, 0))  # the objects do carry the values
        cols["tlp_pod_milli"] = values.copy()
        self.values = values
        for e in self.all:
            e.upload_trimaran_pods(cols)

    def order(self, e):
        """(rows, values): the pod row at every position of the engine's order and its value"""
        rows = e.tlp_order()
        assert rows.min() >= 0 and rows.max() < len(self.values)
        return rows, self.values[rows]

    def check_counts(self):
        """spx_tlp_pod_classes of both ordered engines against numpy; the same number whatever the schedule when it is determined"""
        v = self.values
        n = len(v)
        srt = np.sort(v[_inside(v)])
        n_in = len(srt)
        inside_ev = int(_evaluated_mask(srt).sum()) if n_in else 0
        n_out = n - n_in
        # outside the table, positions [n_in, n): at least the chunk starts among them, and position n_in itself when it starts no chunk
        # (the value before it lies inside the table); at most every row
        starts = len(range(-(-n_in // CHUNK) * CHUNK, n, CHUNK))
        lo = inside_ev + starts + (1 if n_out and n_in % CHUNK else 0)
        hi = inside_ev + n_out
        got = []
        for e in (self.sched, self.value):
            ev, cp = e.tlp_pod_classes()
            assert ev + cp == n
            assert lo <= ev <= hi, (ev, lo, hi)
            _, vals = self.order(e)
            assert ev == int(_evaluated_mask(vals).sum())  # ... and exactly what the order in place makes the sweep evaluate
            got.append(ev)
        if not n_out:
            assert got[0] == got[1] == inside_ev
        print(f"rows {n}: evaluated {got}, bounds [{lo}, {hi}]")
        return got

    def check_orders(self, sched_on=True):
        """the order of `value` is the sorted batch; the order of `sched` is a stable sort of its whole chunks by descending key"""
        v = self.values
        n = len(v)
        n_whole = n // CHUNK
        n_in = int(_inside(v).sum())
        for e, on in ((self.value, False), (self.sched, sched_on)):
            rows, vals = self.order(e)
            assert np.array_equal(np.sort(rows), np.arange(n))          # a permutation of the rows
            chunks = vals[:n_whole * CHUNK].reshape(n_whole, CHUNK)
            firsts = chunks[:, 0]
            if not on:
                assert np.array_equal(vals[:n_in], np.sort(v[_inside(v)]))      # value order, the rows outside the table behind
                assert not _inside(vals[n_in:]).any()
                continue
            # the last, partial chunk stayed last: it holds the largest values / the rows outside the table that value order puts there
            tail = vals[n_whole * CHUNK:]
            if len(tail):
                if n_in >= n_whole * CHUNK:
                    assert np.array_equal(tail[:n_in - n_whole * CHUNK], np.sort(v[_inside(v)])[n_whole * CHUNK:])
                else:
                    assert not _inside(tail).any()
            # the keys, as the sweep will see them, never increase along the launch ...
            keys = _keys(vals)
            assert (np.diff(keys) <= 0).all(), keys.tolist()
            # ... chunks are still runs of the sorted order: inside a chunk the values inside the table ascend, the others behind them
            for c in chunks:
                ins = _inside(c)
                k = int(ins.sum())
                assert ins[:k].all() and (np.diff(c[:k]) >= 0).all()
            # ... and equal keys keep value order (stable): among chunks of one key that lie wholly inside the table, first values ascend
            whole_in = _inside(chunks).all(axis=1)
            for key in np.unique(keys):
                f = firsts[(keys == key) & whole_in]
                assert (np.diff(f) >= 0).all(), (int(key), f.tolist())
        return self.order(self.sched)

    def eval_same(self, form=CLASSES):
        """dirties the tables under another target, then evaluates on all three and compares the tables byte for byte"""
        for e in self.all:
            e.set_tlp(target_utilization=73)
            e.eval(BOTH)
            e.set_tlp(target_utilization=self.target)
            e.eval(BOTH)
            e.sync()
        assert self.plain.tlp_form() == PLAIN
        assert self.sched.tlp_form() == form and self.value.tlp_form() == form, (self.sched.tlp_form(), self.value.tlp_form(), self.sched.tlp_pod_classes())
        tabs = {}
        for p in (TLP, ALLOCATABLE):
            ref = self.plain.all_scores(p)
            for e in (self.sched, self.value):
                bad = e.all_scores(p) != ref
                assert not bad.any(), (p, int(bad.sum()), np.argwhere(bad)[:5].tolist())
            tabs[p] = ref
        return tabs

    def check_oracle(self, oracle, table):
        osnap = oracle.Snapshot(self.snap["nodes"], self.pods, rc=self.snap["rc"], metrics=self.snap["metrics"], assigned=self.snap["assigned"],
                                alloc_params=self.sched.alloc_params, tlp_params=tlp_params(self.hdr, target_utilization=self.target))
        want = osnap.score_rows(TLP, threads=oracle.usable_cpus(), want_norm=False)[0]
        rows = self.values >= 0
        assert rows.any()
        bad = table[rows].astype(np.int64) != want[rows]
        assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist())

    def run(self, oracle, values, form=CLASSES):
        self.upload(values)
        self.check_counts()
        order = self.check_orders()
        tabs = self.eval_same(form)
        self.check_oracle(oracle, tabs[TLP])
        return order


def _heavy_end():
    """600 rows of one value, then 400 distinct increasing ones: 1 000 rows = 15 whole chunks and one of 40 positions"""
    return np.concatenate([np.full(600, 500, np.int64), 1_000 + 7 * np.arange(400, dtype=np.int64)])


def test_heavy_end(gpu_required, hdr, oracle):
    """value order ends in the all-distinct chunks; the schedule launches them first and the one-value chunks behind"""
    with _Trio(hdr) as t:
        _, vals = t.run(oracle, _heavy_end())
        keys = _keys(vals)
        assert keys[0] == CHUNK and keys[-1] == 1 and len(keys) == 15
        assert (vals[:CHUNK] >= 1_000).all() and len(vals) % CHUNK == 40


def test_heavy_start(gpu_required, hdr, oracle):
    """the same batch with the values reversed: the heavy chunks are the first of value order as well"""
    v = _heavy_end()
    with _Trio(hdr) as t:
        _, vals = t.run(oracle, (v.max() + 1 - v)[::-1].copy())
        assert _keys(vals)[0] == CHUNK


def test_all_keys_equal(gpu_required, hdr, oracle):
    """one value everywhere: every key is 1 and the stable sort leaves the order alone"""
    with _Trio(hdr) as t:
        t.run(oracle, np.full(1_000, 1_700, np.int64))
        assert np.array_equal(t.order(t.sched)[1], t.order(t.value)[1])
        assert (_keys(t.order(t.sched)[1]) == 1).all()
    # ... and distinct values in every chunk but with equal keys: chunk c holds 4 values 16 times each, so all keys are 4
    with _Trio(hdr) as t:
        v = np.repeat(100 + 3 * np.arange(64, dtype=np.int64), 16)[:1_000]
        t.run(oracle, np.random.default_rng(1).permutation(v))
        assert np.array_equal(t.order(t.sched)[1], t.order(t.value)[1])


@pytest.mark.parametrize("n_pods", [257, 330])
def test_short_last_chunk_stays_last(gpu_required, hdr, oracle, n_pods):
    """a last chunk of 1 and of 10 positions: it holds the largest values and is no part of the sort; the whole chunks before it have
    keys that rise in value order (1 distinct value per chunk, then 2, ...), so the schedule does move them"""
    reps = np.repeat(np.arange(4, dtype=np.int64), CHUNK)           # chunks 0..3: one value each -> key 1
    reps[CHUNK:2 * CHUNK] = 10 + np.arange(CHUNK) // 16             # chunk 1: 4 values -> key 4
    reps[2 * CHUNK:3 * CHUNK] = 20 + np.arange(CHUNK) // 32         # chunk 2: 2 values -> key 2
    reps[3 * CHUNK:] = 30 + np.arange(CHUNK) // 8                   # chunk 3: 8 values -> key 8
    v = np.concatenate([reps * 50 + 50, np.full(n_pods - 4 * CHUNK, 40_000, np.int64)])
    with _Trio(hdr) as t:
        _, vals = t.run(oracle, np.random.default_rng(n_pods).permutation(v))
        n_whole = n_pods // CHUNK  # (330 rows: a fifth whole chunk, of the large value alone — key 1, behind chunk 0 in the stable sort)
        assert _keys(vals).tolist() == [8, 4, 2, 1] + [1] * (n_whole - 4)
        assert (vals[3 * CHUNK:4 * CHUNK] == 50).all() and (vals[4 * CHUNK:] == 40_000).all()


def test_values_outside_the_table(gpu_required, hdr, oracle):
    """-5, 65 535, 65 536, 2^23 and 2^40 scattered over the batch; 90 rows inside the table's last chunk region so that one chunk
    straddles other_start (its key is 64 whatever it evaluates)"""
    rng = np.random.default_rng(11)
    inside = np.concatenate([np.full(400, 250, np.int64), np.full(300, 900, np.int64), 2_000 + np.arange(10, dtype=np.int64), np.full(20, 65_535, np.int64)])
    outside = np.resize(np.array([-5, 65_536, 1 << 23, 1 << 40], np.int64), 270)
    v = rng.permutation(np.concatenate([inside, outside]))           # 730 inside (11 chunks + 26 positions), 270 outside
    assert len(v) == 1_000 and int(_inside(v).sum()) % CHUNK != 0
    with _Trio(hdr, cls_opt=2) as t:
        _, vals = t.run(oracle, v)
        keys = _keys(vals)
        straddle = [c for c in range(len(keys)) if 0 < int(_inside(vals[c * CHUNK:(c + 1) * CHUNK]).sum()) < CHUNK]
        assert len(straddle) == 1 and keys[straddle[0]] == CHUNK
        assert (keys[:4] == CHUNK).all()  # the chunks with rows outside the table lead the launch


def test_two_uploads_on_one_engine(gpu_required, hdr, oracle):
    """heavy end, then heavy start, on the same engines; the option is read when the order is built, so flipping it between the
    uploads leaves the order in place alone and shows at the next upload"""
    v1 = _heavy_end()
    v2 = (v1.max() + 1 - v1)[::-1].copy()
    with _Trio(hdr) as t:
        t.run(oracle, v1)
        before = t.order(t.sched)
        t.sched.set_option("TLP_CHUNK_SCHED", 0)
        after = t.order(t.sched)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        t.eval_same()                                   # still the scheduled order of v1, still the same bytes
        t.upload(v2)                                    # now built in value order
        t.check_counts()
        t.check_orders(sched_on=False)
        assert np.array_equal(t.order(t.sched)[1], np.sort(v2))
        tabs = t.eval_same()
        t.check_oracle(oracle, tabs[TLP])
        t.sched.set_option("TLP_CHUNK_SCHED", 1)
        t.upload(v1)                                    # and scheduled again
        t.check_counts()
        t.check_orders()
        assert not np.array_equal(t.order(t.sched)[1], np.sort(v1))
        tabs = t.eval_same()
        t.check_oracle(oracle, tabs[TLP])


def test_scan_over_blocks(gpu_required, hdr, oracle):
    """the bins at both ends of the scan's blocks of 1 024 — 0, 1 023, 1 024, 2 047, 65 535 and the bin of the rows outside — and
    3 000 distinct values spread over the table, so that the counts before a bin cross many block totals"""
    rng = np.random.default_rng(5)
    edges = np.array([0, 1_023, 1_024, 2_047, 65_535], np.int64)
    spread = rng.permutation(np.arange(2_048, 65_535, dtype=np.int64))[:3_000 - len(edges)]
    distinct = np.concatenate([edges, spread])
    v = np.concatenate([np.repeat(edges, 5), distinct, rng.choice(distinct, 3_200), np.full(70, 1 << 20, np.int64), np.full(5, -1, np.int64)])
    v = rng.permutation(v)
    assert len(np.unique(v[_inside(v)])) == 3_000
    with _Trio(hdr, cls_opt=2) as t:
        t.run(oracle, v)
        rows, vals = t.order(t.value)
        n_in = int(_inside(v).sum())
        assert np.array_equal(vals[:n_in], np.sort(v[_inside(v)]))
        for b in edges:  # every edge bin starts where numpy says
            assert int(np.argmax(vals == b)) == int((np.sort(v[_inside(v)]) < b).sum())
