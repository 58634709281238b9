"""SPX_OPT_ALLOC_TABLE_KEEP: without a Filter plugin, NodeResourcesAllocatable's score table is one normalised row repeated for every
pod, and spx_eval does not write rows that already hold the row in place.  A stale keep would not crash — it would return plausible
bytes — so every step of every sequence here is held to a second engine that gets the same calls with the option off (it writes the
table on every evaluation, the behaviour before the option existed): Allocatable's and TargetLoadPacking's tables byte for byte, and
on whole object snapshots to the CPU oracle as well.  spx_alloc_table_path says whether the evaluation kept (2) or wrote (1) the
rows, so that a correct skip can be told from no skip: the expected value is asserted wherever the sequence determines it."""
import numpy as np
import pytest

from helpers import ALLOCATABLE, LVRB, NETOVERHEAD, NRT, TLP
from scheduler_plugins_amd import objects as O
from scheduler_plugins_amd import synth
from scheduler_plugins_amd.engine import Engine, mask_of
from scheduler_plugins_amd.multi import PEER_COPY, MultiEngine

pytestmark = pytest.mark.gpu

AT = mask_of(ALLOCATABLE, TLP)
WROTE, KEPT = 1, 2


def path(e) -> int:
    return int(e._lib.spx_alloc_table_path(e._h))


class Pair:
    """two engines driven alike: `k` with the option on (the default), `r` with it off"""

    def __init__(self, options=None):
        self.k, self.r = Engine(0), Engine(0)
        for name, value in (options or {}).items():
            self.both(lambda e: e.set_option(name, value))
        assert self.k.get_option("ALLOC_TABLE_KEEP") == 1  # the default
        self.r.set_option("ALLOC_TABLE_KEEP", 0)

    def close(self):
        self.k.close()
        self.r.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def both(self, fn):
        fn(self.k)
        fn(self.r)

    def eval(self, mask, b=0, end=None, expect=None, ctx=""):
        """evaluate on both, compare every score table of the mask over the rows; `expect`: what spx_alloc_table_path must say on k"""
        end = self.k.n_pods if end is None else end
        self.both(lambda e: (e.eval(mask, b, end), e.sync()))
        if expect is not None:
            assert path(self.k) == expect, (ctx, path(self.k))
        assert path(self.r) == (WROTE if mask & mask_of(ALLOCATABLE) else 0), ctx
        out = {}
        for p in (ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD):
            if (mask >> p) & 1:
                got, want = self.k.all_scores(p, b, end), self.r.all_scores(p, b, end)
                assert np.array_equal(got, want), (ctx, p, int((got != want).sum()))
                out[p] = got
        return out


def load(e, snap):
    e.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])


def check_oracle(oracle, e, snap, tables, ctx=""):
    osnap = oracle.Snapshot(snap["nodes"], snap["pods"], rc=snap["rc"], metrics=snap["metrics"], assigned=snap["assigned"],
                            alloc_params=e.alloc_params, tlp_params=e.tlp_params, lvrb_params=e.lvrb_params)
    for p, got in tables.items():
        _, norm = osnap.score_rows(p)
        assert np.array_equal(got.astype(np.int64), norm), (ctx, p)


def test_repeated_evals_pod_batches_and_node_deltas(gpu_required, hdr, oracle):
    snap = synth.trimaran_snapshot(hdr, 700, 300, seed=3, round_frac=0.1)
    with Pair() as pr:
        pr.both(lambda e: load(e, snap))
        check_oracle(oracle, pr.k, snap, pr.eval(AT, expect=WROTE, ctx="first"), "first")
        for i in range(3):
            check_oracle(oracle, pr.k, snap, pr.eval(AT, expect=KEPT, ctx=f"repeat {i}"), f"repeat {i}")
        pr.eval(mask_of(ALLOCATABLE), expect=KEPT, ctx="Allocatable alone: nothing to launch")
        pr.eval(mask_of(ALLOCATABLE, TLP, LVRB), expect=KEPT, ctx="with LVRB")
        pr.eval(mask_of(ALLOCATABLE, LVRB), expect=KEPT, ctx="LVRB carries no Allocatable stores either")
        # a new pending batch of the same size: the rows of the table do not depend on it
        snap2 = dict(snap, pods=synth.synth_pods(hdr, 300, seed=77))
        pr.both(lambda e: e.upload_trimaran_pods(e.flatten_trimaran_pods(snap2["pods"])))
        check_oracle(oracle, pr.k, snap2, pr.eval(AT, expect=KEPT, ctx="new pods"), "new pods")
        # load-watcher metrics move on some nodes (what a scheduling cycle brings): Allocatable reads none of them
        snap3 = dict(snap2, metrics=synth.synth_metrics(hdr, 700, seed=91))
        cols = pr.k.flatten_trimaran_nodes(snap3["nodes"], snap3["metrics"], snap3["assigned"])
        idx = np.arange(0, 700, 7)
        pr.both(lambda e: e.update_trimaran_nodes(idx, cols))
        pr.eval(AT, expect=KEPT, ctx="node delta")
        pr.both(lambda e: e.upload_trimaran_nodes(cols))
        check_oracle(oracle, pr.k, snap3, pr.eval(AT, expect=KEPT, ctx="node table"), "node table")


def test_a_larger_batch_is_a_new_engine_and_starts_by_writing(gpu_required, hdr, oracle):
    """an engine holds one batch size; the larger batch goes to a new engine, whose table has never been written"""
    for n_pods in (200, 450):
        snap = synth.trimaran_snapshot(hdr, 500, n_pods, seed=5)
        with Pair() as pr:
            pr.both(lambda e: load(e, snap))
            check_oracle(oracle, pr.k, snap, pr.eval(AT, expect=WROTE, ctx=f"{n_pods} first"))
            pr.eval(AT, expect=KEPT, ctx=f"{n_pods} second")


def test_allocatable_reuploads_and_params(gpu_required, hdr, oracle):
    snap = synth.trimaran_snapshot(hdr, 600, 260, seed=4)
    with Pair() as pr:
        pr.both(lambda e: load(e, snap))
        pr.eval(AT, expect=WROTE)
        pr.eval(AT, expect=KEPT)
        base = pr.k.flatten_alloc_nodes(snap["nodes"], snap["rc"])
        # identical columns (a node re-list with unchanged allocatable): the recomputed row is the row in place
        pr.both(lambda e: e.upload_alloc_nodes(base.copy()))
        check_oracle(oracle, pr.k, snap, pr.eval(AT, expect=KEPT, ctx="identical re-upload"), "identical re-upload")
        # changed columns
        changed = base.copy()
        changed[:, ::3] //= 2
        pr.both(lambda e: e.upload_alloc_nodes(changed))
        t = pr.eval(AT, expect=WROTE, ctx="changed columns")
        pr.eval(AT, expect=KEPT, ctx="changed columns, again")
        # a permutation of the nodes: the same multiset of values, another row
        perm = np.roll(np.arange(600), 1)
        assert not np.array_equal(changed[:, perm], changed)
        pr.both(lambda e: e.upload_alloc_nodes(np.ascontiguousarray(changed[:, perm])))
        t2 = pr.eval(AT, expect=WROTE, ctx="permutation")
        assert np.array_equal(t2[ALLOCATABLE][:, 1:], t[ALLOCATABLE][:, :-1])
        # back to the snapshot's own columns, then the parameters
        pr.both(lambda e: e.upload_alloc_nodes(base.copy()))
        check_oracle(oracle, pr.k, snap, pr.eval(AT, expect=WROTE, ctx="base again"), "base again")
        pr.both(lambda e: e.set_allocatable("Most"))
        check_oracle(oracle, pr.k, snap, pr.eval(AT, expect=WROTE, ctx="mode Most"), "mode Most")
        pr.eval(AT, expect=KEPT, ctx="mode Most, again")
        pr.both(lambda e: e.set_allocatable("Most"))  # the same parameters once more: the same row
        pr.eval(AT, expect=KEPT, ctx="same params")
        before = pr.r.all_scores(ALLOCATABLE, 0, 1)[0].copy()
        pr.both(lambda e: e.set_allocatable("Most", {1: 1, 0: 3}))
        t3 = pr.eval(AT, ctx="weights")  # kept exactly when the new weights leave the normalised row as it was
        assert path(pr.k) == (KEPT if np.array_equal(t3[ALLOCATABLE][0], before) else WROTE)
        check_oracle(oracle, pr.k, snap, t3, "weights")
        pr.both(lambda e: e.set_allocatable("Least"))
        check_oracle(oracle, pr.k, snap, pr.eval(AT, expect=WROTE, ctx="mode Least"), "mode Least")


def test_filter_plugins_in_the_mask_then_unmasked_again(gpu_required, hdr):
    snap = synth.full_snapshot(hdr, 300, 240, seed=6, pods_per_group=20, n_namespaces=20)
    params = O.nrt_params(hdr, O.Resources(), "LeastAllocated")

    def load_full(e):
        load(e, snap)
        e.load_nrt_objects(snap["nodes"], snap["nrt"], snap["rc"], snap["pods"], params)
        e.load_network_objects(snap["nodes"], snap["pods"], snap["appgroups"], snap["nettopo"])

    with Pair() as pr:
        pr.both(load_full)
        pr.eval(AT, expect=WROTE)
        pr.eval(AT, expect=KEPT)
        for filt in ((NRT,), (NETOVERHEAD,), (NRT, NETOVERHEAD)):
            # the feasibility-aware normalisation writes other bytes into the same table ...
            pr.eval(mask_of(ALLOCATABLE, TLP, *filt), expect=WROTE, ctx=f"masked {filt}")
            pr.eval(mask_of(ALLOCATABLE, TLP, *filt), expect=WROTE, ctx=f"masked {filt}, again")
            # ... so the broadcast has to come back
            pr.eval(AT, expect=WROTE, ctx=f"unmasked after {filt}")
            pr.eval(AT, expect=KEPT, ctx=f"unmasked after {filt}, again")
        pr.eval(mask_of(ALLOCATABLE, NRT), 10, 50, expect=WROTE, ctx="masked rows")
        pr.eval(AT, 60, 90, expect=WROTE, ctx="unmasked rows elsewhere")
        pr.eval(AT, expect=WROTE, ctx="whole table after masked rows")
        # a caller's feasibility mask is a Filter too
        feas = (np.random.default_rng(2).random((240, 300)) < 0.7).astype(np.uint8)
        pr.both(lambda e: e.upload_feasible_mask(feas))
        pr.eval(AT, expect=WROTE, ctx="caller mask")
        pr.both(lambda e: e.upload_feasible_mask(None))
        pr.eval(AT, expect=WROTE, ctx="caller mask cleared")
        pr.eval(AT, expect=KEPT, ctx="caller mask cleared, again")
        # spx_decide and the commit loop with Filter plugins, then the tables again
        # (path 0 after them: Allocatable's normalisation was folded into the argmax and its table left alone; 1: the masked rows were written)
        pr.both(lambda e: (e.decide(mask_of(ALLOCATABLE, TLP, NRT)), e.sync()))
        assert path(pr.k) in (0, WROTE)
        pr.eval(AT, expect=KEPT if path(pr.k) == 0 else WROTE, ctx="after spx_decide with NRT")
        pr.both(lambda e: e.commit_sequential(mask_of(ALLOCATABLE, TLP, NRT), 0, 40))
        assert pr.k.commit_path() in (2, 3)
        # the cooperative kernel (3) evaluates nothing through spx_eval and touches no table; the per-pod loop (2) ends on a single-row spx_eval
        untouched = pr.k.commit_path() == 3 or path(pr.k) == 0
        pr.eval(AT, expect=KEPT if untouched else WROTE, ctx="after the commit loop with NRT")
        pr.both(lambda e: e.set_option("COMMIT_COOP", 0))
        pr.both(lambda e: e.set_option("DECIDE_UNFUSED", 1))
        pr.both(lambda e: e.commit_sequential(mask_of(ALLOCATABLE, TLP, NRT), 0, 40))
        pr.eval(AT, expect=WROTE, ctx="after the per-pod commit loop, Allocatable's masked rows written")
        pr.eval(AT, expect=KEPT)


def test_row_ranges(gpu_required, hdr):
    snap = synth.trimaran_snapshot(hdr, 400, 500, seed=7)
    n, k = 500, 130
    with Pair() as pr:
        pr.both(lambda e: load(e, snap))
        pr.eval(AT, 0, k, expect=WROTE, ctx="[0,k)")
        pr.eval(AT, 0, k, expect=KEPT, ctx="[0,k) again")
        pr.eval(AT, k, n, expect=WROTE, ctx="[k,n): adjacent, joins")
        pr.eval(AT, 0, n, expect=KEPT, ctx="[0,n)")
        pr.eval(AT, 17, 333, expect=KEPT, ctx="inside")
        pr.eval(AT, 40, 40, ctx="empty range")
    with Pair() as pr:
        pr.both(lambda e: load(e, snap))
        pr.eval(AT, 0, 100, expect=WROTE, ctx="[0,100)")
        pr.eval(AT, 200, 300, expect=WROTE, ctx="[200,300): disjoint, replaces")
        pr.eval(AT, 200, 300, expect=KEPT)
        pr.eval(AT, 0, 100, expect=WROTE, ctx="[0,100) is no longer recorded")
        pr.eval(AT, 0, 150, expect=WROTE, ctx="larger than what is recorded")
        pr.eval(AT, 20, 150, expect=KEPT, ctx="inside the grown range")
        pr.eval(AT, 100, 260, expect=WROTE, ctx="overlaps the end")
        pr.eval(AT, 0, 260, expect=KEPT)
        pr.eval(AT, 0, n, expect=WROTE)
        pr.eval(AT, 0, n, expect=KEPT)


def test_decide_and_commit_then_eval(gpu_required, hdr):
    snap = synth.trimaran_snapshot(hdr, 350, 220, seed=8, round_frac=0.2)
    with Pair() as pr:
        pr.both(lambda e: load(e, snap))
        pr.eval(AT, expect=WROTE)

        def same_decisions():
            for a, b in zip(pr.k.best(), pr.r.best()):
                assert np.array_equal(a, b)

        pr.both(lambda e: (e.decide(AT), e.sync()))  # no table is written
        same_decisions()
        pr.eval(AT, expect=KEPT, ctx="after spx_decide")
        pr.both(lambda e: (e.eval_best(AT), e.sync()))  # the argmax reads the kept table
        same_decisions()
        pr.both(lambda e: e.set_option("DECIDE_UNFUSED", 1))  # spx_eval + spx_eval_best
        pr.both(lambda e: (e.decide(AT), e.sync()))
        assert path(pr.k) == KEPT
        same_decisions()
        got, want = pr.k.commit_sequential(AT), pr.r.commit_sequential(AT)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        pr.eval(AT, expect=KEPT, ctx="after spx_commit_sequential")
        got, want = pr.k.commit_sequential(mask_of(ALLOCATABLE, TLP, LVRB)), pr.r.commit_sequential(mask_of(ALLOCATABLE, TLP, LVRB))
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        pr.eval(mask_of(ALLOCATABLE, TLP, LVRB), expect=KEPT, ctx="after spx_commit_sequential with LVRB")


def test_bound_table_is_always_written(gpu_required, hdr):
    import torch
    snap = synth.trimaran_snapshot(hdr, 300, 128, seed=9)
    with Pair() as pr:
        pr.both(lambda e: load(e, snap))
        want = pr.eval(AT, expect=WROTE)[ALLOCATABLE]
        pr.eval(AT, expect=KEPT)
        _, stride, rows = pr.k.score_table(ALLOCATABLE)
        slabs = [torch.full((rows * stride,), 0xAB, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
        pr.k.bind_score_table(ALLOCATABLE, slabs[0].data_ptr(), stride, rows)
        pr.r.bind_score_table(ALLOCATABLE, slabs[1].data_ptr(), stride, rows)
        for i in range(3):  # the caller owns the memory and overwrites it between evaluations
            assert np.array_equal(pr.eval(AT, expect=WROTE, ctx=f"bound {i}")[ALLOCATABLE], want)
            view = slabs[0].view(rows, stride)[:128, :300].cpu().numpy()
            assert np.array_equal(view, want)
            torch.cuda.synchronize()
            for s in slabs:
                s.fill_(0xAB)
            torch.cuda.synchronize()
        pr.both(lambda e: e.bind_score_table(ALLOCATABLE, 0, 0, 0))  # unbind: an engine-owned table again, never written
        assert np.array_equal(pr.eval(AT, expect=WROTE, ctx="unbound")[ALLOCATABLE], want)
        assert np.array_equal(pr.eval(AT, expect=KEPT, ctx="unbound, again")[ALLOCATABLE], want)
        del slabs


def test_option_flips(gpu_required, hdr, oracle):
    snap = synth.trimaran_snapshot(hdr, 520, 300, seed=10, round_frac=0.3)
    with Pair() as pr:
        pr.both(lambda e: load(e, snap))
        pr.eval(AT, expect=WROTE)
        pr.eval(AT, expect=KEPT)
        pr.k.set_option("ALLOC_TABLE_KEEP", 0)
        pr.eval(AT, expect=WROTE, ctx="option off")
        pr.eval(AT, expect=WROTE, ctx="option off, again")
        pr.k.set_option("ALLOC_TABLE_KEEP", 1)
        pr.eval(AT, expect=KEPT, ctx="option on: the rows were written a moment ago")
        pr.both(lambda e: e.force_reference_kernels(TLP))
        check_oracle(oracle, pr.k, snap, pr.eval(AT, expect=KEPT, ctx="reference kernels"), "reference kernels")
        pr.eval(mask_of(ALLOCATABLE, TLP, LVRB), expect=KEPT, ctx="reference kernels, three plugins")
        pr.both(lambda e: e.force_reference_kernels())
        pr.both(lambda e: e.set_option("TLP_AMB_TABLE", 0))
        check_oracle(oracle, pr.k, snap, pr.eval(AT, expect=KEPT, ctx="no ambiguity table"), "no ambiguity table")
        pr.both(lambda e: e.set_option("TLP_AMB_TABLE", 1))
        pr.eval(AT, expect=KEPT)
    # written by the reference kernels, kept under the fast ones
    with Pair() as pr:
        pr.both(lambda e: load(e, snap))
        pr.both(lambda e: e.force_reference_kernels(TLP))
        pr.eval(AT, expect=WROTE)
        pr.both(lambda e: e.force_reference_kernels())
        check_oracle(oracle, pr.k, snap, pr.eval(AT, expect=KEPT), "fast after reference")
    for align in (16, 256):  # the row stride is part of what is recorded
        with Pair({"ROW_ALIGN": align}) as pr:
            pr.both(lambda e: load(e, snap))
            check_oracle(oracle, pr.k, snap, pr.eval(AT, expect=WROTE, ctx=f"align {align}"), f"align {align}")
            check_oracle(oracle, pr.k, snap, pr.eval(AT, expect=KEPT, ctx=f"align {align}"), f"align {align}")
            pr.eval(AT, 5, 290, expect=KEPT, ctx=f"align {align}")


def test_multi_engine_ranks_on_one_device(gpu_required, hdr):
    snap = synth.trimaran_snapshot(hdr, 410, 1001, seed=11)
    with Engine(0) as ref:
        ref.set_option("ALLOC_TABLE_KEEP", 0)
        load(ref, snap)
        ref.eval(AT)
        ref.sync()
        want = {p: ref.all_scores(p) for p in (ALLOCATABLE, TLP)}
    with MultiEngine([0, 0], PEER_COPY) as m:
        m.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])

        def shards_equal(ctx):
            m.sync()
            for r, e in enumerate(m.engines):
                b, end = m.shard(r)
                for p in (ALLOCATABLE, TLP):
                    assert np.array_equal(e.all_scores(p), want[p][b:end]), (ctx, r, p)

        m.eval(AT)
        shards_equal("first")
        assert [path(e) for e in m.engines] == [WROTE, WROTE]
        m.eval(AT)
        shards_equal("second")
        assert [path(e) for e in m.engines] == [KEPT, KEPT]
        # global tables are bound memory: every rank writes its slice on every evaluation, and the all-gather moves those bytes
        for p in (ALLOCATABLE, TLP):
            m.bind_global_table(p)
        for i in range(2):
            m.eval(AT)
            assert [path(e) for e in m.engines] == [WROTE, WROTE], i
            for p in (ALLOCATABLE, TLP):
                m.allgather_table(p)
            m.sync()
            for rank in range(m.size):
                for p in (ALLOCATABLE, TLP):
                    assert np.array_equal(m.global_rows(p, rank), want[p]), (i, rank, p)
