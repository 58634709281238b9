"""GPU parity (through the C ABI) for SySched (pkg/sysched/sysched.go:234-288).  The arithmetic is integer: every cell of the
normalised uint8 table and of the raw int64 rows is compared with the oracle (tests/sysched_oracle.py, Python sets in the
reference's literal form) at tolerance 0."""
import json
from pathlib import Path

import numpy as np
import pytest

import scheduler_plugins_amd as spx
import sysched_oracle as SO
from scheduler_plugins_amd import objects as O
from scheduler_plugins_amd import synth
from scheduler_plugins_amd.engine import NRT, SYSCHED, TLP, Engine, mask_of

pytestmark = pytest.mark.gpu

G = json.loads((Path(__file__).parent / "golden" / "sysched.json").read_text())
RAW_BUDGET = 256 << 20  # kSyschedRawBudget


def assert_tables(e, snap, want_raw, want_norm, raw_rows=None):
    got = e.all_scores(SYSCHED).astype(np.int64)
    bad = np.argwhere(got != want_norm)
    assert bad.size == 0, f"{len(bad)} normalised cells differ, first {[(int(p), int(n), int(got[p, n]), int(want_norm[p, n])) for p, n in bad[:5]]}"
    for p in (range(len(want_raw)) if raw_rows is None else raw_rows):
        r = e.raw(SYSCHED, int(p))
        assert np.array_equal(r, want_raw[p]), (int(p), np.flatnonzero(r != want_raw[p])[:5])


def load(e, snap):
    e.load_sysched_objects(snap["objects"])


def test_reference_cases_through_the_engine(gpu_required, hdr):
    pr = O.SeccompProfiles([O.seccomp_profile(p["name"], p["namespace"], [{"action": p["action"], "names": p["names"]}]) for p in G["profiles"]])
    k = O.SPO_ANNOTATION
    existing = pr.get_syscalls(O.sysched_pod(annotations={k: G["score"]["existing_pod_annotation"]}))
    pods = [pr.get_syscalls(O.sysched_pod(annotations={k: c["annotation"]})) for c in G["score"]["cases"]] + [pr.get_syscalls(O.sysched_pod())]
    assert pods[2] == frozenset()  # TestScore's SySched has no default profile
    # node 0 = TestScore's "test"; node 1 has no HostSyscalls entry; node 2 hosts the existing pod twice
    hosts, res = [existing, None, existing], [[existing], [], [existing, existing]]
    with Engine(0) as e:
        e.load_sysched_objects(O.build_sysched_objects(hdr, pods, hosts, res))
        raws = np.stack([e.raw(SYSCHED, p) for p in range(3)])
        assert [int(raws[i, 0]) for i in range(2)] == [c["expected"] for c in G["score"]["cases"]]
        assert raws[0].tolist() == [2, 0, 3] and raws[1].tolist() == [0, 0, 0] and (raws[2] == SO.MAX_INT64).all()
        e.eval(mask_of(SYSCHED))
        e.sync()
        got = e.all_scores(SYSCHED)
        assert got[0].tolist() == SO.normalize([2, 0, 3]) == [34, 100, 0]
        assert got[1].tolist() == [100, 100, 100] and got[2].tolist() == [100, 100, 100]  # max == 0; the MaxInt64 row by the wrap
    # TestNormalizeScore's vectors: raw scores 100 / 200 and 0 / 200 from nodes built to produce them
    names = [f"s{i:03d}" for i in range(200)]
    P = frozenset(["p"])
    for scores, expected in ((c["scores"], c["expected"]) for c in G["normalize"]["cases"]):
        hosts = [frozenset(names[:s]) for s in scores]
        with Engine(0) as e:
            e.load_sysched_objects(O.build_sysched_objects(hdr, [P], hosts, [[] for _ in scores]))
            assert e.raw(SYSCHED, 0).tolist() == scores
            e.eval(mask_of(SYSCHED))
            e.sync()
            assert e.scores(SYSCHED, 0).tolist() == expected


@pytest.mark.parametrize("n_nodes,n_pods,seed,profiles", [(257, 1031, 11, 32), (2000, 20000, 12, 24)])
def test_parity_with_oracle(gpu_required, hdr, n_nodes, n_pods, seed, profiles):
    snap = synth.sysched_snapshot(hdr, n_nodes, n_pods, seed=seed, n_profiles=profiles)
    want_raw, want_norm = SO.tables(snap)
    assert snap["n_stale_states"] > 0 and any(h is None for h in snap["host"]) and (snap["pod_set"] == snap["empty_set"]).any()
    with Engine(0) as e:
        load(e, snap)
        u, d = e.sysched_pod_classes()
        assert u + d == n_pods and u <= profiles + 1
        e.eval(mask_of(SYSCHED))
        e.sync()
        assert e.kernel_path(SYSCHED) == 1
        print(f"sysched {n_nodes} x {n_pods}: {e.last_eval_ms():.3f} ms, {u} classes")
        # raw rows: every distinct set once (rows of one set are one launch each; the first pod of every set), all cells
        first = {int(s): p for p, s in reversed(list(enumerate(snap["pod_set"])))}
        assert_tables(e, snap, want_raw, want_norm, raw_rows=sorted(first.values()))
        empty_rows = np.flatnonzero(snap["pod_set"] == snap["empty_set"])
        assert (e.all_scores(SYSCHED, int(empty_rows[0]), int(empty_rows[0]) + 1) == 100).all()
        # a row range (no classes: k_sysched_rows) writes the same bytes
        whole = e.all_scores(SYSCHED)
        lo, hi = n_pods // 3, n_pods // 3 + 37
        e.eval(mask_of(SYSCHED), lo, hi)
        e.sync()
        assert np.array_equal(e.all_scores(SYSCHED, lo, hi), whole[lo:hi])
        e.eval(mask_of(SYSCHED), 5, 6)
        e.sync()
        assert np.array_equal(e.scores(SYSCHED, 5), whole[5])


def test_distinct_sets_take_several_chunks(gpu_required, hdr):
    n_nodes, n_pods = 20000, 3400
    snap = synth.sysched_snapshot(hdr, n_nodes, n_pods, seed=21, n_profiles=16, distinct_pods=True, node_states=24, empty_frac=0.001)
    want_raw, want_norm = SO.tables(snap)
    with Engine(0) as e:
        load(e, snap)
        u, d = e.sysched_pod_classes()
        assert u >= n_pods - 8  # every pod its own set (but the few with the empty set)
        _, stride, _ = e.score_table(SYSCHED)
        per_chunk = RAW_BUDGET // (stride * 4)
        n_sets = snap["objects"].struct.n_sets
        assert n_sets > per_chunk, "the snapshot must not fit one chunk of the raw table"
        e.eval(mask_of(SYSCHED))
        e.sync()
        assert e.kernel_path(SYSCHED) == -(-n_sets // per_chunk) >= 2
        assert_tables(e, snap, want_raw, want_norm, raw_rows=[0, 1, n_pods // 2, n_pods - 1])


def test_zero_maximum_rows_are_all_100(gpu_required, hdr):
    names = [f"s{i}" for i in range(70)]
    A = frozenset(names[:40])
    pods = [A, frozenset(names[:10]), frozenset()]
    hosts = [A, None, frozenset(), A]
    res = [[A, A], [A], [], [A]]
    with Engine(0) as e:
        e.load_sysched_objects(O.build_sysched_objects(hdr, pods, hosts, res))
        e.eval(mask_of(SYSCHED))
        e.sync()
        got = e.all_scores(SYSCHED)
        raw0 = e.raw(SYSCHED, 0)
        assert raw0.tolist() == [SO.score(A, h, r) for h, r in zip(hosts, res)] == [0, 0, 0, 0]
        assert (got[0] == 100).all() and (got[2] == 100).all()
        assert got[1].tolist() == SO.normalize([SO.score(pods[1], h, r) for h, r in zip(hosts, res)])


def feasible_expectation(snap, feas):
    return SO.tables(snap, feasible=feas)


def test_caller_mask_normalises_over_feasible_nodes(gpu_required, hdr):
    n_nodes, n_pods = 700, 90
    snap = synth.sysched_snapshot(hdr, n_nodes, n_pods, seed=31, n_profiles=12, empty_frac=0.03)
    raw, _ = SO.tables(snap)
    feas = np.random.default_rng(3).random((n_pods, n_nodes)) < 0.5
    feas[2] = False                      # no feasible node
    feas[3] = False
    feas[3, 17] = True                   # exactly one
    row = int(np.flatnonzero(snap["pod_set"] != snap["empty_set"])[5])
    feas[row] = True
    feas[row, int(np.argmax(raw[row]))] = False  # the global maximum sits on an infeasible node
    assert raw[row][feas[row]].max() < raw[row].max()
    _, want = feasible_expectation(snap, feas)
    with Engine(0) as e:
        load(e, snap)
        e.upload_feasible_mask(feas.astype(np.uint8))
        e.eval(mask_of(SYSCHED))
        e.sync()
        got = e.all_scores(SYSCHED).astype(np.int64)
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
        assert not got[~feas].any()
        e.upload_feasible_mask(None)
        e.eval(mask_of(SYSCHED))
        e.sync()
        assert np.array_equal(e.all_scores(SYSCHED).astype(np.int64), SO.tables(snap)[1])


def test_nrt_in_the_mask_normalises_over_feasible_nodes(gpu_required, hdr, oracle):
    n_nodes, n_pods = 600, 80
    ns = synth.nrt_snapshot(hdr, n_nodes, n_pods, seed=41)
    snap = synth.sysched_snapshot(hdr, n_nodes, n_pods, seed=42, n_profiles=10)
    params = O.nrt_params(hdr, O.Resources(), "LeastAllocated")
    osnap = oracle.Snapshot(ns["nodes"], ns["pods"], rc=ns["rc"], nrt=ns["nrt"], nrt_params=params)
    feas = osnap.filter_rows(NRT) == 0
    raw, _ = SO.tables(snap)
    moved = [p for p in range(n_pods) if feas[p].any() and raw[p].max() < SO.MAX_INT64 and raw[p][feas[p]].max() < raw[p].max()]
    assert moved, "some row's global maximum must sit on a node the Filter rejects"
    assert (~feas).any() and feas.any()
    _, want = feasible_expectation(snap, feas)
    with Engine(0) as e:
        e.load_nrt_objects(ns["nodes"], ns["nrt"], ns["rc"], ns["pods"], params)
        load(e, snap)
        e.eval(mask_of(NRT, SYSCHED))
        e.sync()
        assert np.array_equal(e.all_status(NRT) == 0, feas)
        got = e.all_scores(SYSCHED).astype(np.int64)
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
        # the argmax refuses a SySched table normalised under another Filter set
        e.eval(mask_of(SYSCHED))
        e.eval(mask_of(NRT))
        with pytest.raises(spx.SpxError):
            e.eval_best(mask_of(NRT, SYSCHED))


@pytest.mark.parametrize("n_changed", [1, 7, None])
def test_node_delta_equals_full_reupload(gpu_required, hdr, n_changed):
    n_nodes, n_pods = 900, 120
    a = synth.sysched_snapshot(hdr, n_nodes, n_pods, seed=51, n_profiles=8, stale_frac=0.1)
    b = synth.sysched_snapshot(hdr, n_nodes, n_pods, seed=52, n_profiles=8, stale_frac=0.1)  # same profiles' shapes, other nodes
    idx = np.arange(n_nodes) if n_changed is None else np.random.default_rng(1).choice(n_nodes, n_changed, replace=False)
    with Engine(0) as e, Engine(0) as ref:
        fa, fb = e.flatten_sysched(a["objects"]), e.flatten_sysched(b["objects"])
        assert fa["W"] == fb["W"]
        # the target: table a with the rows idx taken from table b
        mixed = {k: v.copy() for k, v in fa["nodes"].items()}
        rows = Engine.sysched_node_rows(fb["nodes"], idx)
        keep = np.ones(n_nodes, bool)
        keep[idx] = False
        bits, cnt, ptr = [], [], [0]
        for n in range(n_nodes):
            src = fa["nodes"] if keep[n] else fb["nodes"]
            j0, j1 = src["stale_ptr"][n], src["stale_ptr"][n + 1]
            bits += list(src["stale_bit"][j0:j1]); cnt += list(src["stale_count"][j0:j1]); ptr.append(len(bits))
        mixed["host_bits"][:, idx] = fb["nodes"]["host_bits"][:, idx]
        for c in ("present", "n_resident", "resident_missing"):
            mixed[c][idx] = fb["nodes"][c][idx]
        mixed["stale_ptr"], mixed["stale_bit"], mixed["stale_count"] = np.array(ptr, np.int32), np.array(bits, np.int32), np.array(cnt, np.int32)
        ref.upload_sysched_nodes(mixed)
        ref.upload_sysched_pods(fa["pods"])
        ref.eval(mask_of(SYSCHED))
        ref.sync()
        e.upload_sysched_nodes(fa["nodes"])
        e.upload_sysched_pods(fa["pods"])
        e.eval(mask_of(SYSCHED))
        e.sync()
        before = e.all_scores(SYSCHED)
        e.update_sysched_nodes(idx, rows)
        with pytest.raises(spx.SpxError):  # tables evaluated before the delta are stale
            e.scores(SYSCHED, 0)
        e.eval(mask_of(SYSCHED))
        e.sync()
        assert np.array_equal(e.all_scores(SYSCHED), ref.all_scores(SYSCHED))
        assert not np.array_equal(e.all_scores(SYSCHED), before)
        for p in (0, 17, n_pods - 1):
            assert np.array_equal(e.raw(SYSCHED, p), ref.raw(SYSCHED, p))


def test_eval_best_and_decide_with_tlp(gpu_required, hdr, oracle):
    n_nodes, n_pods = 800, 150
    ts = synth.trimaran_snapshot(hdr, n_nodes, n_pods, seed=61, round_frac=0.1)
    snap = synth.sysched_snapshot(hdr, n_nodes, n_pods, seed=62, n_profiles=9, empty_frac=0.02)
    _, sy = SO.tables(snap)
    w_tlp, w_sy = 3, 5
    with Engine(0) as e:
        e.load_trimaran_objects(ts["nodes"], ts["rc"], ts["pods"], ts["metrics"], ts["assigned"])
        load(e, snap)
        osnap = oracle.Snapshot(ts["nodes"], ts["pods"], rc=ts["rc"], metrics=ts["metrics"], assigned=ts["assigned"], tlp_params=e.tlp_params)
        _, tlp = osnap.score_rows(TLP)
        total = w_tlp * tlp.astype(np.int64) + w_sy * sy
        best = total.max(1)
        e.set_plugin_weights({TLP: w_tlp, SYSCHED: w_sy})
        for how in ("eval_best", "decide"):
            if how == "eval_best":
                e.eval(mask_of(TLP, SYSCHED))
                e.eval_best(mask_of(TLP, SYSCHED))
            else:
                e.decide(mask_of(TLP, SYSCHED))
            e.sync()
            node, score, ties, feas = e.best()
            assert np.array_equal(score, best), how
            assert np.array_equal(node, total.argmax(1)), how  # the lowest index among the ties
            assert np.array_equal(ties, (total == best[:, None]).sum(1)), how
            assert (feas == n_nodes).all()


def test_commit_sequential_rejects_sysched(gpu_required, hdr):
    ts = synth.trimaran_snapshot(hdr, 64, 16, seed=71)
    snap = synth.sysched_snapshot(hdr, 64, 16, seed=72, n_profiles=4)
    with Engine(0) as e:
        e.load_trimaran_objects(ts["nodes"], ts["rc"], ts["pods"], ts["metrics"], ts["assigned"])
        load(e, snap)
        with pytest.raises(spx.SpxError):
            e.commit_sequential(mask_of(TLP, SYSCHED))
        with pytest.raises(spx.SpxError):
            e.commit_sequential(mask_of(SYSCHED))
