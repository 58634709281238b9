"""The literal oracle of CapacityScheduling's dry run with NRT's Filter in the refit (tests/preempt_nrt_oracle.py), CPU only: the whole
walk against preempt_oracle where no node has an NRT, what the seeded generator's largest GPU shape holds, and the constructed cells."""
import pytest

import preempt_cases as PC
import preempt_nrt_cases as CC
import preempt_nrt_oracle as CO
import preempt_oracle as PO
from test_oracle_ptol_nrt import without_nrt

ST = PO.ST


def test_without_any_nrt_the_oracle_is_preempt_oracles():
    """on the reference's tables (tests/golden/capacity_preemption.json) and on a seeded snapshot, in both modes"""
    g = PC.golden()
    models = [PC.golden_model(case) for case in g["dry_run"] + g["post_filter"]] + [CC.model(**CC.SHAPES["65x63"])]
    for m in models:
        bare = without_nrt(m)
        want = PO.dry_run(m, m["pending"])
        assert CO.dry_run(bare, bare["pending"], mode=True) == want
        assert CO.dry_run(bare, bare["pending"], mode=False) == want
    assert {c["status"] for r in want for c in r["cells"]} >= {ST[k] for k in ("CANDIDATE", "NO_VICTIMS", "NOT_FIT", "QUOTA", "ALL_REPRIEVED")}


def again_then_kept_by_f(log):
    """a pod taken for the quota while the stack is not empty, and a later reprieve of the cell that F alone decides"""
    seen = False
    for what in log:
        if what[0] == "again" and what[2] > 0:
            seen = True
        elif what[0] == "kept-by-F" and seen:
            return True
    return False


def test_the_largest_gpu_shape_holds_every_way_the_walk_and_the_filter_can_go():
    """the condition on the generator: with preemption mode on, the oracle's walk over the largest shape the GPU tests run takes each of
    these at least once"""
    m = CC.model(**CC.LARGEST)
    trace, events = set(), {}
    want = CO.dry_run(m, m["pending"], None, True, trace, events)
    assert want == CC.expected(**CC.LARGEST)
    plain = PO.dry_run(m, m["pending"])
    pairs = [(a, b) for r, q in zip(want, plain) for a, b in zip(r["cells"], q["cells"])]
    count = lambda pred: sum(1 for log in events.values() if pred(log))
    assert count(lambda log: ("not-fit-by-F",) in log) >= 1  # NOT_FIT by F only
    assert sum(a["status"] == ST["NOT_FIT"] and b["status"] == ST["QUOTA"] for a, b in pairs) >= 1  # fit-only calls it QUOTA, F ends it at :607
    assert count(lambda log: ("quota",) in log and ("f-passed",) in log) >= 1  # a QUOTA cell in which F passed
    assert count(lambda log: any(w[0] == "kept-by-F" for w in log)) >= 1  # a victim NodeResourcesFit alone would reprieve
    assert count(again_then_kept_by_f) >= 1
    kinds = set()
    for p in m["pending"]:
        in_eq, _ = PO.prefilter_state(m, p)
        kinds.add("none" if in_eq is None else "over" if PO.used_over_min_with(m["quotas"][p["ns"]], in_eq) else "under")
    assert kinds == {"none", "over", "under"}
    assert trace >= {"nothing-to-add", "exceeds", "stale", "no-nrt", "exempt", "not-single", "not-single/simulated", "empty-stack", "scope-pod", "scope-container",
                     "init-container-fails"}
    assert {len(p["containers"]) + len(p["init_containers"]) for p in m["pending"]} >= {1, 8}
    assert {len(n["nrt"]["zones"]) for n in m["nodes"] if n["nrt"]} == {1, 2, 8}
    assert {c["status"] for r in want for c in r["cells"]} == set(ST.values())
    # and the two dry runs differ in both directions, and in the pick
    assert any(a["status"] == ST["NOT_FIT"] and b["status"] == ST["CANDIDATE"] for a, b in pairs)
    assert any(a["status"] == ST["CANDIDATE"] and set(a["victims"]) > set(b["victims"]) for a, b in pairs)
    assert any(r["pick"][:3] != q["pick"][:3] for r, q in zip(want, plain))


def test_mode_disabled_is_the_ordinary_filter_and_differs():
    m = CC.model(**CC.LARGEST)
    on, off = CC.expected(**CC.LARGEST), CC.expected(mode=False, **CC.LARGEST)
    assert on != off
    trace = set()
    CO.dry_run(m, m["pending"][:8], None, False, trace)
    assert not trace & {"nothing-to-add", "exceeds", "not-single/simulated"}  # no simulation ever runs


@pytest.mark.parametrize("name", list(CC.DIRECTIONS))
def test_the_constructed_cells(name):
    m, with_filter, fit_only = CC.DIRECTIONS[name]
    events = {}
    c = CO.dry_run(m, m["pending"], events=events)[0]["cells"][0]
    assert (c["status"], c["victims"]) == with_filter
    c = PO.dry_run(m, m["pending"])[0]["cells"][0]
    assert (c["status"], c["victims"]) == fit_only
    log = events[(0, 0)]
    assert {"kept-victim": ("kept-by-F", 0) in log, "fits-by-totals-only": ("not-fit-by-F",) in log, "not-fit-before-quota": ("not-fit-by-F",) in log,
            "again-pod-on-the-stack": again_then_kept_by_f(log) and ("again", 1, 1) in log}[name]
    if name == "again-pod-on-the-stack":  # the pod taken for the quota is what fails b's Filter: without preemption mode nobody is on the stack
        c = CO.dry_run(m, m["pending"], mode=False)[0]["cells"][0]
        assert (c["status"], c["victims"]) == fit_only
