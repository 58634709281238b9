"""The hand-built twin models of tests/ptol_nrt_cases.py and tests/preempt_nrt_cases.py (nodes that list one NUMA id twice) hold their
edge, shown with the literal oracles alone: the Filter's "inconsistent resource accounting" (filter.go:73-77, from
numaresources.go:172-175) occurs in every model, and every model has a cell that a subtraction without the sign test decides
differently — in both dry runs and in both loops.  No GPU."""
import pytest

import preempt_nrt_cases as CC
import preempt_nrt_oracle as CO
import preempt_nrt_seq_oracle as NSO
import ptol_nrt_cases as NC
import ptol_nrt_oracle as NO
import ptol_nrt_seq_oracle as TNSO

ST = NO.ST
FAMILIES = {"toleration": (NC.twin_models, NO.dry_run, TNSO.run), "capacity": (CC.twin_models, CO.dry_run, NSO.run)}


def cells(result):
    return [[(c["status"], c["victims"]) for c in r["cells"]] for r in result]


@pytest.fixture
def unchecked():
    """subtractResourcesFromNUMANodeList without its sign test, as the oracle read it before, for the length of one test"""
    def run(fn):
        NO.CHECK_ACCOUNTING = False
        try:
            return fn()
        finally:
            NO.CHECK_ACCOUNTING = True
    yield run
    assert NO.CHECK_ACCOUNTING


@pytest.mark.parametrize("name", list(NC.TWIN_MODELS))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_error_occurs_and_changes_a_verdict(family, name, unchecked):
    models, dry_run, loop = FAMILIES[family]
    m = models()[name]
    trace = set()
    want = dry_run(m, m["pending"], trace=trace)
    assert "accounting-error" in trace
    old_trace = set()
    old = unchecked(lambda: dry_run(m, m["pending"], trace=old_trace))
    assert "accounting-error" not in old_trace and cells(old) != cells(want)
    steps, old_steps = loop(m, m["pending"]), unchecked(lambda: loop(m, m["pending"]))
    assert cells(steps) != cells(old_steps)
    assert cells(steps)[0] == cells(want)[0]            # the loop's first row sees the tables as uploaded


@pytest.mark.parametrize("family", list(FAMILIES))
def test_each_cell_of_the_full_model(family, unchecked):
    """rows p0 (3 cpus), p1 (2 + 2), p2 (3) x nodes uneven, even, reprieve, duplicate-free"""
    models, dry_run, loop = FAMILIES[family]
    m = models()["twins"]
    C, NF, R = ST["CANDIDATE"], ST["NOT_FIT"], ST["ALL_REPRIEVED"]
    want = cells(dry_run(m, m["pending"]))
    # uneven: the Error at the first refit, no candidate; even: v's release lands on both twins and both rows take them; reprieve: v2's
    # return puts the smaller twin below zero, both stay evicted (p1's second container finds nothing left: not fit); the free twin of
    # the uneven node takes 3 cpus next to v, and 2 + 2 once v is gone
    assert want[0] == [(NF, []), (C, [0]), (C, [1, 0]), (R, [])]
    assert want[1] == [(NF, []), (C, [0]), (NF, []), (C, [0])]
    assert want[2] == want[0]
    old = cells(unchecked(lambda: dry_run(m, m["pending"])))
    assert old[0] == [(R, []), (C, [0]), (C, [0]), (R, [])]      # without the sign test: fits through the uncaught charge, v2 reprieved
    # the loops: p0 picks a node, p1 and p2 meet what it left — a second step lands on a node an earlier row changed
    steps = loop(m, m["pending"])
    picks = [r["pick"][0] for r in steps]
    assert all(p >= 0 for p in picks) and len(set(picks)) == 3
    assert cells(steps)[1] != want[1] or cells(steps)[2] != want[2]
