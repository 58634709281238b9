"""The literal oracle of CapacityScheduling's sequential preemption loop with NRT's Filter in the refit (tests/preempt_nrt_seq_oracle.py),
on the CPU: what it must agree with, how far its answer is from the three runs the tree already had (the frozen NRT batch, the fit-only
loop, the loop with the preemption mode off) on the models the GPU suite uses, and the two constructed models: the cross-node one, which
pins what only this loop has, and the second visit, which pins T5.  The last test is about the ABI: it needs the
library, no GPU."""
import pytest

import preempt_nrt_cases as CC
import preempt_nrt_oracle as CO
import preempt_nrt_seq_cases as NSC
import preempt_nrt_seq_oracle as NSO
import preempt_seq_oracle as SO
import scheduler_plugins_amd as spx
from test_oracle_ptol_nrt import without_nrt


@pytest.mark.parametrize("kind,name", [("shape", "63x65"), ("shape", "lists"), ("retuned", "12x40")])
def test_one_row_is_the_dry_run(kind, name):
    m = NSC.model(kind, name)
    mask = CC.node_mask(1, len(m["nodes"]), 5)
    for pre in m["pending"][:8]:
        for mode in (True, False):
            assert NSO.run(m, [pre], mode=mode) == CO.dry_run(m, [pre], None, mode)
        assert NSO.run(m, [pre], mask) == CO.dry_run(m, [pre], mask)


def test_without_any_nrt_it_is_the_fit_only_loop():
    m = without_nrt(NSC.model("retuned", "63x65"))
    counters, plain = {}, {}
    want = SO.run(m, m["pending"], counters=plain)
    assert plain["applied"] > 1 and plain["used_moved"] > 0
    for mode in (True, False):
        assert NSO.run(m, m["pending"], mode=mode, counters=counters) == want
        assert counters == plain


def test_the_loop_differs_from_the_three_runs_the_tree_had():
    """rows that end on another node or with other victims than in the frozen NRT batch, the fit-only loop and the loop with mode off,
    and how often a quota's Used moved; zero only where preempt_nrt_seq_cases.ZERO says so"""
    for kind, name in NSC.MODELS:
        seq, counters = NSC.expected(kind, name)
        counts = {"frozen": NSC.differing_rows(seq, NSC.frozen(kind, name)), "fit_only": NSC.differing_rows(seq, NSC.fit_only(kind, name)),
                  "mode_off": NSC.differing_rows(seq, NSC.expected(kind, name, mode=False)[0]), "used_moved": counters["used_moved"]}
        print(kind, name, "rows", len(seq), counts, counters)
        zero = NSC.ZERO.get((kind, name), set())
        assert {k for k, v in counts.items() if v == 0} == zero, (kind, name, counts)


def test_the_cross_node_model():
    """the Filter decides who leaves node A, that moves quota 0's Used, and that decides the cell on node B, which no step touched:
    four paths, four answers"""
    m, mask = NSC.cross_node_model()
    p0, p1 = m["pending"]
    assert CO.NO.pod_qos(p0) == CO.NO.pod_qos(m["nodes"][0]["pods"][0]) == CO.NO.GUARANTEED
    want = NSC.CROSS_NODE
    cells = lambda rows: (NSC.end(rows[0], NSC.A), NSC.end(rows[1], NSC.B))
    counters = {}
    assert cells(NSO.run(m, m["pending"], mask, counters=counters)) == want["loop"]
    assert (counters["used_moved"], counters["over_min_flips"]) == (1, 1)
    assert cells(SO.run(m, m["pending"], mask)) == want["fit_only"]
    assert cells(NSO.run(m, m["pending"], mask, mode=False)) == want["mode_off"]
    assert cells(CO.dry_run(m, m["pending"], mask)) == want["frozen"]
    assert len({str(on_b) for _, on_b in want.values()}) == 4


def test_the_second_visit_pins_t5():
    m = NSC.second_visit_model()
    assert not m["quotas"]
    want = NSC.SECOND_VISIT
    assert [NSC.row_end(r) for r in NSO.run(m, m["pending"])] == want["loop"]
    assert NSC.row_end(SO.run(m, m["pending"])[1]) == want["fit_only_p1"]
    assert NSC.row_end(CO.dry_run(m, m["pending"])[1]) == want["frozen_p1"]
    assert [NSC.row_end(r) for r in NSO.run(m, m["pending"], mode=False)] == want["mode_off"]


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_header_declares_the_loop_and_a_null_engine_is_refused():
    hdr = spx.header()
    assert "spx_preempt_nrt_sequential" in hdr.protos
    assert len(hdr.protos["spx_preempt_nrt_sequential"][1]) == 6
    assert spx.lib().spx_abi_version() == 1
    assert spx.lib().spx_preempt_nrt_sequential(None, None, 0, None, None, 1) == hdr.consts["SPX_ERR_ARG"]
