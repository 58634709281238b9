"""The literal oracle of the sequential preemption loop with NRT's Filter in the refit (tests/ptol_nrt_seq_oracle.py), on the CPU: what
it must agree with, how far its answer is from the three runs the tree already had (the frozen NRT batch, the fit-only loop, the loop
with the preemption mode off) on the models the GPU suite uses, and the constructed second visit that pins T5.  The
last test is about the ABI: it needs the library, no GPU."""
import pytest

import ptol_nrt_cases as NC
import ptol_nrt_oracle as NO
import ptol_nrt_seq_cases as NSC
import ptol_nrt_seq_oracle as NSO
import ptol_seq_oracle as SO
import scheduler_plugins_amd as spx
from test_oracle_ptol_nrt import without_nrt


@pytest.mark.parametrize("name", ["1x1", "63x65", "lists"])
def test_one_row_is_the_dry_run(name):
    m = NC.model(**NC.SHAPES[name])
    mask = NC.node_mask(1, len(m["nodes"]), 5)
    for pre in m["pending"][:8]:
        for mode in (True, False):
            assert NSO.run(m, [pre], mode=mode) == NO.dry_run(m, [pre], None, mode)
        assert NSO.run(m, [pre], mask) == NO.dry_run(m, [pre], mask)


def test_without_any_nrt_it_is_the_fit_only_loop():
    m = without_nrt(NC.model(**NC.SHAPES["65x63"]))
    counters, plain = {}, {}
    want = SO.run(m, m["pending"], counters=plain)
    for mode in (True, False):
        assert NSO.run(m, m["pending"], mode=mode, counters=counters) == want
        assert counters == plain and counters["applied"] > 1


def test_a_list_of_preempt_never_rows_is_the_frozen_batch():
    m = NC.model(**NC.SHAPES["63x65"])
    pres = [dict(p, never=True) for p in m["pending"]]
    want = NO.dry_run(m, pres)
    assert NSO.run(m, pres) == want  # nothing moves
    assert any(r["pick"][0] >= 0 for r in want)


def test_the_loop_differs_from_the_three_runs_the_tree_had_on_every_shape():
    """rows that end on another node or with other victims than in the frozen NRT batch, the fit-only loop and the loop with mode off"""
    for name, kw in NC.SHAPES.items():
        if name == "1x1":
            continue
        seq, counters = NSC.expected(**kw)
        counts = (NSC.differing_rows(seq, NC.expected(**kw)), NSC.differing_rows(seq, NSC.fit_only(**kw)), NSC.differing_rows(seq, NSC.expected(mode=False, **kw)[0]))
        print(name, "rows", len(seq), "vs frozen NRT batch / fit-only loop / mode off:", counts, counters)
        assert all(c >= 1 for c in counts), (name, counts)


def test_the_second_visit_pins_t5():
    m = NSC.second_visit_model()
    p0, p1 = m["pending"]
    assert (NO.pod_qos(p0), NO.pod_qos(m["nodes"][0]["pods"][1])) == (NO.GUARANTEED, NO.GUARANTEED)
    want = NSC.SECOND_VISIT
    assert [NSC.end(r) for r in NSO.run(m, m["pending"])] == want["loop"]
    assert NSC.end(SO.run(m, m["pending"])[1]) == want["fit_only_p1"]
    assert NSC.end(NO.dry_run(m, m["pending"])[1]) == want["frozen_p1"]
    assert [NSC.end(r) for r in NSO.run(m, m["pending"], mode=False)] == want["mode_off"]


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_header_declares_the_loop_and_a_null_engine_is_refused():
    hdr = spx.header()
    assert "spx_preempt_toleration_nrt_sequential" in hdr.protos
    assert len(hdr.protos["spx_preempt_toleration_nrt_sequential"][1]) == 9
    assert spx.lib().spx_abi_version() == 1
    assert spx.lib().spx_preempt_toleration_nrt_sequential(None, None, 0, None, None, None, 0, None, 1) == hdr.consts["SPX_ERR_ARG"]
