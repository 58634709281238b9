"""The literal oracle of CapacityScheduling's sequential preemption loop (tests/preempt_seq_oracle.py), on the CPU: what it must agree
with, each rule of the state model (DESIGN.md 3.9f, T1-T4 and the quota coupling) seen in a later row's cell of a hand-built model, and
how far the loop's answer is from the frozen batch's on the models the GPU suite uses.  The last test is about the ABI: it needs the
library, no GPU."""
import pytest

import preempt_cases as PC
import preempt_oracle as PO
import preempt_seq_cases as SC
import preempt_seq_oracle as SO
import scheduler_plugins_amd as spx


@pytest.mark.parametrize("kind,name", [("plain", "1x1"), ("plain", "63x65"), ("retuned", "63x65")])
def test_one_row_is_the_dry_run(kind, name):
    m = SC.model(kind, **(SC.PLAIN if kind == "plain" else SC.RETUNED)[name])
    mask = PC.node_mask(1, len(m["nodes"]), 5)
    for pre in m["pending"][:12]:
        assert SO.run(m, [pre]) == PO.dry_run(m, [pre])
        assert SO.run(m, [pre], mask) == PO.dry_run(m, [pre], mask)


# ---------------------------------------------------------------------------------------------------------------- the hand-built models
@pytest.mark.parametrize("name", list(SC.HAND))
def test_each_effect_shows_in_a_later_rows_cell(name):
    m, mask, eligible, what = SC.HAND[name]()
    frozen = PO.dry_run(m, m["pending"], mask)
    counters = {}
    seq = SO.run(m, m["pending"], mask, eligible, counters, frozen)
    cell = lambda res: (res[what["row"]]["cells"][what["node"]]["status"], res[what["row"]]["cells"][what["node"]]["victims"])
    assert cell(seq) == what["seq"]
    if "frozen" in what:
        assert cell(frozen) == what["frozen"]
    for k in SO.COUNTERS:
        if k in what:
            assert counters[k] == what[k], (k, counters)


def test_used_moves_only_with_the_in_set_bit():
    with_bit, without = SC.HAND["t1_in_set"](), SC.HAND["t1_not_in_set"]()
    cells = []
    for m, mask, eligible, what in (with_bit, without):
        counters = {}
        seq = SO.run(m, m["pending"], mask, eligible, counters, PO.dry_run(m, m["pending"], mask))
        assert seq[0]["cells"][0]["victims"] == [0]  # the same eviction in both
        cells.append((counters["used_moved"], seq[1]["cells"][1]["status"]))
    assert cells == [(1, SC.NOV), (0, SC.CAND)]


def test_another_namespaces_nomination_counts_only_while_its_quota_is_not_over_min():
    res = {}
    for name in ("t2_other_namespace_not_over_min", "t2_other_namespace_over_min"):
        m, mask, eligible, what = SC.HAND[name]()
        seq = SO.run(m, m["pending"], mask, eligible)
        assert seq[0]["pick"][0] == 0 and seq[0]["cells"][0]["victims"] == [0]  # P0 is nominated to A in both
        res[name] = seq[1]["cells"][1]["status"]
    assert res == {"t2_other_namespace_not_over_min": SC.CAND, "t2_other_namespace_over_min": SC.ALLREP}


# ---------------------------------------------------------------------------------------------------------------- the generated models
def test_the_retuned_models_reach_the_quota_coupling():
    """every counter non-zero somewhere; cells that differ from the frozen batch on nodes no step touched on every shape from 63 x 65 up"""
    seen = {k: 0 for k in SO.COUNTERS}
    for name, kw in SC.RETUNED.items():
        seq, counters = SC.expected("retuned", **kw)
        differ = SC.differing_rows(seq, SC.frozen("retuned", **kw))
        print(name, "rows that end differently:", differ, "of", len(seq), counters, "statuses", sorted(SC.statuses(seq)))
        assert differ >= 1, name
        if name != "12x40":
            assert counters["untouched_cells_differ"] > 0, name
            assert len(SC.statuses(seq)) >= 6, name
        for k in seen:
            seen[k] += counters[k]
    assert all(v > 0 for v in seen.values()), seen


def test_the_plain_generator_differs_from_the_frozen_batch_too():
    for name, kw in SC.PLAIN.items():
        seq, counters = SC.expected("plain", **kw)
        differ = SC.differing_rows(seq, SC.frozen("plain", **kw))
        print(name, "rows that end differently:", differ, "of", len(seq), counters)
        assert differ >= 1 or name == "1x1", name


def test_the_side_tables_precondition_holds_on_the_generated_models():
    """PreFilter's sums walk the nominated pods of present nodes; the quota table's list holds them all.  The one-row GPU test needs both
    to describe the same pods on its shape"""
    m = SC.model("retuned", **SC.RETUNED["63x65"])
    assert not any(nd["nominated"] for nd in m["nodes"] if not nd["present"])
    assert sum(len(nd["nominated"]) for nd in m["nodes"]) > 0


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_header_declares_the_entry_points_and_null_arguments_are_refused():
    hdr = spx.header()
    for name, n_args in (("spx_preempt_sequential", 5), ("spx_upload_preempt_nominated_quota", 2), ("spx_flatten_preempt_nominated_quota", 9)):
        assert name in hdr.protos and len(hdr.protos[name][1]) == n_args, name
    assert "spx_preempt_nominated_quota_soa" in hdr.structs
    assert spx.lib().spx_preempt_sequential(None, None, 0, None, None) == hdr.consts["SPX_ERR_ARG"]
    assert spx.lib().spx_upload_preempt_nominated_quota(None, None) == hdr.consts["SPX_ERR_ARG"]
