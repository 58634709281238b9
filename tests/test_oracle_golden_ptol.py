"""The literal oracle of PreemptionToleration (tests/ptol_oracle.py) against the reference's own tables, transcribed as data in
tests/golden/preemption_toleration.json: parsePreemptionTolerationPolicy's five cases, ExemptedFromPreemption's twelve, and the eight
scenarios of the integration test (one node, one victim candidate: preempted or tolerated)."""
import pytest

import ptol_cases as TC
import ptol_oracle as TO

G = TC.golden()


def test_the_file_holds_the_tables_it_is_named_for():
    assert (len(G["policy"]), len(G["exempted"]), len(G["integration"])) == (5, 12, 8)
    assert G["annotation_keys"] == {"minimum_preemptable_priority": TO.ANNOTATION_MIN, "toleration_seconds": TO.ANNOTATION_TOLERATION}


@pytest.mark.parametrize("case", G["policy"], ids=lambda c: c["source"])
def test_parse_policy(case):
    got = TO.parse_policy(case["priority_class"])
    if case["error"] is not None:
        assert got is None and "invalid syntax" in case["error"]
    else:
        assert got == (case["minimum_preemptable_priority"], case["toleration_seconds"])


@pytest.mark.parametrize("case", G["exempted"], ids=lambda c: c["source"])
def test_exempted_from_preemption(case):
    victim = {"pc": TC.GOLDEN_CLASS, "prio": case["victim_priority"], "scheduled_at": TC.golden_scheduled_at(case["victim_scheduled_at_offset_s"])}
    pre = {"prio": case["preemptor_priority"], "never": case["preempt_never"]}
    classes = TC.golden_class(case["priority_class"])
    if case["error"] is not None:
        with pytest.raises(TO.ClassNotFound):
            TO.exempted(classes, victim, pre, TC.GOLDEN_NOW)
    else:
        assert TO.exempted(classes, victim, pre, TC.GOLDEN_NOW)[0] is case["want"]


@pytest.mark.parametrize("case", G["integration"], ids=lambda c: c["source"])
def test_integration_scenarios(case):
    """"the preemptor gets scheduled and the victim is gone" = node-a is a candidate whose one victim is the victim candidate and is
    picked; "the victim stays and the preemptor is not scheduled" = no victims on the only node, nothing picked"""
    m = TC.golden_integration_model(case)
    (row,) = TO.dry_run(m, m["pending"])
    (cell,) = row["cells"]
    if case["can_tolerate"]:
        assert (cell["status"], cell["victims"], row["pick"][0]) == (TO.ST["NO_VICTIMS"], [], -1)
    else:
        assert (cell["status"], cell["victims"], row["pick"][0]) == (TO.ST["CANDIDATE"], [0], 0)
