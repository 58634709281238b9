"""The reference's own tables for the preemption dry run (tests/golden/capacity_preemption.json: TestDryRunPreemption, TestPostFilter,
TestPodEligibleToPreemptOthers of pkg/capacityscheduling/capacity_scheduling_test.go) through the literal oracle.  CPU only.

One entry of the tables cannot be reproduced by any literal reading of the code under test: the `want` of TestDryRunPreemption's
"cross-namespace preemption" lists t1-p3 alone, but the test never looks at `want`'s victims — its loop compares each result with itself
(`for i, c := range got { gocmp.Diff(c.Victims(), got[i].Victims()) }`, :790-797) and so checks the number of candidates only.  By the
code, t1-p2 and t1-p3 of ns2 are both potential victims (:572 has no priority condition), and each reprieve puts the pod into ns2's
empty `pods` set and grows Used by 50 (addPodIfNotPresent), after which sum(Used) + 50 = 250 exceeds sum(Min) = 200 (:646): both stay
victims.  The test below asserts what the reference's test asserts for that case, the count and the node, and pins the literal result."""
import pytest

import preempt_cases as PC
import preempt_oracle as PO

G = PC.golden()
WRITTEN_BUT_NEVER_COMPARED = {"cross-namespace preemption": ["t1-p2", "t1-p3"]}


@pytest.mark.parametrize("case", G["dry_run"], ids=lambda c: c["name"])
def test_dry_run_preemption(case):
    m = PC.golden_model(case)
    out = PO.dry_run(m, m["pending"])[0]
    got = [{"node": case["node"]["name"], "victims": [m["nodes"][0]["pods"][i]["key"] for i in c["victims"]], "num_pdb_violations": c["n_violations"]}
           for c in out["cells"] if c["status"] == PO.ST["CANDIDATE"]]
    assert len(got) == len(case["want"]) and [g["node"] for g in got] == [w["node"] for w in case["want"]]
    assert [g["num_pdb_violations"] for g in got] == [w["num_pdb_violations"] for w in case["want"]]
    if case["name"] in WRITTEN_BUT_NEVER_COMPARED:
        assert sorted(got[0]["victims"]) == WRITTEN_BUT_NEVER_COMPARED[case["name"]] != case["want"][0]["victims"]
    else:
        assert [sorted(g["victims"]) for g in got] == [w["victims"] for w in case["want"]]


@pytest.mark.parametrize("case", G["post_filter"], ids=lambda c: c["name"])
def test_post_filter_nominates_the_node(case):
    m = PC.golden_model(case)
    node, n_candidates, n_ties, _ = PO.dry_run(m, m["pending"])[0]["pick"]
    assert [case["node"]["name"]][node] == case["want_nominated_node"] and (n_candidates, n_ties) == (1, 1)


@pytest.mark.parametrize("case", G["eligible"], ids=lambda c: c["name"])
def test_pod_eligible_to_preempt_others(case):
    m = PC.golden_model(case)
    pre = m["pending"][0]
    in_eq = pre["req"]  # the tests overwrite the PreFilter state with podReq (:999-1003)
    nominated = 0 if case["pod"]["nominated_node"] == case["node"]["name"] else -1
    assert PO.pod_eligible_to_preempt_others(m, pre, in_eq, case["pod"]["preempt_never"], nominated, case["nominated_unresolvable"]) is case["expected"]
