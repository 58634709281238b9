"""Hand-typed golden tables against what tests/golden/verify_hand_typed.py verified, field by field, in the reference's Go sources.  The
verification runs where a reference checkout is at hand and records each check's item count and each module's digest in
tests/golden/hand_typed_verified.json; these tests hold the modules to that record, so a table edited since fails here until it is
verified again (`python tests/golden/verify_hand_typed.py REFERENCE_CHECKOUT --record`)."""
import json
import sys
from pathlib import Path

GOLDEN = Path(__file__).parent / "golden"


def _verified(*modules):
    """the recorded check counts, after asserting that every named module is the one that was verified"""
    sys.path.insert(0, str(GOLDEN))
    import verify_hand_typed
    rec = json.loads((GOLDEN / "hand_typed_verified.json").read_text())
    for m in modules:
        assert verify_hand_typed.table_digest(m) == rec["tables"][m], f"{m}.py is not the table verified against the Go sources"
    return rec["checks"]


def test_allocatable_table_agrees_with_the_go_source():
    checks = _verified("allocatable")
    assert checks["check_allocatable"] == 14


def test_trimaran_lroc_peaks_tables_agree_with_the_go_sources():
    """trimaran.py COMPUTE_SCORE + MU_SIGMA (17 rows), lroc.py's Beta-distribution tables (10 rows), network.py's Score and Filter cases (11), peaks.py's power model and
    NormalizeScore cases — verified against analysis_test.go, resourcestats_test.go, beta_test.go, peaks_test.go"""
    checks = _verified("trimaran", "lroc", "network", "nrt_helpers", "peaks")
    assert checks["check_trimaran"] == 17
    assert checks["check_trimaran_score_cases"] == 10
    assert checks["check_lroc"] == 10
    assert checks["check_lroc_compute_risk"] == 7
    assert checks["check_network"] == 11
    assert checks["check_nrt_helpers"] == 44
    assert checks["check_nrt_helpers_pods"] == 22
    assert checks["check_nrt_helpers_numa_lists"] == 11
    assert checks["check_peaks"] == 10


def test_round5_tables_agree_with_the_go_sources():
    """what round 4's review listed as still hand-typed only and round 5 re-read: trimaran.py's STATS_* (TestCreateResourceStats), lroc.py's
    GetResourceLimits / GetNodeRequestsAndLimits tables and Score case (the straight-line fixture code of resourcestats_test.go read by a
    small statement reader), nrt_helpers.py's ONLY_NON_NUMA_ZONES and the two OVER_RESERVE flows (straight-line tests, regular expressions)"""
    checks = _verified("trimaran", "lroc", "nrt_helpers")
    assert checks["check_trimaran_stats"] == 10
    assert checks["check_lroc_resource_tables"] == 9
    assert checks["check_nrt_helpers_zones_and_over_reserve"] == 4


def test_preemption_and_integration_tables_agree_with_the_go_sources():
    """the last three hand-typed files: nrt_preemption.py (TestGetNRTPostPodsEviction: fixtures, every case's victims / placement / error / expected zones),
    nrt_preemption_flow.py (TestFilter_PreemptionFlow: the seven straight-line sub-tests read as statements) and integration.py (the five integration tests'
    metrics literals, node and pod quantities, expected placements)"""
    checks = _verified("nrt_preemption", "nrt_preemption_flow", "integration")
    assert checks["check_nrt_preemption"] == 10
    assert checks["check_nrt_preemption_flow"] == 10
    assert checks["check_integration"] == 6


def test_every_hand_typed_module_is_recorded():
    sys.path.insert(0, str(GOLDEN))
    import verify_hand_typed
    rec = json.loads((GOLDEN / "hand_typed_verified.json").read_text())
    assert set(rec["tables"]) == set(verify_hand_typed.HAND_TYPED)
    assert set(rec["checks"]) == {fn.__name__ for fn in verify_hand_typed.CHECKS}
