"""PreemptionToleration's host side (no GPU): spx_flatten_preempt_toleration's three columns against the literal oracle's verdict for
every (preemptor priority, PreemptNever, pod) pair, its restatement of strconv.ParseInt, the two integer wraps and the clamp, the
strict comparison at until == now, the refusals, and spx_preempt_toleration_eligible against a literal loop."""
import ctypes as C

import numpy as np
import pytest

import ptol_cases as TC
import ptol_oracle as TO
import scheduler_plugins_amd as spx
from scheduler_plugins_amd import SpxError, objects
from scheduler_plugins_amd.engine import Engine

HDR = spx.header()
K = HDR.consts
INT32_MIN, INT32_MAX, INT64_MIN, INT64_MAX = -(1 << 31), (1 << 31) - 1, -(1 << 63), (1 << 63) - 1
HAS, MISSING = K["SPX_PTOL_POD_HAS_CLASS"], K["SPX_PTOL_POD_CLASS_MISSING"]
NOW, SEC = TC.GOLDEN_NOW, TC.SEC


class _Host:
    """the flatteners are host code and need no engine (no GPU here)"""
    _lib = spx.lib()
    _hdr = HDR
    _err = SpxError
    _ck_static = staticmethod(Engine._ck_static)
    _PREEMPT_NODE_COLS = Engine._PREEMPT_NODE_COLS
    flatten_quota = Engine.flatten_quota
    flatten_preempt_nodes = Engine.flatten_preempt_nodes
    preempt_nodes_table = Engine.preempt_nodes_table
    flatten_preempt_toleration = Engine.flatten_preempt_toleration
    preempt_toleration_eligible = Engine.preempt_toleration_eligible


def flatten(kw):
    t = TC.tables(**kw)
    h = _Host()
    f = h.flatten_preempt_nodes(t["nodes"], t["rc"], t["quota"], t["preempt"])
    return t, f, h.flatten_preempt_toleration(t["classes"], t["pod_class"], t["pod_scheduled"], t["pod_scheduled_at_ns"], f["pod_src"])


def verdict(cols, j, prio, never, now):
    """what the device concludes from the columns for the pod at table position j: "error", or exempted"""
    flags, mn, until = int(cols["flags"][j]), int(cols["min_preemptable"][j]), int(cols["exempt_until_ns"][j])
    if flags & MISSING:
        return "error"
    return bool(flags & HAS) and (never or (prio < mn and until > now))


def oracle_verdict(m, pod, prio, never, now):
    try:
        return TO.exempted(m["classes"], pod, {"prio": prio, "never": never}, now)[0]
    except TO.ClassNotFound:
        return "error"


# ---------------------------------------------------------------------------------------------------------------- columns against the oracle
def test_columns_give_the_oracles_verdict_for_every_pair():
    kw = dict(n_nodes=70, n_pending=66, seed=4)
    m = TC.model(**kw)
    t, f, cols = flatten(kw)
    assert len(cols["flags"]) == f["pod_ptr"][-1] and not ((cols["flags"] & HAS) & ((cols["flags"] & MISSING) >> 1)).any()
    seen = set()
    for j, src in enumerate(f["pod_src"]):
        node, k = t["assigned_at"][int(src)]
        pod = m["nodes"][node]["pods"][k]
        for prio in (INT32_MIN, 5, 49, 50, 51, 500, 5000, 5001, INT32_MAX):
            for never in (False, True):
                for now in (m["now"] - 2 * SEC, m["now"] - SEC, m["now"] - 1, m["now"], m["now"] + 1, m["now"] + SEC, m["now"] + 31 * SEC):
                    want = oracle_verdict(m, pod, prio, never, now)
                    assert verdict(cols, j, prio, never, now) == want, (pod, prio, never, now)
                    seen.add(want)
    assert seen == {"error", True, False}


def one_pod(value=0, mn=None, tol=None, scheduled_at=NOW, present=True):
    """the columns of one pod whose class has the given value and annotation texts"""
    ann = {}
    if mn is not None:
        ann[objects.PTOL_ANNOTATION_MIN] = mn
    if tol is not None:
        ann[objects.PTOL_ANNOTATION_TOLERATION] = tol
    classes = objects.build_priority_classes(HDR, ["c"], {"c": {"value": value, "annotations": ann}} if present else {})
    cols = _Host().flatten_preempt_toleration(classes, [0], [scheduled_at is not None], [scheduled_at or 0], [0])
    return int(cols["flags"][0]), int(cols["min_preemptable"][0]), int(cols["exempt_until_ns"][0])


# ---------------------------------------------------------------------------------------------------------------- strconv.ParseInt
BAD_TEXTS = ["", " 5", "5 ", "1_0", "0x10", "a", "+", "-", "--5", "+-5", "5a", "1e3", "5.0", "５", "٥"]
GOOD_32 = {"0": 0, "-0": 0, "+5": 5, "-5": -5, "007": 7, "2147483647": INT32_MAX, "-2147483648": INT32_MIN, "+2147483647": INT32_MAX, "0000000000002147483647": INT32_MAX}
GOOD_64 = {"0": 0, "+30": 30, "-1": -1, "9223372036854775807": INT64_MAX, "-9223372036854775808": INT64_MIN, "9223372037": 9223372037}


@pytest.mark.parametrize("text", BAD_TEXTS + ["2147483648", "-2147483649", "99999999999999999999", "9223372036854775807"])
def test_minimum_preemptable_priority_that_does_not_parse(text):
    assert TO.parse_int(text, 32) is None
    assert one_pod(mn=text) == (HAS, INT32_MIN, 0)  # a policy error: never below the minimum, still exempt from PreemptNever


@pytest.mark.parametrize("text", BAD_TEXTS + ["9223372036854775808", "-9223372036854775809", "99999999999999999999"])
def test_toleration_seconds_that_do_not_parse(text):
    assert TO.parse_int(text, 64) is None
    assert one_pod(mn="50", tol=text) == (HAS, INT32_MIN, 0)


@pytest.mark.parametrize("text", list(GOOD_32))
def test_minimum_preemptable_priority_that_parses(text):
    assert TO.parse_int(text, 32) == GOOD_32[text]
    assert one_pod(mn=text)[:2] == (HAS, GOOD_32[text])


@pytest.mark.parametrize("text", list(GOOD_64))
def test_toleration_seconds_that_parse(text):
    tol = GOOD_64[text]
    assert TO.parse_int(text, 64) == tol
    flags, mn, until = one_pod(mn="50", tol=text, scheduled_at=0)
    want = INT64_MAX if tol < 0 else max(INT64_MIN, min(INT64_MAX, TO.wrap(tol * SEC, 64)))
    assert (flags, mn, until) == (HAS, 50, want)


# ---------------------------------------------------------------------------------------------------------------- wraps, clamp, strictness
def test_value_plus_one_wraps_in_int32():
    assert one_pod(value=INT32_MAX)[:2] == (HAS, INT32_MIN)
    assert one_pod(value=INT32_MIN)[:2] == (HAS, INT32_MIN + 1)
    assert one_pod(value=1000)[:2] == (HAS, 1001)
    assert TO.parse_policy({"value": INT32_MAX, "annotations": {}}) == (INT32_MIN, 0)


def test_the_duration_wraps_in_int64_and_the_sum_does_not():
    wrapped = TO.wrap(9223372037 * SEC, 64)
    assert wrapped == 9223372037 * SEC - (1 << 64) < 0 < 9223372036 * SEC < INT64_MAX
    assert one_pod(mn="50", tol="9223372037", scheduled_at=NOW)[2] == NOW + wrapped  # a toleration of 292 years that ended long ago
    assert one_pod(mn="50", tol="9223372036", scheduled_at=NOW)[2] == INT64_MAX     # the sum leaves int64 upwards: clamped
    assert one_pod(mn="50", tol="9223372037", scheduled_at=-NOW)[2] == INT64_MIN    # and downwards
    assert one_pod(mn="50", tol="9223372036", scheduled_at=INT64_MAX - 9223372036 * SEC)[2] == INT64_MAX  # the last sum that fits
    assert one_pod(mn="50", tol="9223372037", scheduled_at=INT64_MIN - wrapped)[2] == INT64_MIN
    for tol, at in (("9223372037", NOW), ("9223372036", NOW), ("9223372037", -NOW)):
        pod = {"pc": "c", "scheduled_at": at}
        classes = {"c": {"value": 0, "annotations": {objects.PTOL_ANNOTATION_MIN: "50", objects.PTOL_ANNOTATION_TOLERATION: tol}}}
        cols = {k: np.array([v]) for k, v in zip(("flags", "min_preemptable", "exempt_until_ns"), one_pod(mn="50", tol=tol, scheduled_at=at))}
        for now in (INT64_MIN, -NOW, 0, NOW, INT64_MAX - 1):
            assert verdict(cols, 0, 5, False, now) == TO.exempted(classes, pod, {"prio": 5, "never": False}, now)[0]


def test_until_equal_to_now_is_not_exempted():
    flags, mn, until = one_pod(mn="50", tol="30", scheduled_at=NOW - 30 * SEC)
    assert (flags, mn, until) == (HAS, 50, NOW)
    cols = {"flags": np.array([flags]), "min_preemptable": np.array([mn]), "exempt_until_ns": np.array([until])}
    assert [verdict(cols, 0, 49, False, now) for now in (NOW - 1, NOW, NOW + 1)] == [True, False, False]
    pod, classes = {"pc": "c", "scheduled_at": NOW - 30 * SEC}, {"c": {"value": 0, "annotations": {objects.PTOL_ANNOTATION_MIN: "50", objects.PTOL_ANNOTATION_TOLERATION: "30"}}}
    assert [TO.exempted(classes, pod, {"prio": 49, "never": False}, now)[0] for now in (NOW - 1, NOW, NOW + 1)] == [True, False, False]


def test_for_ever_and_the_flags():
    assert one_pod(mn="50", tol="-1") == (HAS, 50, INT64_MAX)
    assert one_pod(mn="50", tol="30", scheduled_at=None) == (HAS, 50, INT64_MAX)
    assert one_pod(mn="50") == (HAS, 50, NOW)  # no toleration-seconds: 0
    assert one_pod(present=False) == (MISSING, 0, 0)
    classes = objects.build_priority_classes(HDR, [], {})
    cols = _Host().flatten_preempt_toleration(classes, [-1], [1], [NOW], [0])
    assert (int(cols["flags"][0]), int(cols["min_preemptable"][0]), int(cols["exempt_until_ns"][0])) == (0, 0, 0)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    h = _Host()
    classes = objects.build_priority_classes(HDR, ["c"], {"c": {"value": 0, "annotations": {}}})
    ok = dict(pod_class=[0, -1], pod_scheduled=[1, 0], pod_scheduled_at_ns=[0, 0], pod_src=[1, 0])
    assert h.flatten_preempt_toleration(classes, **ok)["flags"].tolist() == [0, HAS]  # permuted into the table's order
    for bad in (dict(pod_class=[1, -1]), dict(pod_class=[0, -2]), dict(pod_src=[2, 0]), dict(pod_src=[-1, 0])):
        with pytest.raises(RuntimeError):
            h.flatten_preempt_toleration(classes, **dict(ok, **bad))
    # the engine's entry points without an engine
    lib = spx.lib()
    assert lib.spx_upload_preempt_toleration(None, None) == K["SPX_ERR_ARG"]
    assert lib.spx_preempt_toleration_dry_run(None, None, 0, None, None, 0, None) == K["SPX_ERR_ARG"]
    assert lib.spx_flatten_preempt_toleration(None, 0, None, None, None, 0, None, None, None, None) == K["SPX_ERR_ARG"]
    assert lib.spx_preempt_toleration_eligible(None, 0, None, None, None, None, None) == K["SPX_ERR_ARG"]


# ---------------------------------------------------------------------------------------------------------------- PodEligibleToPreemptOthers
def test_eligibility_follows_the_literal_loop():
    kw = dict(n_nodes=70, n_pending=66, seed=4)
    m = TC.model(**kw)
    _, f, _ = flatten(kw)
    rng = np.random.default_rng(5)
    cases = [(p, int(node), bool(unres)) for p in m["pending"] for node, unres in zip(rng.integers(-1, len(m["nodes"]), 12), rng.random(12) < 0.3)]
    cases += [(dict(p, never=True), 0, False) for p in m["pending"][:3]]
    want = [TO.pod_eligible_to_preempt_others(m, p, node, unres) for p, node, unres in cases]
    got = _Host().preempt_toleration_eligible(f, [p["prio"] for p, _, _ in cases], [p["never"] for p, _, _ in cases], [n for _, n, _ in cases], [u for _, _, u in cases])
    assert got.tolist() == want
    assert {(w, p["never"], u) for w, (p, n, u) in zip(want, cases)} >= {(False, True, False), (False, False, False), (True, False, True), (True, False, False)}
    absent = [n for n, node in enumerate(m["nodes"]) if not node["present"]]
    assert absent and _Host().preempt_toleration_eligible(f, [5000], [0], absent[:1], [0]).tolist() == [True]
    with pytest.raises(RuntimeError):
        _Host().preempt_toleration_eligible(f, [5], [0], [len(m["nodes"])], [0])
