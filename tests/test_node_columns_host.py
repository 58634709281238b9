"""Host side of NodeMetadata, PodState and QOSSort: the flatteners (host/flatten_node_columns.cc) against the plain-Python reference
(tests/node_columns_ref.py) and the reference's own test tables (tests/golden/nodemetadata.json, podstate.json, qossort.json), and the
reference itself on the constructed columns of the GPU tests, each asserted to hold the edge it was built for.  No GPU."""
import json
from pathlib import Path

import numpy as np
import pytest

import node_columns_ref as R
from scheduler_plugins_amd import SpxError
from scheduler_plugins_amd import objects as O
from scheduler_plugins_amd.engine import INVALID_SCORE, Engine

GOLDEN = Path(__file__).resolve().parent / "golden"
NOW = 1_700_000_000_123_456_789  # an explicit "now" (ns) in place of time.Now()
INVALID = R.INVALID

# value -> float64 Go parses, or None for an error
PARSE_FLOAT = [("10", 10.0), ("-0", -0.0), ("1e3", 1000.0), ("1E-400", 0.0), ("1e400", None), ("0x1p4", 16.0), ("0x10", None), ("1_0", None),
               ("0x1_0p0", 16.0), (" 1", None), ("1 ", None), ("nan", "nan"), ("NaN", "nan"), ("nan(1)", None), ("+Inf", float("inf")),
               ("infinity", float("inf")), ("9223372036854775807", 2.0 ** 63), ("9223372036854775808", 2.0 ** 63),
               ("-9223372036854775808", -(2.0 ** 63)), ("9.3e18", 9.3e18), ("", None),
               # beyond the list: the grammar's other corners
               ("-Infinity", float("-inf")), ("+nan", None), ("infin", None), ("0x", None), ("0x.p1", None), ("0x1.8p1", 3.0), ("0X_1_2.3_4_5P+1_2", 74565.0),
               ("0x_1_2.3_4_5p+1_2", 74565.0), ("0x1__0p0", None), ("0x1_p0", None), ("0x1p_1", None), ("0x1p1_", None), ("1e", None), ("1e+", None),
               (".5", 0.5), ("5.", 5.0), (".", None), ("+", None), ("1.2.3", None), ("-5.9", -5.9), ("5.9", 5.9), ("1e2_0", None), ("0x1p1024", None),
               ("0x1p-1080", 0.0), ("1,5", None), ("12abc", None), ("١٢", None), ("4e18", 4e18), ("-9.3e18", -9.3e18), ("1e18", 1e18)]


def test_parse_float_grammar_of_the_reference_matches_the_list():
    for s, want in PARSE_FLOAT:
        got = R.parse_float(s)
        if want is None:
            assert got is None, s
        elif want == "nan":
            assert got is not None and np.isnan(got), s
        else:
            assert got == want and np.signbit(got) == np.signbit(want), (s, got)


@pytest.mark.parametrize("strategy", ["Highest", "Lowest"])
def test_number_flattener_against_the_reference(strategy):
    values = [s for s, _ in PARSE_FLOAT] + [None, "0", "-1", "100", "1e-5", "123456789.987"]
    got = Engine.flatten_nodemeta(values, "Number", strategy)
    want = [R.number_score(v, strategy) for v in values]
    assert [int(g) for g in got] == want, [(v, int(g), w) for v, g, w in zip(values, got, want) if int(g) != w]
    by = dict(zip(values, (int(g) for g in got)))
    # NaN, Inf and |v| >= 2^63 convert to MinInt64 and are invalid under either strategy; so is every error
    for s in ("nan", "NaN", "+Inf", "infinity", "-Infinity", "9223372036854775807", "9223372036854775808", "-9223372036854775808", "9.3e18", "-9.3e18",
              "1e400", "0x10", "1_0", " 1", "1 ", "nan(1)", "", None):
        assert by[s] == INVALID == INVALID_SCORE, s
    sign = -1 if strategy == "Lowest" else 1
    assert by["10"] == 10 * sign and by["1e3"] == 1000 * sign and by["0x1p4"] == 16 * sign and by["0x1_0p0"] == 16 * sign
    assert by["-0"] == 0 and by["1E-400"] == 0 and by["-5.9"] == -5 * sign and by["5.9"] == 5 * sign and by["4e18"] == 4 * 10 ** 18 * sign


def rfc3339(ns, offset_minutes=0, digits=0):
    import datetime
    sec, frac = divmod(ns, 10 ** 9)
    t = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=sec + offset_minutes * 60)
    s = t.strftime("%Y-%m-%dT%H:%M:%S")
    if digits:
        s += "." + f"{frac:09d}"[:digits]
    if offset_minutes == 0:
        return s + "Z"
    return s + ("+" if offset_minutes > 0 else "-") + f"{abs(offset_minutes) // 60:02d}:{abs(offset_minutes) % 60:02d}"


@pytest.mark.parametrize("strategy", ["Newest", "Oldest"])
def test_timestamp_flattener_against_the_reference(strategy):
    hour = 3600 * 10 ** 9
    stamps = [NOW - hour, NOW - 72 * hour, NOW - 1, NOW, NOW + 1_500_000_000, NOW + 999_999_999, NOW - 999_999_999, NOW - 86400 * 365 * 30 * 10 ** 9, 0, -1]
    values = []
    for t in stamps:
        for off in (0, 120, -330):
            for digits in (0, 3, 9):
                values.append(rfc3339(t, off, digits))
    values += ["2023-11-14", "2023-11-14T22:13:20", "2023-11-14 22:13:20Z", "2023-11-14t22:13:20Z", "2023-02-29T00:00:00Z", "2024-02-29T00:00:00Z",
               "2023-11-14T24:00:00Z", "2023-11-14T22:60:00Z", "2023-11-14T22:13:60Z", "2023-11-14T2:13:20Z", "2023-11-14T22:13:20.Z",
               "2023-11-14T22:13:20,25Z", "2023-11-14T22:13:20.1234567891234Z", "2023-11-14T22:13:20+0200", "2023-11-14T22:13:20+25:00",
               "2023-11-14T22:13:20+24:00", "2023-11-14T22:13:20Zjunk", " 2023-11-14T22:13:20Z", "not-a-timestamp", "", None, "0000-01-01T00:00:00Z",
               "9000-01-01T00:00:00Z", "1677-01-01T00:00:00Z"]
    got = Engine.flatten_nodemeta(values, "Timestamp", strategy, NOW)
    want = [R.timestamp_score(v, strategy, NOW) for v in values]
    assert [int(g) for g in got] == want, [(v, int(g), w) for v, g, w in zip(values, got, want) if int(g) != w]
    by = dict(zip(values, (int(g) for g in got)))
    sign = -1 if strategy == "Newest" else 1
    assert by["2023-11-14"] == INVALID and by["2023-02-29T00:00:00Z"] == INVALID and by["2024-02-29T00:00:00Z"] != INVALID
    assert by[rfc3339(NOW - hour, 0, 9)] == 3600 * sign and by[rfc3339(NOW - hour, 120, 9)] == 3600 * sign and by[rfc3339(NOW - hour, -330, 9)] == 3600 * sign
    # a timestamp in the future: a negative age, truncated toward zero
    assert by[rfc3339(NOW + 1_500_000_000, 0, 9)] == -1 * sign and by[rfc3339(NOW + 999_999_999, 0, 9)] == 0
    # three digits cut the fraction: .123 against now's .123456789 leaves 0.000456789 s more
    assert by[rfc3339(NOW - hour, 0, 3)] == 3600 * sign and by[rfc3339(NOW - hour, 0, 0)] == 3600 * sign
    # the caller-parsed variant gives the same scores
    ok = [v for v in values if v is not None and R.parse_rfc3339(v) is not None]
    unix = [R.parse_rfc3339(v) for v in ok]
    inside = [i for i, t in enumerate(unix) if R.INT64_MIN <= t <= R.INT64_MAX]
    got_unix = Engine.flatten_nodemeta_unix([unix[i] for i in inside] + [0], [1] * len(inside) + [0], strategy, NOW)
    assert [int(g) for g in got_unix] == [by[ok[i]] for i in inside] + [INVALID]


def test_flattener_refuses_what_the_header_says():
    with pytest.raises(SpxError):
        Engine.flatten_nodemeta(["1"], "Number", "Newest")
    with pytest.raises(SpxError):
        Engine.flatten_nodemeta(["2023-11-14T22:13:20Z"], "Timestamp", "Highest", NOW)
    with pytest.raises(SpxError):
        Engine.flatten_nodemeta_unix([0], [1], "Lowest", NOW)


def test_golden_calculate_score_and_normalize_score():
    g = json.loads((GOLDEN / "nodemetadata.json").read_text())
    assert len(g["calculate_score"]) == 6 and len(g["normalize_score"]) == 8

    def value(node):
        return rfc3339(NOW + node["offset_seconds"] * 10 ** 9) if "offset_seconds" in node else node["value"]

    def raw_of(case, nodes):
        vals = [value(n) for n in nodes]
        got = Engine.flatten_nodemeta(vals, case["type"], case["strategy"], NOW)
        ref = [R.number_score(v, case["strategy"]) if case["type"] == "Number" else R.timestamp_score(v, case["strategy"], NOW) for v in vals]
        assert [int(x) for x in got] == ref, case["name"]
        return ref

    for c in g["calculate_score"]:
        (score,) = raw_of(c, [c])
        assert (score == INVALID) == c["expect_error"], c["name"]
        if "check" in c:
            assert score == c["check"]["eq"] if "eq" in c["check"] else score < c["check"]["lt"], c["name"]
    for c in g["normalize_score"]:
        raw = raw_of(c, c["nodes"])
        norm = R.normalize_nodemeta(raw)
        if "expected_score" in c:
            assert norm == [c["expected_score"]] * len(raw), c["name"]
        else:  # sort.Slice by score descending; the test's expectations never depend on the order of equal scores' names beyond what it lists
            names = [n["name"] for n in c["nodes"]]
            order = sorted(range(len(raw)), key=lambda i: -norm[i])
            assert sorted(norm, reverse=True) == [norm[names.index(n)] for n in c["expected_order"]], c["name"]
            assert [names[i] for i in order if raw[i] != INVALID] == [n for n in c["expected_order"] if raw[names.index(n)] != INVALID], c["name"]
            assert all(norm[i] == 0 for i in range(len(raw)) if raw[i] == INVALID) and all(1 <= norm[i] <= 100 for i in range(len(raw)) if raw[i] != INVALID)


def test_golden_podstate_and_counts():
    g = json.loads((GOLDEN / "podstate.json").read_text())
    assert len(g["cases"]) == 5
    for c in g["cases"]:
        assigned_node, terminating, nominated = [], [], []
        for n, (term, nom, regular) in enumerate(c["nodes"]):  # makeNodeInfo: terminating, nominated and regular pods all sit on the node
            assigned_node += [n] * (term + nom + regular)
            terminating += [1] * term + [0] * (nom + regular)
            nominated += [n] * nom
        raw = Engine.flatten_podstate(len(c["nodes"]), assigned_node, terminating, nominated)
        assert [int(v) for v in raw] == R.podstate_counts(len(c["nodes"]), assigned_node, terminating, nominated) == [t - m for t, m, _ in c["nodes"]]
        assert R.normalize_podstate([int(v) for v in raw]) == c["expected"], c["line"]
    # a node with neither kind of pod, and one with both
    raw = Engine.flatten_podstate(4, [0, 0, 3, 3, 3], [1, 0, 1, 1, 0], [3, 1, 1])
    assert [int(v) for v in raw] == [1, -2, 0, 1]
    assert [int(v) for v in Engine.flatten_podstate(2, [], [], [])] == [0, 0]
    for bad in (dict(assigned_node=[2], assigned_terminating=[1], nominated_node=[]), dict(assigned_node=[-1], assigned_terminating=[0], nominated_node=[]),
                dict(assigned_node=[], assigned_terminating=[], nominated_node=[2]), dict(assigned_node=[], assigned_terminating=[], nominated_node=[-1])):
        with pytest.raises(SpxError):
            Engine.flatten_podstate(2, **bad)


def test_qos_less_on_the_golden_table_and_every_class_pair(hdr):
    g = json.loads((GOLDEN / "qossort.json").read_text())
    assert len(g["cases"]) == 9
    res = O.Resources()
    pods, want_class = [], []
    for c in g["cases"]:
        for p in (c["p1"], c["p2"]):
            pods.append(O.pod([O.container(p["requests"], p["limits"])]))
            want_class.append(1 if p["requests"] is None else 3 if p["requests"] == p["limits"] else 2)
    qos = Engine.flatten_pod_qos(O.build_pod_objects(hdr, res, pods))
    assert [int(q) for q in qos] == want_class
    for k, c in enumerate(g["cases"]):
        t1, t2 = ((p["ts_offset_seconds"] or 0) * 10 ** 9 for p in (c["p1"], c["p2"]))
        a, b = (c["p1"]["priority"], int(qos[2 * k]), t1), (c["p2"]["priority"], int(qos[2 * k + 1]), t2)
        assert Engine.qos_less(*a, *b) == R.qos_less(a, b) == c["want"], c["name"]
    for q1 in (1, 2, 3):
        for q2 in (1, 2, 3):
            for t1, t2 in ((0, 0), (0, 1), (1, 0), (-5, R.INT64_MAX)):
                a, b = (7, q1, t1), (7, q2, t2)
                assert Engine.qos_less(*a, *b) == R.qos_less(a, b) == (q1 > q2 or (q1 == q2 and t1 < t2))
    assert Engine.qos_less(-(1 << 31), 3, 0, (1 << 31) - 1, 1, 9) is False and Engine.qos_less((1 << 31) - 1, 1, 9, -(1 << 31), 3, 0) is True


# ------------------------------------------------------------------ the reference on the constructed GPU cases: each holds its edge
@pytest.mark.parametrize("span", R.RANGES)
def test_constructed_nodemetadata_columns_hold_their_edges(span):
    for place in R.placements(257):
        t = R.table(R.META, 257, 65, span, place)
        lo, hi = t.raw[place[0]], t.raw[place[1]]
        valid = [v for v in t.raw if v != INVALID]
        assert min(valid) == lo and max(valid) == hi and hi - lo == span and INVALID in t.raw
        whole = t.values[t.row("all nodes feasible")]
        assert whole[place[1]] == (100 if span <= R.INT64_MAX // 99 else whole[place[1]]) and whole[place[0]] == 1
        assert all(v == 0 for v, s in zip(whole, t.raw) if s == INVALID)
        unwrapped = [(s - lo) * 99 // span + 1 for s in t.raw if s != INVALID]
        if span > R.INT64_MAX // 99:  # the product wraps for the larger differences: the unwrapped value differs somewhere
            assert [v for v, s in zip(whole, t.raw) if s != INVALID] != unwrapped
        else:
            assert [v for v, s in zip(whole, t.raw) if s != INVALID] == unwrapped
        if span > R.INT64_MAX:
            assert R.wrap64(hi - lo) < 0  # max - min itself wraps to a negative range
        assert (t.want[t.row("no feasible node")] == 0).all()
        one = t.row("one feasible node, valid")
        assert t.values[one][int(np.flatnonzero(t.masks[one])[0])] == 1
        assert (t.want[t.row("one feasible node, invalid")] == 0).all() and (t.want[t.row("feasible nodes all invalid")] == 0).all()
        inner = t.row("global minimum and maximum infeasible")
        feas = [t.raw[n] for n in np.flatnonzero(t.masks[inner]) if t.raw[n] != INVALID]
        assert lo not in feas and hi not in feas  # the range comes from interior nodes (none is left when the span is 1)
        if len(set(feas)) > 1 and max(feas) - min(feas) <= R.INT64_MAX // 99:
            assert t.values[inner][t.raw.index(max(feas))] == 100 and t.values[inner][t.raw.index(min(feas))] == 1
        eq = t.row("all valid feasible nodes equal, invalid ones mixed in")
        assert sorted({t.values[eq][n] for n in np.flatnonzero(t.masks[eq])}) == [0, 1]
        assert (t.want[t.row("all nodes feasible")] == t.unmasked).all()


def test_constructed_podstate_columns_hold_their_edges():
    span = R.podstate_span(257)
    for place in R.placements(257):
        t = R.table(R.PODSTATE, 257, 65, span, place)
        assert t.raw[place[0]] == -((1 << 31) - 1) and t.raw[place[1]] == (1 << 31) - 1 and min(t.raw) == t.raw[place[0]] and max(t.raw) == t.raw[place[1]]
        whole = t.values[t.row("all nodes feasible")]
        assert whole[place[1]] == 100 and whole[place[0]] == 0 and whole == [(s - t.raw[place[0]]) * 100 // span for s in t.raw]
        one = t.row("one feasible node, valid")
        assert (t.want[one] == 0).all() and (t.want[t.row("no feasible node")] == 0).all()
    for span in (1, 99, 100):
        t = R.table(R.PODSTATE, 65, 65, span, (0, 64))
        assert max(t.raw) - min(t.raw) == span and t.values[0][64] == 100 and t.values[0][0] == 0
