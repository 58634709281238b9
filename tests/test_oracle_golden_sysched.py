"""The SySched oracle (tests/sysched_oracle.py) and the product's profile resolution (scheduler_plugins_amd/objects.py) reproduce the
values the reference pins in pkg/sysched/sysched_test.go (tests/golden/sysched.json holds its data)."""
import json
from pathlib import Path

import numpy as np

import sysched_oracle as SO
from scheduler_plugins_amd import objects as O

G = json.loads((Path(__file__).parent / "golden" / "sysched.json").read_text())


def profiles():
    crs = [O.seccomp_profile(p["name"], p["namespace"], [{"action": p["action"], "names": p["names"]}]) for p in G["profiles"]]
    return O.SeccompProfiles(crs, G["default_profile"]["name"], G["default_profile"]["namespace"])


def test_fixture_lists():
    z, x, full = (p["names"] for p in G["profiles"])
    assert (len(z), len(x), len(full)) == (91, 91, 101) and len(set(z)) == 91
    assert set(z) - set(x) == {"fchmod"} and set(x) - set(z) == {"dup3"} and set(x) < set(full)


def test_parse_name_ns():
    for c in G["parse_name_ns"]:
        assert O.parse_name_ns(c["path"]) == (c["namespace"], c["name"])
    assert O.parse_name_ns("") == ("", "") and O.parse_name_ns("x.json") == ("", "")
    assert O.parse_name_ns("operator/ns/a.b.json") == ("ns", "a.b") and O.parse_name_ns("ns/noext") == ("ns", "noext")


def test_read_profile_and_get_syscalls_counts():
    pr = profiles()
    for c in G["read_profile"]:
        got, found = pr.read(c["name"], c["namespace"])
        assert found and len(got) == c["count"]
    for c in G["get_syscalls"]:
        assert len(pr.get_syscalls(O.sysched_pod(**c["pod"]))) == c["count"], c["case"]


def test_get_syscalls_rules():
    crs = [O.seccomp_profile("a", "ns", [{"action": "SCMP_ACT_ALLOW", "names": ["read"]}, {"action": "SCMP_ACT_LOG", "names": ["write"]},
                                         {"action": "SCMP_ACT_ERRNO", "names": ["ptrace"]}, {"action": "SCMP_ACT_TRACE", "names": ["kill"]}]),
           O.seccomp_profile("b", "ns", [{"action": "SCMP_ACT_ALLOW", "names": ["open"]}]),
           O.seccomp_profile("all", "ns", [{"action": "SCMP_ACT_ALLOW", "names": ["read", "write", "open", "close"]}])]
    pr = O.SeccompProfiles(crs, "all", "ns")
    pa, pb = "operator/ns/a.json", "operator/ns/b.json"
    assert pr.get_syscalls(O.sysched_pod(security_context=pa)) == {"read", "write"}  # only ALLOW and LOG are read (:112)
    assert pr.get_syscalls(O.sysched_pod(security_context=pa, containers=[pb, None])) == {"read", "write", "open"}
    assert pr.get_syscalls(O.sysched_pod(init_containers=[pb])) == {"read", "write", "open", "close"}  # init containers are not read: default
    # several seccomp annotations: the smallest key wins (the reference iterates a Go map: unpinned there)
    k = O.SPO_ANNOTATION
    assert pr.get_syscalls(O.sysched_pod(annotations={k + "/z": pa, k + "/y": pb, "other": pa})) == {"open"}
    # a missing CR contributes nothing and the loop moves on (:183-186); a missing CR everywhere falls back to the default
    assert pr.get_syscalls(O.sysched_pod(annotations={k + "/a": "operator/ns/missing.json", k + "/b": pb})) == {"open"}
    assert pr.get_syscalls(O.sysched_pod(security_context="operator/ns/missing.json")) == {"read", "write", "open", "close"}
    # no default profile either: the empty set, which Score answers with math.MaxInt64
    none = O.SeccompProfiles(crs)
    assert none.get_syscalls(O.sysched_pod()) == frozenset()
    assert SO.score(frozenset(), frozenset({"read"}), []) == SO.MAX_INT64


def test_score_golden():
    pr = O.SeccompProfiles([O.seccomp_profile(p["name"], p["namespace"], [{"action": p["action"], "names": p["names"]}]) for p in G["profiles"]])
    k = O.SPO_ANNOTATION
    existing = pr.get_syscalls(O.sysched_pod(annotations={k: G["score"]["existing_pod_annotation"]}))
    H = existing  # addPod: the host set is the union of the residents' sets (sysched.go:310-333)
    for c in G["score"]["cases"]:
        P = pr.get_syscalls(O.sysched_pod(annotations={k: c["annotation"]}))
        assert SO.score(P, H, [existing]) == c["expected"], c["case"]
    assert SO.score(existing, None, []) == 0  # no HostSyscalls entry (:253-259)


def test_normalize_golden():
    for c in G["normalize"]["cases"]:
        assert SO.normalize(c["scores"]) == c["expected"]
    assert SO.normalize([0, 0, 0]) == [100, 100, 100]
    assert SO.normalize([7, 3, 0]) == [0, 100 - 300 // 7, 100]


def test_maxint64_row_normalises_to_100_by_the_wrap():
    # the expectation from int64 wraparound alone: 100 * (2^63 - 1) = 100 * 2^63 - 100 = -100 (mod 2^64), since 100 * 2^63 = 50 * 2^64;
    # -100 / (2^63 - 1) truncates to 0; 100 - 0 = 100
    m = (1 << 63) - 1
    prod = (100 * m) % (1 << 64)
    prod = prod - (1 << 64) if prod >= (1 << 63) else prod
    assert prod == -100
    q = -(100 // m)  # truncation toward zero of -100 / m
    assert q == 0
    expected = 100 - q
    assert SO.normalize([m, m, m]) == [expected] * 3 == [100, 100, 100]
    assert SO.normalize_row(np.array([m, m], np.int64)).tolist() == [100, 100]
