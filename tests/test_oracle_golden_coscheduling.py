"""The Coscheduling oracle (tests/cosched_oracle.py) and the product's Less (spx_cosched_less) reproduce what the reference pins in
pkg/coscheduling/core/core_test.go and coscheduling_test.go (tests/golden/coscheduling.json holds their tables as data).  CPU only."""
import json
from pathlib import Path

import pytest

import cosched_cases as CC
import cosched_oracle as CO
import scheduler_plugins_amd as spx
from scheduler_plugins_amd import objects as O
from scheduler_plugins_amd.engine import Engine

G = json.loads((Path(__file__).parent / "golden" / "coscheduling.json").read_text())
ZERO_TIME = -(1 << 62)  # a PodGroup built without .Time(): Go's zero time, before everything else


class _Host:
    """Engine.cosched_less reads only the library handle: Less is host code and needs no engine (no GPU here)"""
    _lib = spx.lib()
    _ck_static = staticmethod(Engine._ck_static)


def ns_of(seconds):
    return ZERO_TIME if seconds is None else int(round(seconds * 1e9))


def pod_of(d):
    return {"namespace": d["namespace"], "name": d["name"], "labels": d.get("labels", {}), "gated": d.get("gated", False), "requests": d.get("requests", {}),
            "priority": d.get("priority", 0)}


def groups_of(pgs):
    return {f"{g['namespace']}/{g['name']}": {"min_member": g.get("min_member", 0), "min_resources": g.get("min_resources"), "created_ns": ns_of(g.get("created_s"))}
            for g in pgs}


def test_fixture_shape():
    assert G["label"] == O.POD_GROUP_LABEL
    assert (len(G["prefilter"]["cases"]), len(G["check_cluster_resource"]["cases"]), len(G["less"]["cases"])) == (10, 3, 14)
    assert len(G["less_after_schedule_failure"]["steps"]) == 3


@pytest.mark.parametrize("case", G["prefilter"]["cases"], ids=lambda c: c["name"])
def test_prefilter(case):
    pod, pending = pod_of(case["pod"]), [pod_of(p) for p in case["pending_pods"]]
    # the pending pods have no NodeName: the fake lister files them under a NodeInfo without a Node
    nodes = [{"present": False, "allocatable": {}, "pods": pending}] + [{"present": True, "allocatable": n["allocatable"], "pods": []} for n in G["prefilter"]["nodes"]]
    status = CO.prefilter(pod, groups_of(case["pgs"]), pending + [pod], nodes)
    assert (status == CO.SUCCESS) == case["expected_success"], status


@pytest.mark.parametrize("case", G["check_cluster_resource"]["cases"], ids=lambda c: c["name"])
def test_check_cluster_resource(case):
    nodes = [{"present": True, "allocatable": n["allocatable"], "pods": [pod_of(p) for p in case["existing_pods"] if p["node"] == n["name"]]}
             for n in G["check_cluster_resource"]["nodes"]]
    req = {k: CO.canonical_exact(k, v) for k, v in case["min_resources"].items()}  # the test calls CheckClusterResource directly: no pods entry
    ok, _ = CO.check_cluster_resource(nodes, req, case["pg_name"])
    assert ok == case["want"]


def product_less(p1, p2, pgs, last_failed_s):
    """Less(p1, p2) through spx_cosched_less: the two pods as a pending batch, the PodGroups (and failure times) as the group table"""
    hdr = spx.header()
    groups = [O.pod_group(g["namespace"], g["name"], g.get("min_member", 0), None, created_ns=ns_of(g.get("created_s")),
                          last_failed_ns=(ns_of(last_failed_s[f"{g['namespace']}/{g['name']}"]) if f"{g['namespace']}/{g['name']}" in last_failed_s else None)) for g in pgs]
    for full, t in last_failed_s.items():  # a failure recorded for a name without a PodGroup object
        if full not in {f"{g['namespace']}/{g['name']}" for g in pgs}:
            groups.append(O.pod_group(*full.split("/", 1), exists=False, last_failed_ns=ns_of(t)))
    pods = [O.cosched_pod(p["namespace"], p["name"], p.get("labels", {})) for p in (p1, p2)]
    objects = O.build_cosched_objects(hdr, O.Resources(), groups, pods, [], [])
    ts = [ns_of(p.get("initial_attempt_s", 0)) for p in (p1, p2)]
    keys = [O.pod_key(p["namespace"], p["name"]) for p in (p1, p2)]
    return bool(Engine.cosched_less(_Host(), objects, [p["priority"] for p in (p1, p2)], ts, keys, [0], [1])[0])


def oracle_less(p1, p2, pgs, last_failed_s):
    lf = {k: ns_of(v) for k, v in last_failed_s.items()}
    return CO.less(pod_of(p1), ns_of(p1.get("initial_attempt_s", 0)), pod_of(p2), ns_of(p2.get("initial_attempt_s", 0)), groups_of(pgs), lf)


@pytest.mark.parametrize("case", G["less"]["cases"], ids=lambda c: c["name"])
def test_less(case):
    assert oracle_less(case["p1"], case["p2"], case["pgs"], {}) == case["want"]
    assert product_less(case["p1"], case["p2"], case["pgs"], {}) == case["want"]


def test_less_after_schedule_failure():
    c = G["less_after_schedule_failure"]
    for step in c["steps"]:
        for less in (oracle_less, product_less):
            assert less(c["p1"], c["p2"], c["pgs"], step["last_failed_s"]) == step["less_p1_p2"], step["what"]
            if "less_p2_p1" in step:
                assert less(c["p2"], c["p1"], c["pgs"], step["last_failed_s"]) == step["less_p2_p1"], step["what"]


def test_less_ties_fall_to_the_pod_key_and_failure_time_needs_no_object():
    """beyond the reference's table: equal priority and time compare "namespace/name" bytewise (a prefix sorts first), and
    lastFailedSchedulePG is looked up by full name before the PodGroup object is (core.go:376-383)"""
    a = {"namespace": "ns", "name": "p", "priority": 1, "labels": {}, "initial_attempt_s": 5}
    b = {"namespace": "ns", "name": "p1", "priority": 1, "labels": {}, "initial_attempt_s": 5}
    for less in (oracle_less, product_less):
        assert less(a, b, [], {}) and not less(b, a, [], {}) and not less(a, a, [], {})
    c = dict(a, labels={O.POD_GROUP_LABEL: "ghost"}, initial_attempt_s=1)
    d = dict(b, initial_attempt_s=2)
    for less in (oracle_less, product_less):
        assert less(c, d, [], {}) and not less(c, d, [], {"ns/ghost": 3})
