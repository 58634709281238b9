"""The literal oracle of the toleration dry run with NRT's Filter in the refit (tests/ptol_nrt_oracle.py), CPU only: its Filter against the
reference's TestFilter_PreemptionFlow, the whole walk against ptol_oracle where no node has an NRT, and what the seeded generator's
largest GPU shape holds."""
import copy

import pytest

import ptol_cases as TC
import ptol_nrt_cases as NC
import ptol_nrt_oracle as NO
import ptol_oracle as TO
from golden import nrt_preemption_flow as GF
from scheduler_plugins_amd import objects as O


def canonical(rl):
    return {k: O.Resources().canonical(k, v) for k, v in rl.items()}


def flow_pod(p):
    return {"key": f"{p['ns']}/{p['name']}", "init_containers": [],
            "containers": [{"name": c["name"], "requests": canonical(c["requests"]), "limits": canonical(c["limits"])} for c in p["containers"]]}


def flow_node(placement):
    policy, scope = {"SingleNUMANodeContainerLevel": ("single-numa-node", "container")}[GF.NRT["policies"][0]]
    zones = [{"name": z["name"], "resources": [(name, O.Resources().canonical(name, alloc), O.Resources().canonical(name, avail)) for name, _, alloc, avail in z["resources"]]}
             for z in GF.NRT["zones"]]
    return {"nrt": {"zones": zones, "policy": policy, "scope": scope}, "nrt_fresh": True, "alloc_names": set(GF.NODE) | {"pods"},
            "placement": None if placement is None else {(f"{ns}/{name}", ctr): numa for (ns, name, ctr), numa in placement.items()}}


@pytest.mark.parametrize("case", GF.CASES, ids=lambda c: f"L{c['line']}")
def test_filter_reproduces_the_references_preemption_flow(case):
    got = NO.nrt_filter(flow_node(case["placement"]), flow_pod(case["preemptor"]), [flow_pod(v) for v in case["victims"]], case["enabled"])
    assert got == case["want"]


def without_nrt(m):
    m = copy.deepcopy(m)
    for node in m["nodes"]:
        node.update(nrt=None, nrt_fresh=True, placement=None, alloc_names={"cpu", "memory", "ephemeral-storage", "pods"})
    for p in [p for n in m["nodes"] for p in n["pods"]] + m["pending"]:
        p.setdefault("containers", [{"name": "c0", "requests": NC.request_dict(p["req"]), "limits": {}}])
        p.setdefault("init_containers", [])
    return m


def test_without_any_nrt_the_oracle_is_ptol_oracles():
    """on the reference's scenarios (tests/golden/preemption_toleration.json) and on a seeded snapshot, in both modes"""
    models = [TC.golden_integration_model(case) for case in TC.golden()["integration"]] + [NC.model(**NC.SHAPES["65x63"])]
    for m in models:
        bare = without_nrt(m)
        want = TO.dry_run(m, m["pending"])
        assert NO.dry_run(bare, bare["pending"], mode=True) == want
        assert NO.dry_run(bare, bare["pending"], mode=False) == want
    assert any(c["status"] == TO.ST["CANDIDATE"] for r in want for c in r["cells"])


def test_the_largest_gpu_shape_holds_every_way_the_filter_can_go():
    """the condition on the generator: with preemption mode on, the oracle's walk over the largest shape the GPU tests run takes each of
    these at least once"""
    m = NC.model(**NC.LARGEST)
    trace, by_f = set(), []
    want = NO.dry_run(m, m["pending"], None, True, trace, by_f)
    assert want == NC.expected(**NC.LARGEST)
    assert ("not-fit-by-F",) in by_f  # a cell NOT_FIT by F only
    assert any(w[0] == "kept-by-F" for w in by_f)  # a victim NodeResourcesFit alone would reprieve
    assert trace >= {"nothing-to-add", "exceeds", "stale", "no-nrt", "exempt", "not-single", "not-single/simulated", "empty-stack", "scope-pod", "scope-container",
                     "init-container-fails"}
    assert trace & {"nothing-to-add/not-single", "exceeds/not-single"}  # a failed simulation on a node whose policy would not filter
    assert {len(p["containers"]) + len(p["init_containers"]) for p in m["pending"]} >= {1, 8}
    assert {len(n["nrt"]["zones"]) for n in m["nodes"] if n["nrt"]} == {1, 2, 8}
    status = {c["status"] for r in want for c in r["cells"]}
    assert status >= {TO.ST[k] for k in ("CANDIDATE", "NO_VICTIMS", "NOT_FIT", "ALL_REPRIEVED", "SKIPPED")}
    # and the two dry runs differ in both directions: cells only this one refuses, victims only this one keeps
    plain = TO.dry_run(m, m["pending"])
    pairs = [(a, b) for r, q in zip(want, plain) for a, b in zip(r["cells"], q["cells"])]
    assert any(a["status"] == TO.ST["NOT_FIT"] and b["status"] == TO.ST["CANDIDATE"] for a, b in pairs)
    assert any(a["status"] == TO.ST["CANDIDATE"] and a["n_victims"] > b["n_victims"] for a, b in pairs)
    assert any(r["pick"][:3] != q["pick"][:3] for r, q in zip(want, plain))


def test_mode_disabled_is_the_ordinary_filter_and_differs():
    m = NC.model(**NC.LARGEST)
    on, off = NC.expected(**NC.LARGEST), NC.expected(mode=False, **NC.LARGEST)
    assert on != off
    trace = set()
    NO.dry_run(m, m["pending"][:8], None, False, trace)
    assert not trace & {"nothing-to-add", "exceeds", "not-single/simulated"}  # no simulation ever runs
