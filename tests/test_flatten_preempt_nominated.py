"""spx_flatten_preempt_nominated_quota (host only): the side table of CapacityScheduling's sequential loop against the model — the
records in the order of spx_flatten_preempt_nodes' nominated CSR, each with its namespace (quota or not) and its
computePodResourceRequest; records on absent nodes left out; a wrong count refused."""
import copy

import numpy as np
import pytest

import preempt_seq_cases as SC
import scheduler_plugins_amd as spx
from scheduler_plugins_amd import SpxError, objects
from scheduler_plugins_amd.engine import Engine

K = spx.header().consts


def model_with_an_absent_nominated_node():
    m = copy.deepcopy(SC.model("retuned", **SC.RETUNED["63x65"]))
    holders = [n for n, nd in enumerate(m["nodes"]) if nd["nominated"] and nd["present"]]
    assert len(holders) >= 3
    m["nodes"][holders[1]]["present"] = False
    return m, holders[1]


class _Host:
    """the flatteners are host code and need no engine (no GPU here)"""
    _lib = spx.lib()
    _hdr = spx.header()
    _err = SpxError
    _ck_static = staticmethod(Engine._ck_static)
    flatten_preempt_nodes = Engine.flatten_preempt_nodes
    flatten_preempt_nominated_quota = Engine.flatten_preempt_nominated_quota


def flatten(m):
    t = objects.build_preempt_tables(spx.header(), m)
    e = _Host()
    f = e.flatten_preempt_nodes(t["nodes"], t["rc"], t["quota"], t["preempt"])
    return e, t, f, e.flatten_preempt_nominated_quota(t["nodes"], t["rc"], t["quota"], t["preempt"], len(f["nom_priority"]))


def test_order_requests_and_namespaces():
    m, absent = model_with_an_absent_nominated_node()
    e, t, f, side = flatten(m)
    want = [(n, p) for n, nd in enumerate(m["nodes"]) if nd["present"] for p in nd["nominated"]]
    assert len(want) == len(side["ns"]) == f["nom_ptr"][-1] > 0
    assert all(n != absent for n, _ in want) and m["nodes"][absent]["nominated"]  # the records of the absent node are left out
    # the objects' order: build_preempt_tables lists the nominated pods node by node, absent nodes included
    objs = [(n, p) for n, nd in enumerate(m["nodes"]) for p in nd["nominated"]]
    assert [objs[i][1]["key"] for i in side["nom_src"]] == [p["key"] for _, p in want]
    for j, (n, p) in enumerate(want):
        assert f["nom_ptr"][n] <= j < f["nom_ptr"][n + 1]
        assert side["ns"][j] == p["ns"]
        assert side["quota_req"][j].tolist() == p["req"]["v"]
        assert side["quota_req_present"][j] == p["req"]["p"]
        assert (f["nom_priority"][j], f["nom_pending_row"][j]) == (p["prio"], p["row"])  # the same record of the node table
        assert f["nom_fit_req"][j].tolist() == p["fit"]
    assert {p["ns"] for _, p in want} - set(m["quotas"]), "no nominated pod of a namespace without quota"
    assert any(p["req"]["p"] for _, p in want), "no nominated pod with a scalar key"


def test_a_wrong_count_is_refused_and_an_empty_table_is_fine():
    m, _ = model_with_an_absent_nominated_node()
    e, t, f, side = flatten(m)
    with pytest.raises(SpxError) as err:
        e.flatten_preempt_nominated_quota(t["nodes"], t["rc"], t["quota"], t["preempt"], len(side["ns"]) + 1)
    assert err.value.code == K["SPX_ERR_ARG"]
    for nd in m["nodes"]:
        nd["nominated"] = []
    e, t, f, side = flatten(m)
    assert len(side["ns"]) == 0 and f["nom_ptr"][-1] == 0
