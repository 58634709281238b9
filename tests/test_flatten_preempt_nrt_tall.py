"""spx_flatten_preempt_nrt keeps its 8 zones per node: a node that lists 9 to 64 zones — which the dense NRT flattener now writes as
a placeholder row instead of failing — is refused by name before any walk over its zones.  Host side, no GPU."""
import copy

import pytest

import ptol_nrt_cases as NC
from test_flatten_preempt_nrt import KW, node_with, raises_arg, tampered


def _make_tall(m, n, zones, donor):
    node = m["nodes"][n]
    if node["nrt"] is None:
        node["nrt"] = copy.deepcopy(m["nodes"][donor]["nrt"])
    z = node["nrt"]["zones"]
    node["nrt"]["zones"] = [dict(z[0], name=f"node-{k}") for k in range(zones)]


@pytest.mark.parametrize("zones", [9, 16, 64])
def test_tall_nodes_are_refused_by_name(zones):
    m0 = NC.model(**KW)
    last = len(m0["nodes"]) - 1
    with_pods = node_with(m0, lambda node: len(node["pods"]) >= 2 and node["placement"])
    without = node_with(m0, lambda node: not node["placement"])
    bare = next((n for n, node in enumerate(m0["nodes"]) if node["nrt"] is not None and not node["pods"]), None)
    targets = {with_pods, without, last, 0} | ({bare} if bare is not None else set())
    assert len(targets) >= 3
    for n in sorted(targets):
        raises_arg(tampered(lambda m, n=n: _make_tall(m, n, zones, with_pods)), f"node {n}")


def test_two_tall_nodes_name_the_first():
    m0 = NC.model(**KW)
    a = node_with(m0, lambda node: len(node["pods"]) >= 2 and node["placement"])
    last = len(m0["nodes"]) - 1
    assert a < last

    def both(m):
        _make_tall(m, last, 16, a)
        _make_tall(m, a, 9, a)
    raises_arg(tampered(both), f"node {a}")


def test_eight_zones_still_pass():
    m0 = NC.model(**KW)
    n = node_with(m0, lambda node: len(node["pods"]) >= 2 and node["placement"])
    tampered(lambda m: _make_tall(m, n, 8, n))()
