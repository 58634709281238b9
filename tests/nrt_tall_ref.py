"""LeastNUMANodes' subset search in plain Python, written from pkg/noderesourcetopology/least_numa.go (numaNodesRequired :156-174,
findSuitableCombination :176-208, minAvgDistanceInCombinations :102-114, nodesAvgDistance :116-138, combineResources :140-154,
checkResourcesFit :210-222, isValidCombineResources :224-233, normalizeScore :91-100, leastNUMAPodScopeScore :73-89) and
pluginhelpers.go:163-173 (onlyNonNUMAResources) — a second anchor for the oracle's walk over more than 8 zones, which the reference's
own test tables (8 zones at most) do not reach.

Every subset of every size is enumerated with itertools.combinations, in its order (gonum's combin.Combinations is lexicographic as
well), and tested: there is no short cut of any kind.  Quantities are Python integers, distances numpy.float32 as the reference's
float32.  The distances of a node's subsets do not depend on the request, so they are kept per (node, size) — that is a cache of what
the Go code recomputes, not a change of what it computes.

A node is a list of zones in NRT list order: {"id": NUMA id, "resources": {name: int}, "costs": {NUMA id: int}}; a request is
{name: int}.  Guaranteed QoS throughout (any other class scores 100 before the search, score.go:71-75)."""
import itertools

import numpy as np

MAX_DISTANCE = 255   # maxDistanceValue
MAX_NODE_SCORE, MIN_NODE_SCORE = 100, 0


def nodes_avg_distance(zones, combo):
    if len(combo) == 0:
        return np.float32(MAX_DISTANCE)
    accu = 0
    for a in combo:
        for b in combo:
            accu += zones[a]["costs"].get(zones[b]["id"], MAX_DISTANCE)
    return np.float32(accu) / np.float32(len(combo) * len(combo))


class Node:
    """a zone list with the distances of its subsets, by size, computed when first asked for"""

    def __init__(self, zones):
        self.zones = zones
        self._by_size = {}

    def subsets(self, k):
        """[(combination, average distance)] for every combination of size k, and the smallest distance among them (from 255)"""
        if k not in self._by_size:
            combos = [(c, nodes_avg_distance(self.zones, c)) for c in itertools.combinations(range(len(self.zones)), k)]
            min_avg = np.float32(MAX_DISTANCE)
            for _, d in combos:
                if d < min_avg:
                    min_avg = d
            self._by_size[k] = (combos, min_avg)
        return self._by_size[k]


def find_suitable_combination(node, request, k):
    combos, min_avg = node.subsets(k)
    zones = node.zones
    # per zone, once per call instead of once per combination: does it report every requested name (isValidCombineResources), and
    # what it holds of each name that is asked for with a non-zero quantity (combineResources + checkResourcesFit)
    reports_all = [all(name in z["resources"] for name in request) for z in zones]
    asked = [(quantity, [z["resources"].get(name, 0) for z in zones]) for name, quantity in request.items() if quantity != 0]
    best, min_distance = None, np.float32(256)
    for combo, distance in combos:
        if not all(reports_all[z] for z in combo):
            continue
        if any(sum(held[z] for z in combo) < quantity for quantity, held in asked):   # isResourceSetSuitable, Guaranteed
            continue
        if distance == min_avg:
            return combo, True
        if distance < min_distance:
            min_distance, best = distance, combo
    return best, False


def numa_nodes_required(node, request):
    """(the chosen list positions, the set of their NUMA ids, is-minimal-distance), or (None, None, False)"""
    for k in range(1, len(node.zones) + 1):
        combo, is_min = find_suitable_combination(node, request, k)
        if combo is not None:
            return combo, {node.zones[z]["id"] for z in combo}, is_min
    return None, None, False


def normalize_score(count, is_min, max_numa):
    per = MAX_NODE_SCORE // max_numa
    score = MAX_NODE_SCORE - count * per
    return score + per // 2 if is_min else score


def only_non_numa(node, request):
    return not any(name in z["resources"] for name in request for z in node.zones)


def pod_scope_score(node, request, max_numa=8):
    if only_non_numa(node, request):
        return MAX_NODE_SCORE
    _, ids, is_min = numa_nodes_required(node, request)
    if ids is None:
        return MIN_NODE_SCORE
    return normalize_score(len(ids), is_min, max_numa)
