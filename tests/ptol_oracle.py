"""PreemptionToleration.PostFilter's preemption dry run as literal Python loops on plain dicts: test infrastructure, nothing of the product.

    parsePreemptionTolerationPolicy   pkg/preemptiontoleration/preemption_toleration_policy.go:55-83
    ExemptedFromPreemption            pkg/preemptiontoleration/preemption_toleration.go:129-181
    SelectVictimsOnNode               :188-299
    PodEligibleToPreemptOthers        :339-364

The model is preempt_oracle's without quotas, decorated: snap["classes"] = {name: {"value", "annotations": {key: text}}}, snap["now"] (ns),
a pod's "pc" (PriorityClassName, "" = none) and "scheduled_at" (ns of its PodScheduled=True condition, None = no such condition), a
preemptor's "never".  Nothing here knows the flattener's encoding: the policy is parsed from the annotation texts for every pair.

NodeResourcesFit with the nominated pods, the order of MoreImportantPod with ties by position, filterPodsWithPDBViolation and
pickOneNodeForPreemption are preempt_oracle's: this plugin copies them from the same upstream code.
"""
from __future__ import annotations

import preempt_oracle as PO

S = 8
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
ST = dict(PO.ST, CLASS_ERROR=7)
ANNOTATION_MIN = "preemption-toleration.scheduling.x-k8s.io/minimum-preemptable-priority"
ANNOTATION_TOLERATION = "preemption-toleration.scheduling.x-k8s.io/toleration-seconds"
# the exits of ExemptedFromPreemption, in its order
EXITS = ("NO_CLASS_NAME", "CLASS_NOT_FOUND", "PREEMPT_NEVER", "POLICY_ERROR", "PRIORITY_REACHES_MINIMUM", "TOLERATES_FOR_EVER", "NOT_SCHEDULED", "BY_TIME")


class ClassNotFound(Exception):
    """pcLister.Get failed (:139-142)"""


def wrap(v: int, bits: int) -> int:
    """two's complement wrap of an integer to `bits` bits, as Go's fixed-width arithmetic does"""
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def parse_int(s: str, bits: int):
    """strconv.ParseInt(s, 10, bits): the value, or None for an error.  Base 10: one optional sign, then ASCII digits only."""
    if s == "":
        return None
    neg, digits = False, s
    if s[0] in "+-":
        neg, digits = s[0] == "-", s[1:]
    if digits == "" or any(c not in "0123456789" for c in digits):
        return None
    v = 0
    for c in digits:
        v = v * 10 + (ord(c) - ord("0"))
    v = -v if neg else v
    if v < -(1 << (bits - 1)) or v > (1 << (bits - 1)) - 1:
        return None  # ErrRange
    return v


def parse_policy(pc: dict):
    """-> (MinimumPreemptablePriority, TolerationSeconds), or None for an error"""
    ann = pc["annotations"]
    if ANNOTATION_MIN not in ann:
        mn = wrap(pc["value"] + 1, 32)
    else:
        mn = parse_int(ann[ANNOTATION_MIN], 32)
        if mn is None:
            return None
    if ANNOTATION_TOLERATION not in ann:
        tol = 0
    else:
        tol = parse_int(ann[ANNOTATION_TOLERATION], 64)
        if tol is None:
            return None
    return mn, tol


def exempted(classes: dict, victim: dict, pre: dict, now: int):
    """-> (exempted, the exit taken); raises ClassNotFound"""
    if victim["pc"] == "":
        return False, "NO_CLASS_NAME"
    if victim["pc"] not in classes:
        raise ClassNotFound(victim["pc"])
    if pre["never"]:
        return True, "PREEMPT_NEVER"
    policy = parse_policy(classes[victim["pc"]])
    if policy is None:
        return False, "POLICY_ERROR"
    mn, tol = policy
    if pre["prio"] >= mn:
        return False, "PRIORITY_REACHES_MINIMUM"
    if tol < 0:
        return True, "TOLERATES_FOR_EVER"
    if victim["scheduled_at"] is None:
        return True, "NOT_SCHEDULED"
    duration = wrap(tol * 10**9, 64)  # time.Duration(TolerationSeconds) * time.Second
    return victim["scheduled_at"] + duration > now, "BY_TIME"  # Time.Add does not wrap; After is strict


def select_victims_on_node(snap, pre, node, exits=None):
    """-> (status, victim positions in the node's list most important first, numViolatingVictim); exits: a set that collects the exits
    ExemptedFromPreemption took"""
    all_pods = node["pods"]
    on_node = set(range(len(all_pods)))
    requested = [0] * S
    for p in all_pods:
        for s in range(S):
            if s != 3:
                requested[s] += p["fit"][s]

    def remove_pod(i):
        on_node.discard(i)
        for s in range(S):
            if s != 3:
                requested[s] -= all_pods[i]["fit"][s]

    def add_pod(i):
        on_node.add(i)
        for s in range(S):
            if s != 3:
                requested[s] += all_pods[i]["fit"][s]

    potential = []
    for i, p in enumerate(all_pods):  # nodeInfo.GetPods(), :218
        if p["prio"] >= pre["prio"]:
            continue
        try:
            ex, how = exempted(snap["classes"], p, pre, snap["now"])
        except ClassNotFound:
            if exits is not None:
                exits.add("CLASS_NOT_FOUND")
            return ST["CLASS_ERROR"], [], 0
        if exits is not None:
            exits.add(how)
        if not ex:
            potential.append(i)
            remove_pod(i)
    if not potential:
        return ST["NO_VICTIMS"], [], 0
    if not PO.fits(node, on_node, requested, pre):
        return ST["NOT_FIT"], [], 0
    victims, n_violating = [], 0
    potential = PO.important_first(all_pods, potential)
    violating, rest = PO.filter_pods_with_pdb_violation(all_pods, potential, snap["pdbs"])

    def reprieve(i):
        add_pod(i)
        ok = PO.fits(node, on_node, requested, pre)
        if not ok:
            remove_pod(i)
            victims.append(i)
        return ok

    for i in violating:
        if not reprieve(i):
            n_violating += 1
    for i in rest:
        reprieve(i)
    if violating and rest:
        victims = PO.important_first(all_pods, victims)
    if not victims:
        return ST["ALL_REPRIEVED"], [], 0  # upstream's DryRunPreemption drops a node without victims
    return ST["CANDIDATE"], victims, n_violating


def cell(snap, pre, node, exits=None):
    status, victims, n_violating = select_victims_on_node(snap, pre, node, exits)
    out = {"status": status, "victims": victims, "n_victims": len(victims), "n_violations": n_violating, "hi_prio": 0, "prio_sum": 0, "start": 0}
    if status == ST["CANDIDATE"]:
        pods = node["pods"]
        hi = max(pods[i]["prio"] for i in victims)
        out["hi_prio"] = hi
        out["prio_sum"] = sum(pods[i]["prio"] + (1 << 31) for i in victims)
        out["start"] = min(pods[i]["start"] for i in victims if pods[i]["prio"] == hi)
    return out


def dry_run(snap, preemptors, node_mask=None, exits=None):
    """-> per preemptor {"cells": [per node], "pick": (node, n_candidates, n_ties, level)}; node_mask[i][n] == 0 or an absent node: SKIPPED"""
    out = []
    for i, pre in enumerate(preemptors):
        cells = []
        for n, node in enumerate(snap["nodes"]):
            if not node["present"] or (node_mask is not None and not node_mask[i][n]):
                cells.append({"status": ST["SKIPPED"], "victims": [], "n_victims": 0, "n_violations": 0, "hi_prio": 0, "prio_sum": 0, "start": 0})
            else:
                cells.append(cell(snap, pre, node, exits))
        out.append({"cells": cells, "pick": PO.pick_one_node(cells)})
    return out


def pod_eligible_to_preempt_others(snap, pre, nominated_node, nominated_unresolvable):
    """PodEligibleToPreemptOthers (:339-364); nominated_node: index into snap["nodes"] or -1"""
    if pre["never"]:
        return False
    if nominated_node >= 0:
        if nominated_unresolvable:
            return True
        node = snap["nodes"][nominated_node]
        if node["present"]:
            for p in node["pods"]:
                if p["terminating"] and p["prio"] < pre["prio"]:
                    return False
    return True
