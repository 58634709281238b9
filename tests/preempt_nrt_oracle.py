"""CapacityScheduling's preemption dry run with NodeResourceTopologyMatch's Filter in the refit, as literal Python loops on plain dicts:
test infrastructure, nothing of the product.

    SelectVictimsOnNode                pkg/capacityscheduling/capacity_scheduling.go:486-677
    removePod / addPod                 :513, :523 (RunPreFilterExtensionRemovePod / AddPod: every PreFilter plugin's, NRT's among them)
    the Filter runs                    :607 (after the potential victims are gone), :636 (inside reprievePod)
    TopologyMatch.Filter and the rest  tests/ptol_nrt_oracle.py (nrt_filter: F(p, n, stack))

The walk is preempt_oracle.select_victims_on_node written out again with NRT's preemption stack next to the node's clone: removePod
pushes, addPod pops, and both refits are NodeResourcesFit-with-nominated && F.  The removal for the quota (:646-649) is a removePod like
any other: that pod is on the stack at every later Filter run of the cell.  The model is preempt_oracle's, decorated as
ptol_nrt_oracle describes (containers, zones, placement info).  cmp2, the quota gates, PreFilter's sums, NodeResourcesFit, the orders,
the PDB filter and pickOneNodeForPreemption are preempt_oracle's; cell and dry_run are its with the mode and the traces passed through.
"""
from __future__ import annotations

import preempt_oracle as PO
import ptol_nrt_oracle as NO

ST = PO.ST
S = PO.S


def select_victims_on_node(snap, pre, node, in_eq, total, mode=True, trace=None, events=None):
    """-> (status, victim positions in the node's list most important first, numViolatingVictim).  trace: a set that collects which way
    each Filter call went (ptol_nrt_oracle.nrt_filter's notes).  events: a list that receives, for this cell,
        ("not-fit-by-F",)            F alone fails at :607
        ("f-passed",)                F ran at :607 and passed
        ("quota",)                   the cell ends at :613 as QUOTA
        ("kept-by-F", position)      a victim NodeResourcesFit alone would have reprieved
        ("again", position, stack size before it is pushed)   a pod that fits and is removed for the quota"""
    say = events.append if events is not None else (lambda what: None)
    eqs = dict(snap["quotas"])  # ElasticQuotaSnapshotState.Clone, made lazily: a quota is copied when this cell first writes to it
    cloned = set()

    def writable(ns):
        if ns not in cloned:
            eq = eqs[ns]
            eqs[ns] = {"min": eq["min"], "max": eq["max"], "used": PO.resource(eq["used"]["v"], eq["used"]["p"]), "pods": set(eq["pods"])}
            cloned.add(ns)
        return eqs[ns]

    all_pods = node["pods"]
    on_node = set(range(len(all_pods)))  # nodeInfo.Pods of the node's clone
    stack = []  # NRT's preemption stack: positions in removal order
    requested = [0] * S
    for p in all_pods:
        for s in range(S):
            if s != 3:
                requested[s] += p["fit"][s]
    has_eq = pre["ns"] in eqs

    def remove_pod(i):
        if i not in on_node:
            raise PO.RemoveTwice()
        on_node.discard(i)
        stack.append(i)
        for s in range(S):
            if s != 3:
                requested[s] -= all_pods[i]["fit"][s]
        if all_pods[i]["ns"] in eqs:
            PO.delete_pod_if_present(writable(all_pods[i]["ns"]), all_pods[i])

    def add_pod(i):
        on_node.add(i)
        stack.remove(i)
        for s in range(S):
            if s != 3:
                requested[s] += all_pods[i]["fit"][s]
        if all_pods[i]["ns"] in eqs:
            PO.add_pod_if_not_present(writable(all_pods[i]["ns"]), all_pods[i])

    def refit():
        """-> (NodeResourcesFit, F or None when the framework stopped at NodeResourcesFit)"""
        fit = PO.fits(node, on_node, requested, pre)
        if not fit:
            return False, None
        return True, NO.nrt_filter(node, pre, [all_pods[i] for i in stack], mode, trace) is None

    potential = []
    if has_eq:
        more_than_min = PO.used_over_min_with(eqs[pre["ns"]], in_eq)
        for i in PO.walk_order(all_pods):
            p = all_pods[i]
            info = eqs.get(p["ns"])
            if info is None:
                continue
            if more_than_min:
                if p["ns"] == pre["ns"] and p["prio"] < pre["prio"]:
                    potential.append(i)
                    remove_pod(i)
            elif p["ns"] != pre["ns"] and PO.used_over_min(info):
                potential.append(i)
                remove_pod(i)
    else:
        for i in PO.walk_order(all_pods):
            p = all_pods[i]
            if p["ns"] in eqs:
                continue
            if p["prio"] < pre["prio"]:
                potential.append(i)
                remove_pod(i)
    if not potential:
        return ST["NO_VICTIMS"], [], 0
    fit, f = refit()
    if not (fit and f):
        if fit:
            say(("not-fit-by-F",))
        return ST["NOT_FIT"], [], 0
    say(("f-passed",))
    if has_eq and (PO.used_over_max_with(eqs[pre["ns"]], pre["req"]) or PO.aggregated_used_over_min_with(eqs, pre["req"])):
        say(("quota",))
        return ST["QUOTA"], [], 0
    victims, n_violating = [], 0
    potential = PO.important_first(all_pods, potential)
    violating, rest = PO.filter_pods_with_pdb_violation(all_pods, potential, snap["pdbs"])

    def reprieve(i):
        add_pod(i)
        fit, f = refit()
        ok = fit and f
        if fit and not f:
            say(("kept-by-F", i))
        if not ok:
            remove_pod(i)
            victims.append(i)
        if has_eq and (PO.used_over_max_with(eqs[pre["ns"]], in_eq) or PO.aggregated_used_over_min_with(eqs, total)):
            if ok:
                say(("again", i, len(stack)))
            remove_pod(i)
            victims.append(i)
        return ok

    try:
        for i in violating:
            if not reprieve(i):
                n_violating += 1
        for i in rest:
            reprieve(i)
    except PO.RemoveTwice:
        return ST["REMOVE_TWICE"], [], 0
    if violating and rest:
        victims = PO.important_first(all_pods, victims)
    if not victims:
        return ST["ALL_REPRIEVED"], [], 0
    return ST["CANDIDATE"], victims, n_violating


def cell(snap, pre, node, in_eq, total, mode=True, trace=None, events=None):
    """preempt_oracle.cell over this walk: status, counts and the keys pickOneNodeForPreemption reads"""
    status, victims, n_violating = select_victims_on_node(snap, pre, node, in_eq, total, mode, trace, events)
    out = {"status": status, "victims": victims, "n_victims": len(victims), "n_violations": n_violating, "hi_prio": 0, "prio_sum": 0, "start": 0}
    if status == ST["CANDIDATE"]:
        pods = node["pods"]
        hi = max(pods[i]["prio"] for i in victims)
        out["hi_prio"] = hi
        out["prio_sum"] = sum(pods[i]["prio"] + (1 << 31) for i in victims)
        out["start"] = min(pods[i]["start"] for i in victims if pods[i]["prio"] == hi)
    return out


def dry_run(snap, preemptors, node_mask=None, mode=True, trace=None, events=None):
    """as preempt_oracle.dry_run.  events: a dict (row index, node) -> that cell's list of events"""
    out = []
    for i, pre in enumerate(preemptors):
        in_eq, total = PO.prefilter_state(snap, pre)
        cells = []
        for n, node in enumerate(snap["nodes"]):
            if not node["present"] or (node_mask is not None and not node_mask[i][n]):
                cells.append({"status": ST["SKIPPED"], "victims": [], "n_victims": 0, "n_violations": 0, "hi_prio": 0, "prio_sum": 0, "start": 0})
            else:
                log = [] if events is not None else None
                cells.append(cell(snap, pre, node, in_eq, total, mode, trace, log))
                if log:
                    events[(i, n)] = log
        out.append({"cells": cells, "pick": PO.pick_one_node(cells)})
    return out
