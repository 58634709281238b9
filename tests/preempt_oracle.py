"""CapacityScheduling.PostFilter's preemption dry run as literal Python loops on plain dicts: test infrastructure, nothing of the product.

    SelectVictimsOnNode            pkg/capacityscheduling/capacity_scheduling.go:486-677
    RemovePod / AddPod             :290-329, elasticquota.go:155-187 (addPodIfNotPresent / deletePodIfPresent on the `pods` set)
    PreFilter's nominated sums     :226-265
    filterPodsWithPDBViolation     :889-934
    PodEligibleToPreemptOthers     :409-484
    cmp / cmp2 and the over-min / over-max gates   elasticquota.go:48-59, :109-131, :189-221

Not in the reference tree and restated from upstream kube-scheduler: NodeResourcesFit's fitsRequest with default args (the only Filter the
reference's own tests register), "a node without victims is no candidate" (DryRunPreemption) and pickOneNodeForPreemption.

A Resource is {"v": [8 ints], "p": mask}: cpu milli, memory, ephemeral, pods, four scalar slots; bit s (4..7) of p = the scalar key exists in
the map (an absent key reads 0).  A pod is {"key", "ns", "prio", "start", "fit": [8] (what NodeInfo charges; fit[3] is ignored, a pod
counts once), "req": Resource (computePodResourceRequest), "pdbs": [ascending indices into snap["pdbs"] (the DisruptionsAllowed list) of the PDBs whose selector
matches it and that do not list it in DisruptedPods], "terminating", "row" (pending row of a nominated pod, or -1)}.

Ties in (priority, start time): sort.Slice is unstable in the reference; here every sort breaks them by the position in the node's list.
"""
from __future__ import annotations

S = 8
INT64_MAX = (1 << 63) - 1
ST = {"CANDIDATE": 0, "NO_VICTIMS": 1, "NOT_FIT": 2, "QUOTA": 3, "ALL_REPRIEVED": 4, "REMOVE_TWICE": 5, "SKIPPED": 6}


class RemoveTwice(Exception):
    """nodeInfo.RemovePod of a pod that is no longer on the node (:647 after :639)"""


def resource(v=None, p=0):
    return {"v": list(v) if v is not None else [0] * S, "p": p}


def r_add(a, b):  # framework.Resource.Add of util.ResourceList(b)
    for s in range(S):
        a["v"][s] += b["v"][s]
    a["p"] |= b["p"]


def cmp2(x1, x2, y, bound):  # elasticquota.go:193-221
    for s in range(4):
        if x1["v"][s] + x2["v"][s] > y["v"][s]:
            return True
    for s in range(4, S):
        if (x1["p"] >> s) & 1:
            yq = y["v"][s] if (y["p"] >> s) & 1 else bound
            if x1["v"][s] + x2["v"][s] > yq:
                return True
    return False


def cmp(x, y, bound):
    return cmp2(x, resource(), y, bound)


def used_over_min_with(eq, req):
    return cmp2(req, eq["used"], eq["min"], 0)


def used_over_max_with(eq, req):
    return cmp2(req, eq["used"], eq["max"], INT64_MAX)


def used_over_min(eq):
    return cmp(eq["used"], eq["min"], 0)


def aggregated_used_over_min_with(eqs, req):  # elasticquota.go:48-59
    used, mn = resource(), resource()
    for eq in eqs.values():
        r_add(used, eq["used"])
        r_add(mn, eq["min"])
    r_add(used, req)
    return cmp(used, mn, 0)


def delete_pod_if_present(eq, pod):  # elasticquota.go:172-187
    if pod["key"] not in eq["pods"]:
        return
    eq["pods"].discard(pod["key"])
    for s in range(S):
        eq["used"]["v"][s] -= pod["req"]["v"][s]
    eq["used"]["p"] |= pod["req"]["p"]  # SetScalar


def add_pod_if_not_present(eq, pod):  # elasticquota.go:155-170
    if pod["key"] in eq["pods"]:
        return
    eq["pods"].add(pod["key"])
    for s in range(S):
        eq["used"]["v"][s] += pod["req"]["v"][s]
    eq["used"]["p"] |= pod["req"]["p"]


def prefilter_state(snap, pre):
    """PreFilter's podReq and the two nominated sums (:226-265); None, None for a preemptor without quota"""
    eqs = snap["quotas"]
    if pre["ns"] not in eqs:
        return None, None
    in_eq, total = resource(), resource()
    for node in snap["nodes"]:
        if not node["present"]:
            continue
        for p in node["nominated"]:
            if p["row"] == pre["row"]:
                continue
            info = eqs.get(p["ns"])
            if info is None:
                continue
            if p["ns"] == pre["ns"] and p["prio"] >= pre["prio"]:
                r_add(in_eq, p["req"])
                r_add(total, p["req"])
            elif p["ns"] != pre["ns"] and not used_over_min(info):
                r_add(total, p["req"])
    r_add(in_eq, pre["req"])
    r_add(total, pre["req"])
    return in_eq, total


def fits(node, pods, requested, pre):
    """NodeResourcesFit with default args under RunFilterPluginsWithNominatedPods: the node's nominated pods of priority >= the preemptor's
    (other than itself) are added first; passing with them implies passing without them for this Filter"""
    n_pods = len(pods)
    req = list(requested)
    for p in node["nominated"]:
        if p["prio"] >= pre["prio"] and p["row"] != pre["row"]:
            n_pods += 1
            for s in range(S):
                if s != 3:
                    req[s] += p["fit"][s]
    if n_pods + 1 > node["alloc"][3]:
        return False
    if all(pre["fit"][s] == 0 for s in range(S) if s != 3):
        return True
    for s in range(S):
        if s != 3 and pre["fit"][s] > 0 and pre["fit"][s] > node["alloc"][s] - req[s]:
            return False
    return True


def walk_order(pods):
    """positions of the node's list, least important first (:537-539)"""
    return sorted(range(len(pods)), key=lambda i: (pods[i]["prio"], -pods[i]["start"], i))


def important_first(pods, positions):
    return sorted(positions, key=lambda i: (-pods[i]["prio"], pods[i]["start"], i))


def filter_pods_with_pdb_violation(pods, positions, pdbs):  # :889-934
    allowed = [b for b in pdbs]
    violating, rest = [], []
    for i in positions:
        hit = False
        for k in pods[i]["pdbs"]:  # ascending = the PDB list's order
            allowed[k] -= 1
            if allowed[k] < 0:
                hit = True
        (violating if hit else rest).append(i)
    return violating, rest


def select_victims_on_node(snap, pre, node, in_eq, total):
    """-> (status, victim positions in the node's list most important first, numViolatingVictim)"""
    eqs = dict(snap["quotas"])  # ElasticQuotaSnapshotState.Clone, made lazily: a quota is copied when this cell first writes to it
    cloned = set()

    def writable(ns):
        if ns not in cloned:
            eq = eqs[ns]
            eqs[ns] = {"min": eq["min"], "max": eq["max"], "used": resource(eq["used"]["v"], eq["used"]["p"]), "pods": set(eq["pods"])}
            cloned.add(ns)
        return eqs[ns]

    all_pods = node["pods"]
    on_node = set(range(len(all_pods)))  # nodeInfo.Pods of the node's clone
    requested = [0] * S
    for p in all_pods:
        for s in range(S):
            if s != 3:
                requested[s] += p["fit"][s]
    has_eq = pre["ns"] in eqs

    def remove_pod(i):
        if i not in on_node:
            raise RemoveTwice()
        on_node.discard(i)
        for s in range(S):
            if s != 3:
                requested[s] -= all_pods[i]["fit"][s]
        if all_pods[i]["ns"] in eqs:
            delete_pod_if_present(writable(all_pods[i]["ns"]), all_pods[i])

    def add_pod(i):
        on_node.add(i)
        for s in range(S):
            if s != 3:
                requested[s] += all_pods[i]["fit"][s]
        if all_pods[i]["ns"] in eqs:
            add_pod_if_not_present(writable(all_pods[i]["ns"]), all_pods[i])

    potential = []
    if has_eq:
        more_than_min = used_over_min_with(eqs[pre["ns"]], in_eq)
        for i in walk_order(all_pods):
            p = all_pods[i]
            info = eqs.get(p["ns"])
            if info is None:
                continue
            if more_than_min:
                if p["ns"] == pre["ns"] and p["prio"] < pre["prio"]:
                    potential.append(i)
                    remove_pod(i)
            elif p["ns"] != pre["ns"] and used_over_min(info):
                potential.append(i)
                remove_pod(i)
    else:
        for i in walk_order(all_pods):
            p = all_pods[i]
            if p["ns"] in eqs:
                continue
            if p["prio"] < pre["prio"]:
                potential.append(i)
                remove_pod(i)
    if not potential:
        return ST["NO_VICTIMS"], [], 0
    if not fits(node, on_node, requested, pre):
        return ST["NOT_FIT"], [], 0
    if has_eq and (used_over_max_with(eqs[pre["ns"]], pre["req"]) or aggregated_used_over_min_with(eqs, pre["req"])):
        return ST["QUOTA"], [], 0
    victims, n_violating = [], 0
    potential = important_first(all_pods, potential)
    violating, rest = filter_pods_with_pdb_violation(all_pods, potential, snap["pdbs"])

    def reprieve(i):
        add_pod(i)
        ok = fits(node, on_node, requested, pre)
        if not ok:
            remove_pod(i)
            victims.append(i)
        if has_eq and (used_over_max_with(eqs[pre["ns"]], in_eq) or aggregated_used_over_min_with(eqs, total)):
            remove_pod(i)
            victims.append(i)
        return ok

    try:
        for i in violating:
            if not reprieve(i):
                n_violating += 1
        for i in rest:
            reprieve(i)
    except RemoveTwice:
        return ST["REMOVE_TWICE"], [], 0
    if violating and rest:
        victims = important_first(all_pods, victims)
    if not victims:
        return ST["ALL_REPRIEVED"], [], 0
    return ST["CANDIDATE"], victims, n_violating


def cell(snap, pre, node, in_eq, total):
    """one (preemptor, node) cell: status, counts and the keys pickOneNodeForPreemption reads"""
    status, victims, n_violating = select_victims_on_node(snap, pre, node, in_eq, total)
    out = {"status": status, "victims": victims, "n_victims": len(victims), "n_violations": n_violating, "hi_prio": 0, "prio_sum": 0, "start": 0}
    if status == ST["CANDIDATE"]:
        pods = node["pods"]
        hi = max(pods[i]["prio"] for i in victims)
        out["hi_prio"] = hi
        out["prio_sum"] = sum(pods[i]["prio"] + (1 << 31) for i in victims)
        out["start"] = min(pods[i]["start"] for i in victims if pods[i]["prio"] == hi)
    return out


PICK_KEYS = (lambda c: c["n_violations"], lambda c: c["hi_prio"], lambda c: c["prio_sum"], lambda c: c["n_victims"], lambda c: -c["start"])


def pick_one_node(cells):
    """pickOneNodeForPreemption over the CANDIDATE cells of one preemptor: (node or -1, candidates, size of the final tie set, the level 1..6
    that decided; 0 with fewer than two candidates)"""
    cand = [n for n, c in enumerate(cells) if c["status"] == ST["CANDIDATE"]]
    n_cand = len(cand)
    if not cand:
        return -1, 0, 0, 0
    level = 6
    for k, key in enumerate(PICK_KEYS):
        best = min(key(cells[n]) for n in cand)
        cand = [n for n in cand if key(cells[n]) == best]
        if len(cand) == 1:
            level = min(level, k + 1)
    if n_cand == 1:
        level = 0  # upstream returns the only candidate before comparing anything
    return cand[0], n_cand, len(cand), level


def dry_run(snap, preemptors, node_mask=None):
    """-> per preemptor {"cells": [per node], "pick": (node, n_candidates, n_ties, level)}; node_mask[i][n] == 0 or an absent node: SKIPPED"""
    out = []
    for i, pre in enumerate(preemptors):
        in_eq, total = prefilter_state(snap, pre)
        cells = []
        for n, node in enumerate(snap["nodes"]):
            if not node["present"] or (node_mask is not None and not node_mask[i][n]):
                cells.append({"status": ST["SKIPPED"], "victims": [], "n_victims": 0, "n_violations": 0, "hi_prio": 0, "prio_sum": 0, "start": 0})
            else:
                cells.append(cell(snap, pre, node, in_eq, total))
        out.append({"cells": cells, "pick": pick_one_node(cells)})
    return out


def pod_eligible_to_preempt_others(snap, pre, in_eq, preempt_never, nominated_node, nominated_unresolvable):
    """PodEligibleToPreemptOthers (:409-484); nominated_node: index into snap["nodes"] or -1"""
    if preempt_never:
        return False
    if nominated_node < 0:
        return True
    if nominated_unresolvable:
        return True
    node = snap["nodes"][nominated_node]
    if not node["present"]:
        return True
    eqs = snap["quotas"]
    pre_eq = eqs.get(pre["ns"])
    if pre_eq is not None:
        more_than_min = used_over_min_with(pre_eq, in_eq)
        for p in node["pods"]:
            if p["terminating"]:
                info = eqs.get(p["ns"])
                if info is None:
                    continue
                if p["ns"] == pre["ns"] and p["prio"] < pre["prio"]:
                    return False
                if p["ns"] != pre["ns"] and not more_than_min and used_over_min(info):
                    return False
    else:
        for p in node["pods"]:
            if p["ns"] in eqs:
                continue
            if p["terminating"] and p["prio"] < pre["prio"]:
                return False
    return True
