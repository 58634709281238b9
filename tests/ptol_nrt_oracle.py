"""PreemptionToleration's dry run with NodeResourceTopologyMatch's Filter in the refit, as literal Python loops on plain dicts: test
infrastructure, nothing of the product.

    SelectVictimsOnNode                pkg/preemptiontoleration/preemption_toleration.go:188-299 (RunFilterPluginsWithNominatedPods at :250, :268)
    TopologyMatch.Filter               pkg/noderesourcetopology/filter.go:179-245, the handlers :42-176
    PreFilter / AddPod / RemovePod     pkg/noderesourcetopology/prefilter.go:51-102 (the preemption stack)
    GetNRTPostPodsEviction             pkg/noderesourcetopology/preemption/preemption.go:39-157
    IsExclusive                        pkg/noderesourcetopology/resourcerequests/exclusive.go:78-102
    subtractResourcesFromNUMANodeList  pkg/noderesourcetopology/numaresources.go:137-182 (its error, :172-175, is the Filter's fwk.Error)

The model is ptol_oracle's, decorated.  A node: "nrt" (None = the cache has none) = {"zones": [{"name", "resources": [(resource name,
allocatable, available)]}], "policy", "scope"} with every zone of type Node, "nrt_fresh", "alloc_names" (the keys of the node's
allocatable) and "placement" (None = no placement info, else {(pod key, container name): NUMA id or -1}; a missing key is a failed lookup).
A pod, assigned or pending: "containers" and "init_containers" = [{"name", "requests": {name: quantity}, "limits": {...}}], cpu in
millicores.  Nothing here knows the flattener's encoding: zones are found by their names, releases are summed per call from the container
requests, and the zone table is copied and changed for every Filter call.

ExemptedFromPreemption, NodeResourcesFit with the nominated pods, the order of MoreImportantPod, filterPodsWithPDBViolation and
pickOneNodeForPreemption are ptol_oracle's and preempt_oracle's.
"""
from __future__ import annotations

import preempt_oracle as PO
import ptol_oracle as TO

ST = TO.ST
GUARANTEED, BURSTABLE, BESTEFFORT = "Guaranteed", "Burstable", "BestEffort"
# the Filter's messages
INVALID_TOPOLOGY = "invalid node topology data"
NOTHING_TO_ADD = "eviction simulation in NRT is not possible:no resources to add, cannot process eviction simulation"
EXCEEDS = "eviction simulation in NRT is not possible:resource release request exceeds NUMA allocatable"
CANNOT_ALIGN = {"init": "cannot align init container", "app": "cannot align container", "pod": "cannot align pod"}
ACCOUNTING = "inconsistent resource accounting"  # fwk.Error, not Unschedulable (filter.go:73-77): a Filter that did not succeed all the same
CHECK_ACCOUNTING = True  # False: subtractResourcesFromNUMANodeList without its sign test (see subtract); only tests switch it


def is_native(name):  # v1helper.IsNativeResource
    return "/" not in name or "kubernetes.io/" in name


def is_hugepage(name):
    return name.startswith("hugepages-")


def is_numa_affine(name):  # numaresources.go:120-135
    return name in ("cpu", "memory") or is_hugepage(name)


def is_host_level(name):  # numaresources.go:105-118
    return name in ("ephemeral-storage", "storage") or not is_native(name)


def all_containers(pod):
    return list(pod.get("init_containers", [])) + list(pod["containers"])


def pod_qos(pod):
    """v1qos.ComputePodQOS over cpu and memory; zero quantities are ignored"""
    requests, limits, guaranteed = {}, {}, True
    for c in all_containers(pod):
        for name, q in c.get("requests", {}).items():
            if name in ("cpu", "memory") and q > 0:
                requests[name] = requests.get(name, 0) + q
        found = set()
        for name, q in c.get("limits", {}).items():
            if name in ("cpu", "memory") and q > 0:
                found.add(name)
                limits[name] = limits.get(name, 0) + q
        if found != {"cpu", "memory"}:
            guaranteed = False
    if not requests and not limits:
        return BESTEFFORT
    if guaranteed:
        for name, q in requests.items():
            if limits.get(name) != q:
                guaranteed = False
    if guaranteed and len(requests) == len(limits):
        return GUARANTEED
    return BURSTABLE


def include_non_native(pod):  # resourcerequests.IncludeNonNative: any container, init ones included
    return any(not is_native(name) for c in all_containers(pod) for name in c.get("requests", {}))


def is_exclusive(name, q, qos, reported):  # exclusive.go:78-102
    if not is_native(name):
        return name in reported
    if qos != GUARANTEED:
        return False
    if name == "cpu":
        return q > 0 and q % 1000 == 0
    if name == "memory" or is_hugepage(name):
        return q > 0
    return False


def numa_id(zone_name):  # numanode.NameToID
    if not zone_name.startswith("node-"):
        return -1
    try:
        return int(zone_name[len("node-"):])
    except ValueError:
        return -1


def post_eviction(zones, stack, placement):
    """GetNRTPostPodsEviction on a copy of `zones` ([{"name", "resources": [[name, allocatable, available]]}]): (zones, None) or
    (None, message)"""
    reported = {r[0] for z in zones for r in z["resources"]}  # cache.ResourceNamesFromNRT
    releases = {}
    for pod in stack:
        qos = pod_qos(pod)
        if qos != GUARANTEED and not include_non_native(pod):
            continue
        for c in pod["containers"]:
            key = (pod["key"], c["name"])
            if key not in placement or placement[key] == -1:
                continue
            for name, q in c["requests"].items():
                if is_exclusive(name, q, qos, reported):
                    at = (placement[key], name)
                    releases[at] = releases.get(at, 0) + q
    if not releases:
        return None, NOTHING_TO_ADD
    for z in zones:
        zid = numa_id(z["name"])
        if zid < 0:
            continue
        for (numa, name), q in releases.items():
            if numa != zid:
                continue
            for r in z["resources"]:
                if r[0] == name:
                    if r[2] + q > r[1]:
                        return None, EXCEEDS
                    r[2] += q
                    break  # the first ResourceInfo of that name
    return zones, None


def fits_any(numa_nodes, requests, qos, alloc_names):
    """resourcesAvailableInAnyNUMANodes (filter.go:93-163): the lowest NUMA id every requested resource fits on, or None"""
    ids = set(range(64))
    for name, q in requests.items():
        if q == 0:
            continue
        if name not in alloc_names:
            return None
        has_affinity, fit = False, set()
        for z in numa_nodes:
            if name not in z["res"]:
                continue
            has_affinity = True
            if (qos != GUARANTEED and is_numa_affine(name)) or z["res"][name] >= q:  # isResourceSetSuitable
                fit.add(z["id"])
        if not has_affinity and is_host_level(name):
            continue
        ids &= fit
        if not ids:
            return None
    return min(ids)


def subtract(numa_nodes, requests, qos, chosen, check=True):
    """every zone that carries the id is charged; False = a remainder below zero (numaresources.go:172-175: two zones share the id and
    only one of them holds the request), where the reference stops with an error.  check=False: the charge without that test, as this
    oracle and the kernels read it before — kept for the tests that show where the two readings part"""
    for z in numa_nodes:
        if z["id"] != chosen:
            continue
        for name, q in requests.items():
            if qos != GUARANTEED and is_numa_affine(name):
                continue
            if q == 0 or name not in z["res"]:
                continue
            if check and z["res"][name] - q < 0:
                return False
            z["res"][name] -= q
    return True


def effective_request(pod):  # GetPodEffectiveRequest without overhead
    out = {}
    for c in pod["containers"]:
        for name, q in c["requests"].items():
            out[name] = out.get(name, 0) + q
    for c in pod.get("init_containers", []):
        for name, q in c["requests"].items():
            if name not in out or q > out[name]:
                out[name] = q
    return out


def single_numa(zones, pre, scope, alloc_names):
    """the pod-scope or container-scope handler (filter.go:42-176) on a private NUMA node list: None, or the message"""
    numa_nodes = [{"id": numa_id(z["name"]), "res": {r[0]: r[2] for r in z["resources"]}} for z in zones if numa_id(z["name"]) >= 0]
    qos = pod_qos(pre)
    if scope == "pod":
        return None if fits_any(numa_nodes, effective_request(pre), qos, alloc_names) is not None else CANNOT_ALIGN["pod"]
    for c in pre.get("init_containers", []):  # must fit, never subtracted
        if fits_any(numa_nodes, c["requests"], qos, alloc_names) is None:
            return CANNOT_ALIGN["init"]
    for c in pre["containers"]:
        chosen = fits_any(numa_nodes, c["requests"], qos, alloc_names)
        if chosen is None:
            return CANNOT_ALIGN["app"]
        if not subtract(numa_nodes, c["requests"], qos, chosen, CHECK_ACCOUNTING):
            return ACCOUNTING
    return None


def nrt_filter(node, pre, stack, mode, trace=None):
    """F(p, n, stack): None = pass, else the message.  stack: the node's pods that are currently removed; mode: preemption mode enabled
    (prefilter.go:52: without it the stack is never kept).  trace: a set that collects which way the call went."""
    note = (lambda what: trace.add(what)) if trace is not None else (lambda what: None)
    if pod_qos(pre) == BESTEFFORT and not include_non_native(pre):
        note("exempt")
        return None
    if not node["nrt_fresh"]:
        note("stale")
        return INVALID_TOPOLOGY
    nrt = node["nrt"]
    if nrt is None:
        note("no-nrt")
        return None
    zones = [{"name": z["name"], "resources": [list(r) for r in z["resources"]]} for z in nrt["zones"]]
    victims = list(stack) if mode else []
    simulated = False
    if not victims:
        note("empty-stack")
    if victims and node["placement"] is not None and len(node["placement"]) != 0:
        zones, message = post_eviction(zones, victims, node["placement"])
        if message is not None:
            note(("nothing-to-add" if message == NOTHING_TO_ADD else "exceeds") + ("" if nrt["policy"] == "single-numa-node" else "/not-single"))
            return message
        simulated = True
    if nrt["policy"] != "single-numa-node":
        note("not-single/simulated" if simulated else "not-single")
        return None
    note("scope-" + nrt["scope"])
    message = single_numa(zones, pre, nrt["scope"], node["alloc_names"])
    if message == CANNOT_ALIGN["init"]:
        note("init-container-fails")
    if message == ACCOUNTING:
        note("accounting-error")
    return message


def select_victims_on_node(snap, pre, node, mode=True, trace=None, fit_only_trace=None):
    """ptol_oracle.select_victims_on_node with the refit NodeResourcesFit-with-nominated && F.  fit_only_trace: a list that receives
    ("kept-by-F", position) for every victim NodeResourcesFit alone would have reprieved, and ("not-fit-by-F",) when F alone fails at
    the first refit."""
    all_pods = node["pods"]
    on_node = set(range(len(all_pods)))
    stack = []  # NRT's preemption stack: positions in removal order
    requested = [0] * TO.S
    for p in all_pods:
        for s in range(TO.S):
            if s != 3:
                requested[s] += p["fit"][s]

    def remove_pod(i):
        on_node.discard(i)
        stack.append(i)
        for s in range(TO.S):
            if s != 3:
                requested[s] -= all_pods[i]["fit"][s]

    def add_pod(i):
        on_node.add(i)
        stack.remove(i)
        for s in range(TO.S):
            if s != 3:
                requested[s] += all_pods[i]["fit"][s]

    def refit(why=None):
        fit = PO.fits(node, on_node, requested, pre)
        f = nrt_filter(node, pre, [all_pods[i] for i in stack], mode, trace) is None if fit else True  # the framework stops at the first failing Filter
        if fit and not f and fit_only_trace is not None and why is not None:
            fit_only_trace.append(why)
        return fit and f

    potential = []
    for i, p in enumerate(all_pods):
        if p["prio"] >= pre["prio"]:
            continue
        try:
            ex, _ = TO.exempted(snap["classes"], p, pre, snap["now"])
        except TO.ClassNotFound:
            return ST["CLASS_ERROR"], [], 0
        if not ex:
            potential.append(i)
            remove_pod(i)
    if not potential:
        return ST["NO_VICTIMS"], [], 0
    if not refit(("not-fit-by-F",)):
        return ST["NOT_FIT"], [], 0
    victims, n_violating = [], 0
    potential = PO.important_first(all_pods, potential)
    violating, rest = PO.filter_pods_with_pdb_violation(all_pods, potential, snap["pdbs"])

    def reprieve(i):
        add_pod(i)
        ok = refit(("kept-by-F", i))
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
        return ST["ALL_REPRIEVED"], [], 0
    return ST["CANDIDATE"], victims, n_violating


def cell(snap, pre, node, mode=True, trace=None, fit_only_trace=None):
    status, victims, n_violating = select_victims_on_node(snap, pre, node, mode, trace, fit_only_trace)
    out = {"status": status, "victims": victims, "n_victims": len(victims), "n_violations": n_violating, "hi_prio": 0, "prio_sum": 0, "start": 0}
    if status == ST["CANDIDATE"]:
        pods = node["pods"]
        hi = max(pods[i]["prio"] for i in victims)
        out["hi_prio"] = hi
        out["prio_sum"] = sum(pods[i]["prio"] + (1 << 31) for i in victims)
        out["start"] = min(pods[i]["start"] for i in victims if pods[i]["prio"] == hi)
    return out


def dry_run(snap, preemptors, node_mask=None, mode=True, trace=None, fit_only_trace=None):
    """as ptol_oracle.dry_run"""
    out = []
    for i, pre in enumerate(preemptors):
        cells = []
        for n, node in enumerate(snap["nodes"]):
            if not node["present"] or (node_mask is not None and not node_mask[i][n]):
                cells.append({"status": ST["SKIPPED"], "victims": [], "n_victims": 0, "n_violations": 0, "hi_prio": 0, "prio_sum": 0, "start": 0})
            else:
                cells.append(cell(snap, pre, node, mode, trace, fit_only_trace))
        out.append({"cells": cells, "pick": PO.pick_one_node(cells)})
    return out
