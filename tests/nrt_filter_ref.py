"""NodeResourceTopologyMatch's single-NUMA Filter in plain Python, written from pkg/noderesourcetopology/filter.go
(singleNUMAContainerLevelHandler :42-81, resourcesAvailableInAnyNUMANodes :93-163, singleNUMAPodLevelHandler :165-176, Filter :179-245)
and numaresources.go (isHostLevelResource :105-118, isNUMAAffineResource :120-135, isResourceSetSuitable :137-142,
subtractResourcesFromNUMANodeList :145-182) — a second anchor for the oracle's status where zones share a NUMA id, which the
reference's own test tables do not reach.

No short cut of any kind: the NUMA node list is copied per call, every zone is visited in list order, and a charge stops at the first
remainder below zero, as the Go code does.  Quantities are Python integers (cpu in millicores).

A node is a list of zones in NRT list order, {"id": NUMA id, "resources": {name: int}}; a pod is {"containers": [...],
"init_containers": [...]} with each container {"requests": {name: int}, "limits": {name: int}, "sidecar": bool}.  The status is the
status table's: 0 pass, 1 invalid topology, 2 / 3 an init / sidecar container, 4 a container, 5 the pod, 255 fwk.Error.

Pod scope takes the sum of the app containers, raised to each init container's request (GetPodEffectiveRequest without overhead);
a sidecar is read as an init container there, which is enough for examples whose sidecars fit either everywhere or nowhere."""
from ptol_nrt_oracle import BESTEFFORT, GUARANTEED, include_non_native, is_host_level, is_numa_affine, pod_qos

INVALID, INIT, SIDECAR, CONTAINER, POD, ERROR = 1, 2, 3, 4, 5, 255


def fits_any(numa_nodes, requests, qos, alloc_names):
    """the lowest NUMA id every requested resource fits on, or None"""
    bitmask = set(range(64))
    for name, quantity in requests.items():
        if quantity == 0:
            continue
        if name not in alloc_names:
            return None
        has_affinity, resource_bitmask = False, set()
        for node in numa_nodes:
            if name not in node["resources"]:
                continue
            has_affinity = True
            if not ((qos != GUARANTEED and is_numa_affine(name)) or node["resources"][name] >= quantity):
                continue
            resource_bitmask.add(node["id"])
        if not has_affinity and is_host_level(name):
            continue
        bitmask &= resource_bitmask
        if not bitmask:
            return None
    return min(bitmask)


def subtract(numa_nodes, numa_id, qos, requests):
    """False = the reference's error: a remainder below zero"""
    for node in numa_nodes:
        if node["id"] != numa_id:
            continue
        for name, quantity in requests.items():
            if qos != GUARANTEED and is_numa_affine(name):
                continue
            if quantity == 0 or name not in node["resources"]:
                continue
            left = node["resources"][name] - quantity
            if left < 0:
                return False
            node["resources"][name] = left
    return True


def container_level(numa_nodes, pod, qos, alloc_names):
    for c in pod["init_containers"]:
        if fits_any(numa_nodes, c["requests"], qos, alloc_names) is None:
            return SIDECAR if c["sidecar"] else INIT
    for c in pod["containers"]:
        numa_id = fits_any(numa_nodes, c["requests"], qos, alloc_names)
        if numa_id is None:
            return CONTAINER
        if not subtract(numa_nodes, numa_id, qos, c["requests"]):
            return ERROR
    return 0


def pod_level(numa_nodes, pod, qos, alloc_names):
    request = {}
    for c in pod["containers"]:
        for name, q in c["requests"].items():
            request[name] = request.get(name, 0) + q
    for c in pod["init_containers"]:
        for name, q in c["requests"].items():
            request[name] = max(request.get(name, 0), q)
    return 0 if fits_any(numa_nodes, request, qos, alloc_names) is not None else POD


def filter_status(zones, pod, fresh, policy, alloc_names):
    """zones: None = the node has no NRT object; policy: "container", "pod" or None (not single-NUMA)"""
    qos = pod_qos(pod)
    if qos == BESTEFFORT and not include_non_native(pod):
        return 0
    if not fresh:
        return INVALID
    if zones is None or policy is None:
        return 0
    numa_nodes = [{"id": z["id"], "resources": dict(z["resources"])} for z in zones]
    return (pod_level if policy == "pod" else container_level)(numa_nodes, pod, qos, alloc_names)
