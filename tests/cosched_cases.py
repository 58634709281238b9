"""Shared by the Coscheduling tests: snapshots as plain data (the form tests/cosched_oracle.py reads), their conversion to the
object tables, what the literal oracle expects of them, the closed form recomputed from flattened columns, and a seeded generator of
snapshots that reach every status and every kernel path."""
from fractions import Fraction

import numpy as np

import cosched_oracle as CO
from scheduler_plugins_amd import objects as O

LABEL = O.POD_GROUP_LABEL
SCALAR = "example.com/gpu"


def make_pod(namespace, name, group=None, gated=False, requests=None):
    return O.cosched_pod(namespace, name, {LABEL: group} if group else {}, gated, None, requests)


def build(hdr, snap):
    """snapshot -> (res, spx_node_objects, spx_cosched_objects).  snap: nodes (oracle form), groups [O.pod_group(..)], pending [pod],
    other_listed [pod]"""
    res = O.Resources()
    for k in ("cpu", "memory", "pods", SCALAR):  # fixed ids whatever the snapshot names first
        res.id(k)
    nodes = O.build_node_objects(hdr, res, [O.node(n["allocatable"]) for n in snap["nodes"]])
    assigned = [dict(p, node=i) for i, n in enumerate(snap["nodes"]) for p in n["pods"]]
    objects = O.build_cosched_objects(hdr, res, snap["groups"], snap["pending"], assigned, [n["present"] for n in snap["nodes"]], snap.get("other_listed", ()))
    return res, nodes, objects


def group_key(g):
    return O.pod_group_full_name(g["namespace"], g["name"])


def expected(snap, res, slot_res):
    """the literal oracle's answers: status per pending pod, and per group of snap["groups"] (pass_mask, open_mask, {slot: gap})"""
    existing = {group_key(g): g for g in snap["groups"] if g.get("exists", True)}
    listed = list(snap["pending"]) + [p for n in snap["nodes"] for p in n["pods"]] + list(snap.get("other_listed", ()))
    backed = {group_key(g) for g in snap["groups"] if g["backed_off"]}
    permitted = {group_key(g) for g in snap["groups"] if g["permitted"]}
    by_label = {}
    for p in listed:
        by_label.setdefault(CO.full_name(p), []).append(p)
    cache = {}
    slot_of = {res.names[int(r)]: s for s, r in enumerate(slot_res)}
    verdicts = []
    for g in snap["groups"]:
        if not g.get("exists", True) or g["min_resources"] is None:
            verdicts.append((0, 0, {}))
            continue
        req = CO.min_resources_request(g)
        ok, remaining = CO.check_cluster_resource(snap["nodes"], req, group_key(g))
        cache[group_key(g)] = ok  # PreFilter below asks the same question for every pod of the group
        named = sum(1 << slot_of[k] for k in req)
        open_mask = sum(1 << slot_of[k] for k in remaining)
        # the tables carry a cpu request rounded up to a milli (MilliValue()); against integer sums its gap is the exact gap rounded up
        verdicts.append((named & ~open_mask, open_mask, {slot_of[k]: O._ceil(Fraction(v)) for k, v in remaining.items()}))
    status = [CO.prefilter(p, existing, by_label.get(CO.full_name(p), []), snap["nodes"], backed, permitted, cache) for p in snap["pending"]]
    return np.array(status, np.uint8), verdicts


def closed_form(f, g):
    """the device's arithmetic for group g from the flattened columns, in Python integers: (pass_mask, open_mask, {slot: gap})"""
    present = [i for i in range(f["N"]) if f["node_present"][i]]
    steps = {int(f["step_node"][k]): [int(x) for x in f["step_add"][k]] for k in range(f["step_ptr"][g], f["step_ptr"][g + 1])}
    pass_mask = open_mask = 0
    gaps = {}
    for s in range(f["S"]):
        if not (int(f["req_mask"][g]) >> s) & 1:
            continue
        req, run, best = int(f["req"][g][s]), 0, None
        for i in present:
            run += int(f["left_base"][s][i]) + (steps[i][s] if i in steps else 0)
            best = run if best is None else max(best, run)
        if best is not None and best >= req:
            pass_mask |= 1 << s
        else:
            open_mask |= 1 << s
            gaps[s] = req - run
    return pass_mask, open_mask, gaps


def draw_snapshot(seed, n_nodes, n_groups, n_walk, step_lens=None, pods_per_group=2, first_absent=None, last_absent=None, kinds=range(10), edges=None, n_pending=None):
    """a snapshot over {cpu, memory, pods, one scalar} with over-requested nodes (negative left-overs), absent nodes, nodes without the
    scalar, and groups drawn so that every status occurs.  The first n_walk groups have assigned pods; step_lens[i] = how many nodes
    host group i's pods (default: 1 to 3), group 0's on node 0 and group 1's on the last node when those are present.
    kinds[g % len] picks what group g is about: 1 backed off, 2 too few siblings, 3 gated below quorum, 4 no PodGroup object, 5 MinMember 0,
    6 permitted, 9 no MinResources, anything else plain; edges[g % len] (default: drawn) where its cpu request sits relative to the
    snapshot's largest prefix sum: 0 at it, 1 one above, 2 a third, 3 far above, 4 half, 5 one below."""
    kinds = list(kinds)
    rng = np.random.default_rng(seed)
    nodes = []
    for i in range(n_nodes):
        alloc = {"cpu": f"{int(rng.integers(1, 65)) * 1000}m", "memory": int(rng.integers(1, 513)) << 30, "pods": int(rng.integers(4, 111))}
        if rng.random() < 0.7:
            alloc[SCALAR] = int(rng.integers(0, 9))
        present = bool(rng.random() > 0.1) if n_nodes > 1 else True
        pods = []
        for j in range(int(rng.integers(0, 4))):
            over = 3 if rng.random() < 0.15 else 1  # some nodes are over-requested: allocatable shrank under their pods
            req = {"cpu": f"{int(rng.integers(100, 24000)) * over}m", "memory": int(rng.integers(1, 96) * over) << 30}
            if SCALAR in alloc and rng.random() < 0.3:
                req[SCALAR] = int(rng.integers(1, 4) * over)
            pods.append(make_pod("bg", f"bg-{i}-{j}", requests=req))
        nodes.append({"present": present, "allocatable": alloc, "pods": pods})
    if first_absent is not None:
        nodes[0]["present"] = not first_absent
    if last_absent is not None:
        nodes[-1]["present"] = not last_absent
    present_idx = [i for i, n in enumerate(nodes) if n["present"]]
    if present_idx:  # whatever was drawn, one present node is over-requested for certain
        hog = nodes[present_idx[len(present_idx) // 2]]
        hog["pods"].append(make_pod("bg", "hog", requests={"memory": hog["allocatable"]["memory"] + (1 << 30)}))
    # the prefix sums of the snapshot without anybody's pods removed, only to pick requests near the edge (nothing is checked with them)
    can = lambda k, n: CO.node_resource(n, "nobody/nothing").get(k, 0)
    base_max = {}
    for k in ("cpu", "memory", "pods", SCALAR):
        run, best = 0, None
        for i in present_idx:
            run += can(k, nodes[i])
            best = run if best is None else max(best, run)
        base_max[k] = best if best is not None else 0
    groups, pending, other = [], [], []
    for g in range(n_groups):
        ns, name = f"ns{g % 7}", f"pg{g}"
        kind = kinds[g % len(kinds)]
        if g < n_walk and kind in (4, 9):  # a group with assigned pods takes the walk only if it reaches the resource check
            kind = 0
        members = pods_per_group + int(rng.integers(0, 2))
        hosts = []
        if g < n_walk and present_idx:
            want = step_lens[g] if step_lens and g < len(step_lens) else int(rng.integers(1, 4))
            want = min(want, len(present_idx))
            hosts = sorted(int(x) for x in rng.choice(present_idx, size=want, replace=False))
            if g == 0 and nodes[0]["present"] and 0 not in hosts:
                hosts[0] = 0
            if g == 1 and nodes[-1]["present"] and n_nodes - 1 not in hosts:
                hosts[-1] = n_nodes - 1
            for h in sorted(set(hosts)):
                for j in range(int(rng.integers(1, 3))):
                    req = {"cpu": f"{int(rng.integers(100, 8000))}m", "memory": int(rng.integers(1, 32)) << 30}
                    if rng.random() < 0.5:
                        req[SCALAR] = int(rng.integers(1, 3))  # counted only where the node lists the scalar
                    nodes[h]["pods"].append(make_pod(ns, f"{name}-a{h}-{j}", name, requests=req))
        n_assigned = sum(1 for h in set(hosts) for p in nodes[h]["pods"] if p["labels"].get(LABEL) == name and p["namespace"] == ns)
        listed = members + n_assigned
        min_member, n_gated, backed, permitted, min_res, exists = max(0, listed - int(rng.integers(0, 2))), 0, False, False, None, True
        if kind == 1:
            backed = True
        elif kind == 2:
            min_member = listed + 1 + int(rng.integers(0, 3))
        elif kind == 3:
            n_gated = int(rng.integers(1, 3))
            min_member = listed + n_gated  # with the gated pods listed too: MinMember - listed + gated = gated > 0
        elif kind == 4:
            exists = False
        elif kind == 5:
            min_member = 0
        if kind != 9 and exists:
            edge = int(rng.integers(0, 6)) if edges is None else edges[g % len(edges)]
            cpu_max = base_max["cpu"]
            cpu = {0: cpu_max, 1: cpu_max + 1, 2: max(1, cpu_max // 3), 3: cpu_max * 4 + 7, 4: max(1, cpu_max // 2), 5: cpu_max - 1}[edge]
            min_res = {"cpu": f"{max(cpu, 0)}m"}
            if rng.random() < 0.6:
                min_res["memory"] = max(0, base_max["memory"] // int(rng.integers(1, 4)) + int(rng.integers(-1, 2)))
            if rng.random() < 0.5:
                min_res[SCALAR] = max(0, base_max[SCALAR] // int(rng.integers(1, 3)) + int(rng.integers(-1, 2)))
            permitted = kind == 6
        for j in range(members):
            pending.append(make_pod(ns, f"{name}-p{j}", name))
        for j in range(n_gated):
            other.append(make_pod(ns, f"{name}-g{j}", name, gated=True))
        groups.append(O.pod_group(ns, name, min_member, min_res, created_ns=1000 + g, backed_off=backed, permitted=permitted, exists=exists))
    for n in nodes:
        n.pop("_node_info", None)  # the oracle's per-node cache was filled before the groups' pods moved in
    pending.append(make_pod("ns0", "plain"))  # a pod without the label
    while n_pending is not None and len(pending) < n_pending:
        pending.append(make_pod("ns1", f"plain-{len(pending)}"))
    assert n_pending is None or len(pending) == n_pending
    order = rng.permutation(len(pending))
    return {"nodes": nodes, "groups": groups, "pending": [pending[i] for i in order], "other_listed": other}
