"""Hand-built snapshots whose nodes of at most eight NUMA zones list one NUMA id twice or more ("twins") — for
tests/test_nrt_dense_twins_host.py (the oracle alone, and two plain Python readings of the Go source, show each example holds its edge)
and tests/test_gpu_nrt_dense_twins.py (k_nrt, k_nrt_long and k_nrt_wide against the oracle, cell by cell).

subtractResourcesFromNUMANodeList (numaresources.go:145-182) charges a container to every zone that carries the id it was given.  With
even twins the node holds one container per distinct id.  With uneven twins the container fits the larger one, the smaller one goes
below zero, and the Filter ends with fwk.Error "inconsistent resource accounting" (filter.go:73-77): status 255 (SPX_NRT_ST_ERROR).

The builders are tests/nrt_tall_cases.py's (tall_nrt, g, burstable, case, build work for any zone count).  Every example is small — at
most 70 nodes and 40 pod rows — and decided by its edge, not by its size."""
from scheduler_plugins_amd import objects as O

import nrt_tall_cases as TC
from nrt_tall_cases import CONTAINER, DEV, HP, NONE, POD, besteffort, burstable, case, g, tall_nrt
from nrt_tall_edge_cases import ids_ends, ids_paired, shared_ln_pod_case

ERROR = 255
ZONE_COUNTS = [2, 3, 4, 5, 8]


# ------------------------------------------------------------------ NUMA ids by list position
def ids_lo_hi(n):
    """twins of the lowest id at positions 3 and 4: one sits in the packed ids' low word, the other in the high word (n >= 5)"""
    return [1, 2, 3, 0, 0, 4, 5, 6][:n]


def ids_one(n):
    """every zone carries one id"""
    return [0] * n


def ids_high(n):
    """twins of an id that is not the lowest: 0 1 1 2 3 ... (n >= 3)"""
    return [0, 1, 1] + list(range(2, n - 1))


def ids_sparse(n):
    """sparse twins: 63 63 5 40 ... (not for LeastNUMANodes, whose container scope takes ids as list positions)"""
    return ([63, 63] + [5, 40, 17, 9, 33, 21])[:n]


def ids_sparse_free(n):
    return ([63, 62] + [5, 40, 17, 9, 33, 21])[:n]


def patterns(n, sparse):
    """the distinct shared-id patterns of a zone count, by name; `sparse`: with the ones that hold ids from the zone count up"""
    out = {}
    for name, pat in (("paired", ids_paired), ("ends", ids_ends), ("one", ids_one)) + ((("lo-hi", ids_lo_hi),) if n >= 5 else ()) + \
            ((("sparse", ids_sparse),) if sparse else ()):
        if pat(n) not in out.values():
            out[name] = pat(n)
    return out


def twin_positions(ids):
    """positions of the zones that carry the lowest id that occurs more than once"""
    t = min(i for i in ids if ids.count(i) > 1)
    return [p for p, i in enumerate(ids) if i == t]


def is_twin_node(t):
    ids = [O.numa_name_to_id(z["name"]) for z in t["zones"]]
    return len(set(ids)) < len(ids)


# ------------------------------------------------------------------ even twins
def even_case(n, sparse=False):
    """one core per zone; a row of k one-core containers for k = 1 .. n.  A node holds one container per distinct id: ceil(n/2) for
    paired ids, n - 1 where the two ends share one (or the twins sit at positions 3 and 4, or an id above the lowest is shared), one
    where every zone carries the same id, n on the duplicate-free twin (the last node).  c["ids"]: the id list of each node"""
    pats = dict(patterns(n, sparse))
    if n >= 3:
        pats["high"] = ids_high(n)
    pats["free"] = list(range(n))
    if sparse:
        pats["sparse-free"] = ids_sparse_free(n)
    c = case([tall_nrt(ids, ["1"] * n) for ids in pats.values()], [O.pod([g("1")] * k) for k in range(1, n + 1)])
    c["ids"], c["names"] = list(pats.values()), list(pats)
    return c


# ------------------------------------------------------------------ uneven twins
# what the first carrier of the twin id holds ("big") and what every other carrier holds ("small"), per kind of node
KINDS = {
    "cpu-1m": (("2", "4Gi", {}), ("1999m", "4Gi", {})),                   # short by exactly one millicore
    "memory": (("2", "4Gi", {}), ("2", "32Mi", {})),                      # uneven in memory only
    "device": (("4", "4Gi", {DEV: "2"}), ("4", "4Gi", {DEV: "1"})),       # uneven in a device only
}
QUIET_KINDS = {
    "to-zero": (("3", "4Gi", {}), ("2", "4Gi", {})),                      # the smaller twin ends at exactly 0
    "unreported": (("4", "4Gi", {DEV: "2"}), ("4", "4Gi", {})),           # the smaller twin does not report the device: skipped
}
OTHER = ("0", "4Gi", {})         # a zone that is no twin: no Guaranteed container of these examples fits it, whatever its id
ROOMY = ("8", "8Gi", {DEV: "4"})


def uneven_nrt(ids, kind, policy=CONTAINER, other=OTHER, twins=None):
    big, small = {**KINDS, **QUIET_KINDS}[kind]
    tw = twin_positions(ids) if twins is None else twins
    spec = [(big if p == tw[0] else small) if p in tw else other for p in range(len(ids))]
    extras = [dict(s[2], **{HP: "1Gi"}) for s in spec]
    return tall_nrt(ids, [s[0] for s in spec], [s[1] for s in spec], extras, policy)


def reader(i):
    """a row that passes on the table as uploaded and on no table an Error row's charge is left on: one core, 16 MiB and one device
    of what the smaller twin holds (1 999 m, 32 MiB, one device).  `i` keeps the readers of an example apart, so that no two of them
    form one class of pods and every one is evaluated where it stands"""
    return O.pod([g("1", f"{16 * 1024 + i}Ki", {DEV: "1"})])


def closing_row(k):
    """k - 1 containers of 1 m and 256 KiB, then one that takes what the larger twin has left of cpu — one millicore more than the
    smaller one has — one KiB more memory than the smaller one has left, and two devices: the k-th container raises the Error"""
    return O.pod([g("1m", "256Ki")] * (k - 1) + [g(f"{2001 - k}m", f"{32 * 1024 - 256 * (k - 1) + 1}Ki", {DEV: "2"})])


def error_rows(longest=65):
    """(name, pod, {kind: status}) in row order; a reader follows every row that is an Error anywhere.  Devices: the zones of the
    cpu-1m and memory nodes report none, so a device request is host-level there and skipped.  longest: the containers of the longest
    row (65: a long row of the dense tables; 64: the most a wide snapshot takes)"""
    E, C = ERROR, TC.ST["container"]
    tiny = g("1m", "1Mi")
    rows = [
        ("one", O.pod([g("2", "64Mi", {DEV: "2"})]), {"cpu-1m": E, "memory": E, "device": E}),
        ("later-device", O.pod([g("1"), g("1", "64Mi", {DEV: "2"})]), {"cpu-1m": E, "memory": E, "device": E}),
        ("burstable-device", O.pod([burstable(1, "64Mi", {DEV: "2"})]), {"cpu-1m": 0, "memory": 0, "device": E}),
        ("eighth", O.pod([tiny] * 7 + [g("1993m", "26Mi", {DEV: "2"})]), {"cpu-1m": E, "memory": E, "device": E}),
        ("ninth", O.pod([tiny] * 8 + [g("1992m", "25Mi", {DEV: "2"})]), {"cpu-1m": E, "memory": E, "device": E}),
        ("longest", closing_row(longest), {"cpu-1m": E, "memory": E, "device": E}),
        ("error-then-unfit", O.pod([g("2", "64Mi", {DEV: "2"}), g("5")]), {"cpu-1m": E, "memory": E, "device": E}),
        ("besteffort-device", O.pod([besteffort({DEV: "2"})]), {"cpu-1m": 0, "memory": 0, "device": E}),
    ]
    out = []
    for i, r in enumerate(rows):
        out += [r, (f"reader-{i}", reader(i), {"cpu-1m": 0, "memory": 0, "device": 0})]
    out += [
        ("init-first", O.pod([g("2")], [g("100")]), dict.fromkeys(KINDS, TC.ST["init"])),
        ("sidecar-first", O.pod([g("2")], [dict(g("100"), sidecar=True)]), dict.fromkeys(KINDS, TC.ST["sidecar"])),
        ("unfit-then-error", O.pod([g("5"), g("2", "64Mi", {DEV: "2"})]), dict.fromkeys(KINDS, C)),
        ("seven-tiny", O.pod([tiny] * 7), dict.fromkeys(KINDS, 0)),
    ]
    return out


def uneven_case(n, sparse=False, longest=65):
    """every shared-id pattern of the zone count x every kind of uneven twins, in container scope (the nodes the Error is planted on);
    then the same in pod scope (never an Error), the duplicate-free twin of each kind, a stale node and one whose policy is not
    single-NUMA.  c["plan"][node] = (pattern name, kind, what): what in "twin", "pod-scope", "free", "stale", "not-single";
    c["want"][row] = {kind: status} on the "twin" nodes"""
    pats = patterns(n, sparse)
    nrts, plan, fresh = [], [], []
    for what, policy in (("twin", CONTAINER), ("pod-scope", POD)):
        for name, ids in pats.items():
            for kind in KINDS:
                nrts.append(uneven_nrt(ids, kind, policy)), plan.append((name, kind, what)), fresh.append(True)
    first = next(iter(pats.values()))
    for kind in KINDS:
        nrts.append(uneven_nrt(list(range(n)), kind, twins=twin_positions(first))), plan.append(("free", kind, "free")), fresh.append(True)
    nrts.append(uneven_nrt(first, "cpu-1m")), plan.append(("paired", "cpu-1m", "stale")), fresh.append(False)
    nrts.append(uneven_nrt(first, "cpu-1m", NONE)), plan.append(("paired", "cpu-1m", "not-single")), fresh.append(True)
    rows = error_rows(longest)
    c = case(nrts, [r[1] for r in rows], fresh)
    c["plan"], c["rows"], c["want"] = plan, [r[0] for r in rows], [r[2] for r in rows]
    return c


def quiet_case(n):
    """uneven twins that never raise the Error: the smaller twin ends at exactly 0, or does not report the device (it is skipped); twins
    of an id above the lowest next to a roomy zone with the lowest id (never charged); Burstable pods whose cpu, memory and hugepages
    would go below zero (affine resources are not subtracted); BestEffort pods without a non-native request.  Every cell passes, except
    the row whose second container finds no room"""
    ids = ids_paired(n)
    nrts = [uneven_nrt(ids, k) for k in QUIET_KINDS]
    plan = [("paired", k, "twin") for k in QUIET_KINDS]
    if n >= 3:
        nrts += [uneven_nrt(ids_high(n), k, other=ROOMY) for k in KINDS]
        plan += [("high", k, "twin") for k in KINDS]
    pods =[O.pod([g("2", "64Mi", {DEV: "2"})]), reader(0), O.pod([g("1"), g("1", "16Mi", {DEV: "1"})]), reader(1),
            O.pod([burstable(3, "8Gi", {HP: "2Gi"})]), O.pod([burstable("2500m", "5Gi"), burstable("2500m", "5Gi", {HP: "1Gi"})]),
            O.pod([besteffort()]), O.pod([g("2", "64Mi", {DEV: "1"}), g("2", "64Mi", {DEV: "1"})])]
    c = case(nrts, pods)
    c["plan"] = plan
    return c


def mixed_case(n_nodes=70, twin_col=37):
    """one uneven twin node (4 zones, paired ids, short by a millicore) among position-id nodes of the same sizes: the column the
    rank-space and fused Filter launches must not be run on"""
    ids = ids_paired(4)
    tw = twin_positions(ids)
    nrts = [uneven_nrt(ids if i == twin_col else list(range(4)), "cpu-1m", twins=tw) for i in range(n_nodes)]
    rows = error_rows()
    c = case(nrts, [r[1] for r in rows if r[0] not in ("ninth", "longest")])
    c["twin_col"] = twin_col
    return c


def with_slots(c, n_slots):
    """the case with n_slots resource slots instead of its own (the names its zones report or its containers request): every zone and
    every node reports further devices that no pod asks for"""
    names = {k for t in c["nrts"] if t is not None for z in t["zones"] for k in z["resources"]}
    names |= {k for p in c["pods"] for ctr in p["containers"] + p["init_containers"] for k in ctr["requests"]}
    more = {f"example.com/pool{i}": "4" for i in range(n_slots - len(names))}
    nrts = [None if t is None else dict(t, zones=[dict(z, resources=dict(z["resources"], **more)) for z in t["zones"]]) for t in c["nrts"]]
    nodes = [dict(nd, allocatable=dict(nd["allocatable"], **more), capacity=dict(nd["capacity"], **more)) for nd in c["nodes"]]
    return dict(c, nrts=nrts, nodes=nodes)


def ln_case(n, policy=POD):
    """tests/nrt_tall_edge_cases.py's LeastNUMANodes example on nodes of at most eight zones: the count is of distinct ids, and in
    container scope the greedy subtraction takes the chosen ids as list positions (every id stays below the zone count)"""
    return shared_ln_pod_case(n, policy)


# ------------------------------------------------------------------ every example, by name: (builder, strategies)
def examples():
    out = {}
    for n in ZONE_COUNTS:
        out[f"even-{n}"] = (lambda n=n: even_case(n), TC.STRATEGIES)
        out[f"even-sparse-{n}"] = (lambda n=n: even_case(n, sparse=True), TC.NOT_LEAST_NUMA)
        out[f"uneven-{n}"] = (lambda n=n: uneven_case(n), TC.STRATEGIES)
        out[f"uneven-sparse-{n}"] = (lambda n=n: uneven_case(n, sparse=True), TC.NOT_LEAST_NUMA)
        out[f"quiet-{n}"] = (lambda n=n: quiet_case(n), TC.STRATEGIES)
        if n >= 4:
            out[f"least-numa-{n}"] = (lambda n=n: ln_case(n), ["LeastNUMANodes"])
            out[f"least-numa-container-{n}"] = (lambda n=n: ln_case(n, CONTAINER), ["LeastNUMANodes"])
    out["mixed"] = (mixed_case, TC.STRATEGIES)
    return out


# ------------------------------------------------------------------ a seeded full profile with twins, for what reads the status table
def twin_profile(hdr, n_nodes=130, n_pods=60, seed=7, share=0.5):
    """synth.full_snapshot with paired ids (0 0 1 1 ...) on about `share` of its nodes: their zone quantities are drawn
    independently, so the twins are uneven and the Error occurs by itself.  -> (snapshot, the relabelled nodes)"""
    import numpy as np

    from nrt_edges import relabel_node
    from scheduler_plugins_amd import synth
    snap = synth.full_snapshot(hdr, n_nodes, n_pods, seed=seed)
    snap["nrt_params"] = O.nrt_params(hdr, O.Resources(), "LeastAllocated")
    nrt = snap["nrt"]
    ptr, ids = nrt.array("zone_ptr"), nrt.array("zone_numa_id")
    twins = []
    for i in np.flatnonzero(np.random.default_rng(seed).random(len(ptr) - 1) < share):
        nz = int(ptr[i + 1] - ptr[i])
        if nz >= 2:
            relabel_node(nrt, i, (np.arange(nz) // 2).astype(ids.dtype))
            twins.append(int(i))
    return snap, twins
