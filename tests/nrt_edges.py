"""Edge-case generators for NodeResourceTopologyMatch's long-row and wide kernels (kernels_nrt_long.hip, kernels_nrt_wide.hip).

synth.nrt_snapshot writes NUMA ids equal to list positions, gives the extra resources to a pod's first app container only and keeps
every quantity far from a zone boundary.  The mutators here edit a seeded snapshot towards what the two kernels distinguish: NUMA ids
that are not positions (permuted, or sparse in 0..63), extra resources in later / init / sidecar containers, zone quantities that are
decided by the charges of the containers before, more non-zero slots than the wide kernel caches, and the container-count limits.

Every knob does two things: a random share of the snapshot is mutated (breadth), and a small hand-shaped case is planted on reserved
nodes and pod rows (build()'s "edges" dict names them) so that the edge decides cells in every example, whatever the seed -
tests/test_nrt_edges_host.py asserts exactly that with the oracle alone, over the example lists the GPU tests draw from.

The generator stays inside the domain where the reference is defined: under LeastNUMANodes the ids stay a permutation of the positions
(subtractFromNUMAs indexes the zone list with the id and panics out of range), no Guaranteed pod has an empty request list, and a Guaranteed container
always names cpu and memory (the API server defaults requests to limits, and a Guaranteed pod has both limits on every container): the
single-entry and all-zero lists are containers of Burstable pods."""
from typing import NamedTuple

import numpy as np

from scheduler_plugins_amd import synth
from scheduler_plugins_amd._abi import Table
from test_gpu_property import _mutate_nrt

GiB, MiB = 1 << 30, 1 << 20
STRATEGIES = ["LeastAllocated", "MostAllocated", "BalancedAllocation", "LeastNUMANodes"]
APP, INIT, SIDECAR = 0, 1, 2
CPU, MEM = 0, 1
WIDE_MAX_CTRS = 64   # SPX_NRT_WIDE_MAX_CTRS
CONTAINER_SCOPE = (3 << 1) | 0  # legacy policy SingleNUMANodeContainerLevel


class Example(NamedTuple):
    route: str        # "long": the dense tables + k_nrt_long; "wide": k_nrt_wide
    seed: int
    strategy: str
    numa_ids: str     # "position" | "permuted" | "sparse"
    spread: bool
    tight_extra: bool
    many_slots: bool
    max_numa: bool
    unit_log2: int
    slots: int        # 4 / 6 (dense tables; on the wide route through SPX_OPT_NRT_WIDE), 9 / 12 / 32 (wide tables)


def _examples(route, n, seed):
    """a fixed list: the strategies in turn, every id mode each strategy allows, the other knobs from a seeded stream"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        strategy = STRATEGIES[i % 4]
        modes = ("permuted", "position", "permuted") if strategy == "LeastNUMANodes" else ("permuted", "sparse", "position", "sparse")
        slots = (4, 6)[(i // 4) % 2] if route == "long" else (9, 12, 32, 6, 4, 12)[(i // 4) % 6]
        out.append(Example(route, int(rng.integers(1, 10_000)), strategy, modes[(i // 4) % len(modes)], bool(rng.random() < 0.7),
                           bool(rng.random() < 0.7), bool(rng.random() < 0.6), bool(rng.random() < 0.5), int(rng.choice([20, 16, 24, 0])), slots))
    return out


EXAMPLES_LONG = _examples("long", 32, 1)
EXAMPLES_WIDE = _examples("wide", 48, 2)


# ------------------------------------------------------------------ object tables <-> editable lists
class _Edit:
    """the pod, zone and node-allocatable lists of a snapshot as Python objects; tables() writes them back"""

    def __init__(self, hdr, snap):
        self.hdr, self.snap = hdr, snap
        p = snap["pods"]
        cptr = p.array("ctr_ptr")
        lists = {}
        for name in ("req", "lim"):
            ptr, res, qty = p.array(f"{name}_ptr"), p.array(f"{name}_res"), p.array(f"{name}_qty")
            lists[name] = [dict(zip(res[ptr[c]:ptr[c + 1]].tolist(), qty[ptr[c]:ptr[c + 1]].tolist())) for c in range(len(ptr) - 1)]
        kind = p.array("ctr_kind")
        self.pods = [[dict(kind=int(kind[c]), req=lists["req"][c], lim=lists["lim"][c]) for c in range(cptr[i], cptr[i + 1])]
                     for i in range(len(cptr) - 1)]
        n = snap["nrt"]
        ptr, res, qty = n.array("zres_ptr"), n.array("zres_res"), n.array("zres_avail")
        self.zones = [dict(zip(res[ptr[z]:ptr[z + 1]].tolist(), qty[ptr[z]:ptr[z + 1]].tolist())) for z in range(len(ptr) - 1)]
        self.zone_ptr = n.array("zone_ptr")
        nd = snap["nodes"]
        ptr, res, qty = nd.array("scalar_ptr"), nd.array("scalar_res"), nd.array("scalar_qty")
        self.scalars = [dict(zip(res[ptr[i]:ptr[i + 1]].tolist(), qty[ptr[i]:ptr[i + 1]].tolist())) for i in range(len(ptr) - 1)]

    def node_zones(self, node):
        return self.zones[self.zone_ptr[node]:self.zone_ptr[node + 1]]

    @staticmethod
    def _csr(lists):
        ptr = np.zeros(len(lists) + 1, np.int32)
        np.cumsum([len(l) for l in lists], out=ptr[1:])
        return (ptr, np.array([k for l in lists for k in l], np.int32), np.array([v for l in lists for v in l.values()], np.int64))

    def tables(self):
        hdr, snap = self.hdr, self.snap
        p = snap["pods"]
        ctrs = [c for pod in self.pods for c in pod]
        cptr = np.zeros(len(self.pods) + 1, np.int32)
        np.cumsum([len(pod) for pod in self.pods], out=cptr[1:])
        rptr, rres, rqty = self._csr([c["req"] for c in ctrs])
        lptr, lres, lqty = self._csr([c["lim"] for c in ctrs])
        keep = ("ovh_ptr", "ovh_res", "ovh_qty", "priority", "queue_ts", "appgroup", "selector", "ns")
        snap["pods"] = Table(hdr, "spx_pod_objects", n_pods=len(self.pods), ctr_ptr=cptr, ctr_kind=np.array([c["kind"] for c in ctrs], np.uint8),
                             req_ptr=rptr, req_res=rres, req_qty=rqty, lim_ptr=lptr, lim_res=lres, lim_qty=lqty, **{f: p.array(f) for f in keep})
        n = snap["nrt"]
        zptr, zres, zavail = self._csr(self.zones)
        keep = ("has_nrt", "fresh", "legacy_policy", "attr_scope", "attr_policy", "attr_max_numa", "zone_ptr", "zone_is_node", "zone_numa_id",
                "zcost_ptr", "zcost_numa_id", "zcost_value", "assumed_ptr", "arl_ptr", "arl_res", "arl_qty")
        snap["nrt"] = Table(hdr, "spx_nrt_objects", n_nodes=int(n.struct.n_nodes), zres_ptr=zptr, zres_res=zres, zres_avail=zavail,
                            **{f: n.array(f) for f in keep})
        nd = snap["nodes"]
        sptr, sres, sqty = self._csr(self.scalars)
        keep = ("alloc_cpu_milli", "alloc_mem", "alloc_eph", "alloc_pods", "cap_cpu_milli", "region", "zone")
        snap["nodes"] = Table(hdr, "spx_node_objects", n_nodes=int(nd.struct.n_nodes), scalar_ptr=sptr, scalar_res=sres, scalar_qty=sqty,
                              **{f: nd.array(f) for f in keep})
        return snap


def pod_qos(pod):
    """v1qos.GetPodQOS over cpu and memory: 0 Guaranteed, 1 Burstable, 2 BestEffort"""
    req, lim, guaranteed = {}, {}, True
    for c in pod:
        for r in (CPU, MEM):
            if c["req"].get(r, 0) > 0:
                req[r] = req.get(r, 0) + c["req"][r]
            if c["lim"].get(r, 0) > 0:
                lim[r] = lim.get(r, 0) + c["lim"][r]
        if not (c["lim"].get(CPU, 0) > 0 and c["lim"].get(MEM, 0) > 0):
            guaranteed = False
    if not req and not lim:
        return 2
    if guaranteed and all(lim.get(r) == q for r, q in req.items()) and len(req) == len(lim):
        return 0
    return 1


def _g(cpu, extra=None, kind=APP, mem=MiB):
    rl = {CPU: cpu, MEM: mem}
    rl.update(extra or {})
    return dict(kind=kind, req=dict(rl), lim=dict(rl))


def unit_of(res):
    """one unit of a spreadable resource: hugepages come in whole pages / GiB, device pools in pieces"""
    if res == synth.RES_HUGEPAGES_2MI:
        return 2 * MiB
    if res == synth.RES_HUGEPAGES_1GI or (res >= synth.RES_EXTRA0 and synth.extra_resource_is_hugepage(res - synth.RES_EXTRA0)):
        return GiB
    return 1


def spreadable(ex):
    """the resources beyond cpu and memory of an example's snapshot, ascending id"""
    if ex.slots > 6:
        return [synth.RES_HUGEPAGES_2MI, synth.RES_DEVICE] + [synth.RES_EXTRA0 + k for k in range(ex.slots - 4)]
    return [synth.RES_HUGEPAGES_2MI, synth.RES_DEVICE] + ([synth.RES_HUGEPAGES_1GI, synth.RES_DEVICE2] if ex.slots == 6 else [])


# ------------------------------------------------------------------ the knobs
def relabel_node(nrt, node, new_ids):
    """zone ids of one node replaced (list order kept); the cost rows name NUMA ids and are relabelled with the same map"""
    ids, ptr = nrt.array("zone_numa_id"), nrt.array("zone_ptr")
    cp, cid = nrt.array("zcost_ptr"), nrt.array("zcost_numa_id")
    a, b = int(ptr[node]), int(ptr[node + 1])
    m = {int(o): int(nw) for o, nw in zip(ids[a:b], new_ids)}
    ids[a:b] = new_ids
    for k in range(cp[a], cp[b]):
        cid[k] = m.get(int(cid[k]), int(cid[k]))


def mutate_numa_ids(nrt, rng, mode, share=0.5):
    ptr = nrt.array("zone_ptr")
    ids = nrt.array("zone_numa_id")
    if mode == "position":
        return
    for i in np.flatnonzero(rng.random(len(ptr) - 1) < share):
        nz = int(ptr[i + 1] - ptr[i])
        if nz == 0:
            continue
        if mode == "permuted":
            relabel_node(nrt, i, ids[ptr[i]:ptr[i + 1]][rng.permutation(nz)].copy())
        else:
            relabel_node(nrt, i, rng.choice(64, nz, replace=False).astype(np.int32))


def mutate_spread(ed, rng, ex, share=0.35):
    """1-6 spreadable resources in several containers of multi-container Guaranteed and Burstable pods"""
    pool = spreadable(ex)
    for pod in ed.pods:
        qos = pod_qos(pod)
        apps = [c for c in pod if c["kind"] == APP]
        if qos == 2 or len(pod) < 2 or not apps or rng.random() >= share:
            continue
        picks = [int(r) for r in rng.choice(pool, min(len(pool), int(rng.integers(1, 7))), replace=False)]

        def give(c, r, units):
            c["req"][r] = c["lim"][r] = units * unit_of(r)
        for r in picks[:2]:  # the same slot in consecutive app containers
            for c in apps[:int(rng.integers(2, 5))]:
                give(c, r, int(rng.integers(0, 3)))
        for r in picks[2:]:  # any container, init and sidecar included
            for c in pod:
                if rng.random() < 0.3:
                    give(c, r, int(rng.integers(0, 3)))
        give(apps[-1], picks[-1], 1)  # (when picks[-1] went nowhere else: a slot that only the last container names)
        if qos == 1 and len(apps) > 2:
            r = picks[0]
            apps[1]["req"], apps[1]["lim"] = {r: unit_of(r)}, {r: unit_of(r)}   # a list of one entry
            apps[2]["req"] = {k: 0 for k in apps[2]["req"]} or {r: 0}            # every quantity zero
            apps[2]["lim"] = dict(apps[2]["req"])


def mutate_many_slots(ed, rng, ex, share=0.15):
    """Guaranteed pods whose containers name 5-10 non-zero slots"""
    pool = spreadable(ex)
    if len(pool) < 3:
        return
    for pod in ed.pods:
        if pod_qos(pod) != 0 or rng.random() >= share:
            continue
        n = int(rng.integers(3, min(len(pool), 8) + 1))
        picks = sorted(int(r) for r in rng.choice(pool, n, replace=False))
        for c in pod:
            if c["kind"] == APP or rng.random() < 0.5:
                for r in picks:
                    c["req"][r] = c["lim"][r] = int(rng.integers(1, 3)) * unit_of(r)


def mutate_tight_extra(ed, rng, ex, share=0.25):
    """zone quantities equal to the requests of the first k app containers of some pod that names the resource, -1 / +0 / +1; under
    LeastNUMANodes also half a container's request (it must span two zones)"""
    half = ex.strategy == "LeastNUMANodes"
    for r in spreadable(ex) + [CPU]:
        users = [[c["req"][r] for c in pod if c["kind"] == APP and c["req"].get(r, 0) > 0] for pod in ed.pods if pod_qos(pod) != 2]
        users = [u for u in users if u]
        if not users:
            continue
        for z in ed.zones:
            if r in z and rng.random() < (share / 2 if r == CPU else share):
                u = users[int(rng.integers(len(users)))]
                if half and rng.random() < 0.3:
                    z[r] = u[0] // 2
                else:
                    z[r] = max(0, sum(u[:int(rng.integers(1, len(u) + 1))]) + int(rng.integers(-1, 2)))


def force_container_counts(hdr, snap, rng, counts):
    """chosen Guaranteed rows with exactly counts[k] containers (synth.lengthen_pods' copy-and-divide rule); -> {count: row}"""
    ed = _Edit(hdr, snap)
    rows = [i for i, pod in enumerate(ed.pods) if pod_qos(pod) == 0 and len(pod) <= 8]
    rows = [int(r) for r in rng.choice(rows, len(counts), replace=False)]
    for row, n in zip(rows, counts):
        snap["pods"] = synth.lengthen_pods(hdr, snap["pods"], rows=[row], seed=row, lo=n, hi=n)
    return dict(zip(counts, rows))


# ------------------------------------------------------------------ planted cases
def _claim_nodes(ed, nrt, k, rng):
    """k container-scope single-numa-node nodes with eight zones, fresh, no assumed pods"""
    ptr, ap = nrt.array("zone_ptr"), nrt.array("assumed_ptr")
    ok = np.flatnonzero((np.diff(ptr) == 8) & (nrt.array("has_nrt") == 1) & (np.diff(ap) == 0))
    nodes = [int(n) for n in rng.choice(ok, k, replace=False)]
    for n in nodes:
        nrt.array("fresh")[n] = 1
        nrt.array("legacy_policy")[n] = CONTAINER_SCOPE
        nrt.array("attr_scope")[n] = -1
        nrt.array("attr_policy")[n] = -1
        for z in ed.node_zones(n):
            z[CPU], z[MEM] = 64000, 64 * GiB
    return nodes


def _report(ed, node, res, qty_of_pos):
    """node lists `res` in its allocatable and every zone reports it, position p with qty_of_pos(p)"""
    if res not in (CPU, MEM):
        ed.scalars[node][res] = 1024 * unit_of(res)
    for p, z in enumerate(ed.node_zones(node)):
        z[res] = qty_of_pos(p)


def _free_rows(ed, taken, k, rng):
    rows = [i for i in range(len(ed.pods)) if i not in taken]
    rows = [int(r) for r in rng.choice(rows, k, replace=False)]
    taken.update(rows)
    return rows


def build(hdr, ex: Example):
    """-> (snapshot dict, edges dict).  edges: the planted nodes and rows and what the oracle must say there"""
    rng = np.random.default_rng(ex.seed)
    n_nodes, n_pods = (130, 50) if ex.strategy == "LeastNUMANodes" else (300 + ex.seed % 83, 200 - ex.seed % 37)
    extra = ex.slots - 4 if ex.slots > 6 else 0
    snap = synth.nrt_snapshot(hdr, n_nodes, n_pods, seed=ex.seed, wide=ex.slots == 6, long_frac=0.06, long_ctrs=(9, 20), extra_res=extra,
                              extra_req_frac=0.3)
    counts = (8, 9, 63, 64) if ex.route == "wide" else (8, 9, 64, 65, 200)
    edges = {"count_rows": force_container_counts(hdr, snap, rng, counts)}
    _mutate_nrt(snap, rng, 0.5, 0.2 if ex.tight_extra else 0.0, False, ex.max_numa, ex.unit_log2)
    nrt = snap["nrt"]
    mutate_numa_ids(nrt, rng, ex.numa_ids)
    ed = _Edit(hdr, snap)
    if ex.spread:
        mutate_spread(ed, rng, ex)
    if ex.many_slots:
        mutate_many_slots(ed, rng, ex)
    if ex.tight_extra:
        mutate_tight_extra(ed, rng, ex)
    taken = set(edges["count_rows"].values())
    pool = spreadable(ex)
    B = pool[-1] if ex.slots > 6 else CPU          # the resource that decides the planted Filter cases: the last slot of a wide table
    S = pool[-1]                                   # ... and of the spread / tight cases: always beyond cpu and memory
    uB, uS = (1000 if B == CPU else unit_of(B)), unit_of(S)
    small = 100                                    # cpu of a planted container when cpu is not the deciding resource
    g1, g2, g3, g6, t_lo, t_eq, t_hi, t_half = _claim_nodes(ed, nrt, 8, rng)

    # --- where a Filter charge goes: the zone with the lowest id holds two containers, every other zone one
    ids = nrt.array("zone_numa_id")
    a = int(nrt.array("zone_ptr")[g1])
    if ex.numa_ids != "position":  # the lowest id away from position 0; sparse: every id >= 8, one >= 32
        new = rng.permutation(8) if ex.numa_ids == "permuted" else rng.choice(np.arange(8, 64), 8, replace=False)
        if ex.numa_ids == "sparse" and not (new >= 32).any():
            new[1] = 40
        if new[0] == new.min():
            new = np.roll(new, 3)
        relabel_node(nrt, g1, new.astype(np.int32))
    low = int(np.argmin(ids[a:a + 8]))
    _report(ed, g1, B, lambda p: 2 * uB if p == low else uB)
    ctr = _g(1000) if B == CPU else _g(small, {B: uB})
    r_fail = next(i for i in rng.permutation(len(ed.pods) - 1) if i not in taken and i + 1 not in taken)
    r_fail, r_pass = int(r_fail), int(r_fail) + 1  # neighbours: a run of long rows for the row-range tests to split
    taken.update((r_fail, r_pass))
    ed.pods[r_fail], ed.pods[r_pass] = [dict(ctr, req=dict(ctr["req"]), lim=dict(ctr["lim"])) for _ in range(10)], \
        [dict(ctr, req=dict(ctr["req"]), lim=dict(ctr["lim"])) for _ in range(9)]
    edges["charge"] = dict(node=g1, fail=r_fail, ok=r_pass, low_pos=low)

    # --- LeastNUMANodes, container scope: subtractFromNUMAs uses the chosen ids as list positions (oracle appendix B.1)
    if ex.strategy == "LeastNUMANodes":
        if ex.numa_ids != "position":
            relabel_node(nrt, g2, np.array([1, 0, 2, 3, 4, 5, 6, 7], np.int32))
        else:
            relabel_node(nrt, g2, np.arange(8, dtype=np.int32))
        _report(ed, g2, CPU, lambda p: (4000, 1000)[p] if p < 2 else 0)
        (r,) = _free_rows(ed, taken, 1, rng)
        ed.pods[r] = [_g(3000), _g(3000)] + [_g(1) for _ in range(8)]
        edges["greedy"] = dict(node=g2, row=r)

    # --- spread: init and sidecar containers name S without being charged, consecutive app containers are, the last one fails
    if ex.spread:
        _report(ed, g3, S, lambda p: 2 * uS if p == 5 else 0)
        r_fail, r_pass = _free_rows(ed, taken, 2, rng)
        head = [_g(small, {S: 2 * uS}, INIT), _g(small, {S: uS}, SIDECAR), _g(small), _g(small, {S: uS}), _g(small, {S: uS})]
        ed.pods[r_fail] = head + [_g(small) for _ in range(5)] + [_g(small, {S: uS})]
        ed.pods[r_pass] = head + [_g(small) for _ in range(5)] + [_g(small)]
        (r_b,) = _free_rows(ed, taken, 1, rng)  # Burstable: a list of one entry, a list of zeros, among containers without limits
        burst = lambda rl: dict(kind=APP, req=dict(rl), lim={})
        ed.pods[r_b] = [burst({CPU: small, MEM: MiB}), dict(kind=APP, req={S: uS}, lim={S: uS}), burst({CPU: 0, MEM: 0, S: 0}),
                        dict(kind=APP, req={S: 2 * uS}, lim={S: 2 * uS})] + [burst({CPU: small}) for _ in range(6)]
        edges["spread"] = dict(node=g3, fail=r_fail, ok=r_pass, burstable=r_b)

    # --- many_slots: every spreadable resource (up to eight) next to cpu and memory, the last one alone needs two zones
    if ex.many_slots and len(pool) >= 3:
        named = pool[-8:]
        for r in named[:-1]:
            _report(ed, g6, r, lambda p: 64 * unit_of(r))
        _report(ed, g6, named[-1], lambda p: unit_of(named[-1]))
        r_all, r_four = _free_rows(ed, taken, 2, rng)
        big = {r: unit_of(r) for r in named[:-1]}
        big[named[-1]] = 2 * unit_of(named[-1])
        first4 = dict(list(sorted(big.items()))[:2])   # with cpu and memory: the first four non-zero slots
        ed.pods[r_all] = [_g(small, big)] + [_g(small) for _ in range(8)]
        ed.pods[r_four] = [_g(small, first4)] + [_g(small) for _ in range(8)]
        edges["many"] = dict(node=g6, all=r_all, four=r_four, n_slots=2 + len(big))

    # --- tight_extra: one pod, three nodes of one shape: the zone holds what the pod's app containers ask for -1 / +0 / +1
    if ex.tight_extra:
        (r,) = _free_rows(ed, taken, 1, rng)
        ed.pods[r] = [_g(small, {S: (1 + i % 2) * uS}) for i in range(9)]
        total = sum(c["req"][S] for c in ed.pods[r])
        for node, d in ((t_lo, -1), (t_eq, 0), (t_hi, 1)):
            _report(ed, node, S, lambda p: total + d if p == 3 else 0)
        edges["tight"] = dict(row=r, lo=t_lo, eq=t_eq, hi=t_hi)
        if ex.strategy == "LeastNUMANodes":  # half a request in each of two zones: both emptied exactly by the first container
            relabel_node(nrt, t_half, np.arange(8, dtype=np.int32))
            _report(ed, t_half, S, lambda p: uS if p in (2, 6) else 0)
            (r,) = _free_rows(ed, taken, 1, rng)
            ed.pods[r] = [_g(small, {S: 2 * uS}), _g(small, {S: uS})] + [_g(small) for _ in range(7)]
            edges["half"] = dict(node=t_half, row=r)
    ed.tables()
    edges["rows"] = sorted(taken)
    return snap, edges


NRT_FIELDS = ("has_nrt", "fresh", "legacy_policy", "attr_scope", "attr_policy", "attr_max_numa", "zone_ptr", "zone_is_node", "zone_numa_id",
              "zres_ptr", "zres_res", "zres_avail", "zcost_ptr", "zcost_numa_id", "zcost_value", "assumed_ptr", "arl_ptr", "arl_res", "arl_qty")


def ids_reset_to_positions(hdr, nrt):
    """a copy of the NRT objects with every node's NUMA ids equal to the list positions again (cost rows relabelled)"""
    out = Table(hdr, "spx_nrt_objects", n_nodes=int(nrt.struct.n_nodes), **{f: nrt.array(f).copy() for f in NRT_FIELDS})
    ptr = out.array("zone_ptr")
    for i in range(len(ptr) - 1):
        if ptr[i + 1] > ptr[i]:
            relabel_node(out, i, np.arange(ptr[i + 1] - ptr[i], dtype=np.int32))
    return out


def edge_rows(snap, ex):
    """the rows the two kernels are there for: more than eight containers, or a request beyond cpu and memory"""
    p = snap["pods"]
    n_ctr = np.diff(p.array("ctr_ptr"))
    names = np.zeros(len(n_ctr), bool)
    res, rptr, cptr = p.array("req_res"), p.array("req_ptr"), p.array("ctr_ptr")
    for i in range(len(n_ctr)):
        names[i] = (res[rptr[cptr[i]]:rptr[cptr[i + 1]]] > MEM).any()
    return np.flatnonzero((n_ctr > 8) | names)
