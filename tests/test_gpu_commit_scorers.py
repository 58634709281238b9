"""spx_commit_sequential with LowRiskOverCommitment and Peaks in the mask.

Method of test_gpu_commit.py::test_commit_sequential_full_profile: after every decision the test applies the bookkeeping to its
Python-side state — for LowRiskOverCommitment the bound pod joins its node's pod list (nodeInfo.GetPods() of the next cycle) —
rebuilds the object tables and lets the CPU oracle evaluate the next pod's row from scratch.  Both scorers are +-1 plugins, so the
check has two halves:
  cells     the row each pod saw (the score tables after the call): LROC's and Peaks' bytes within +-1 of the oracle's row on every
            feasible node, every other plugin's bytes and every status exactly equal;
  decision  node, weighted score, tie count and the unschedulable verdict equal the numpy argmax over the fetched bytes (the
            engine's own rows with the oracle's feasibility and weights, lowest index among ties), exactly.
The Python state follows the engine's decision, so one +-1 cell cannot derail the rest of the batch.

Peaks rows of a pod that requests no cpu are rounding noise of two nearly equal exp() values stretched over 0..100 (inherited from
the reference, tests/test_gpu_peaks.py's docstring): their cells are not compared with the oracle; the decision half still holds."""
import ctypes as C

import numpy as np
import pytest

import scheduler_plugins_amd as spx
from helpers import ALLOCATABLE, CAPACITY, LROC, LVRB, NETOVERHEAD, NRT, PEAKS, TLP, lroc_params, lvrb_params, tlp_params
from scheduler_plugins_amd import objects as O
from scheduler_plugins_amd import synth
from scheduler_plugins_amd.engine import Engine, mask_of

WINDOW_END = 1_700_000_000
SYSCHED = 9
MI = 1 << 20


# ------------------------------------------------------------------ the form selection, on the CPU
def test_lroc_commit_form_bounds():
    """(largest node column) + (sum of the batch's pod column) per column selects the form: below 2^47 with no limit below its
    request float32 (1), below 2^52 float64 (2), otherwise int64 (0)"""
    fn = spx.lib().spx_internal_lroc_commit_form
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64, C.c_int32]

    def form(node_max, pod_sum, alloc_max=0, cover=1):
        a, b = (C.c_int64 * 4)(*node_max), (C.c_int64 * 4)(*pod_sum)
        return fn(a, b, alloc_max, cover)

    z = [0, 0, 0, 0]
    assert form(z, z) == 1
    assert form([1 << 46] * 4, [(1 << 46) - 1] * 4) == 1            # 2^47 - 1
    for c in range(4):                                              # each column on its own reaches 2^47: float64
        nm, ps = list(z), list(z)
        nm[c], ps[c] = (1 << 47) - 5, 5
        assert form(nm, ps) == 2, c
        nm[c], ps[c] = (1 << 47) - 5, 4
        assert form(nm, ps) == 1, c
        nm[c], ps[c] = (1 << 52) - 1, 0
        assert form(nm, ps) == 2, c
        nm[c], ps[c] = (1 << 51), (1 << 51)                         # 2^52: int64
        assert form(nm, ps) == 0, c
    assert form(z, z, cover=0) == 2                                 # a limit below its request: no float32 form
    assert form(z, z, alloc_max=1 << 47) == 2 and form(z, z, alloc_max=1 << 52) == 0 and form(z, z, alloc_max=1 << 53) == 0
    big = (1 << 63) - 1
    assert form([big] * 4, [big] * 4) == 0                          # the bound itself does not wrap
    assert form([-1, 0, 0, 0], z) == 0


# ------------------------------------------------------------------ trimaran-only masks
def _scenario(n_nodes, n_pods, seed, big_mem=False):
    """Small nodes and pods whose limits are a multiple of their requests: over the batch some node's summed limits cross its
    capacity and some node's summed requests reach it (asserted by the test on its own state).  A tenth of the nodes has no
    metrics; pod 1 requests nothing, pod 2's manifest has limits below its requests (the flattener raises them)."""
    rng = np.random.default_rng(seed)
    small = n_nodes <= 30
    nodes, metrics, on = [], {}, {}
    for i in range(n_nodes):
        cpu = int(rng.choice([2, 4] if small else [4, 8, 16]))
        mem = int(rng.choice([4, 8] if small else [16, 32])) << 30
        if big_mem and i == n_nodes - 1:
            mem = 1 << 53
        nodes.append(O.node({"cpu": f"{cpu}", "memory": mem}))
        if rng.random() < 0.9:
            metrics[i] = [("CPU", "AVG", float(rng.integers(5, 60))), ("CPU", "STD", float(rng.integers(0, 15))),
                          ("Memory", "AVG", float(rng.integers(5, 70))), ("Memory", "STD", float(rng.integers(0, 15)))]
        if rng.random() < 0.5:   # pods already running: requests at 40-70 % of the node, limits just below its capacity
            rq = int(cpu * 1000 * rng.uniform(0.4, 0.7))
            on[i] = [O.pod([O.container({"cpu": f"{rq}m", "memory": mem // 4}, {"cpu": f"{cpu * 1000 - 200}m", "memory": mem - 100 * MI})])]
    pods = []
    for i in range(n_pods):
        cpu = int(rng.choice([250, 500, 1000]))
        mem = int(rng.choice([128, 512, 1024])) * MI
        k = float(rng.choice([1.0, 2.0, 4.0]))
        req = {"cpu": f"{cpu}m", "memory": mem}
        lim = None if rng.random() < 0.3 else {"cpu": f"{int(cpu * k)}m", "memory": int(mem * k)}
        pods.append(O.pod([O.container(req, lim)]))
    if n_pods > 2:
        pods[1] = O.pod([O.container()])
        pods[2] = O.pod([O.container({"cpu": "800m", "memory": 900 * MI}, {"cpu": "300m", "memory": 100 * MI})])
    return nodes, metrics, pods, on


def _argmax(total, feasible):
    if not feasible.any():
        return -1, 0, 0
    best = int(total[feasible].max())
    ties = np.flatnonzero(feasible & (total == best))
    return int(ties[0]), best, int(ties.size)


def _cells_close(plugin, got, want, feasible, i):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))[feasible]
    assert d.size == 0 or d.max() <= 1, (plugin, i, int(d.max()))


def _run_trimaran(hdr, oracle, plugins, weights, n_nodes, n_pods, seed, form="graph", lroc="float32", check_crossing=False):
    nodes, metrics, pods, on0 = _scenario(n_nodes, n_pods, seed, big_mem=(lroc == "int64"))
    res = O.Resources()
    node_t, pod_t, rc = O.build_node_objects(hdr, res, nodes), O.build_pod_objects(hdr, res, pods), res.table(hdr)
    met_t = O.build_metrics_objects(hdr, n_nodes, metrics, window_end=WINDOW_END)
    pm = synth.synth_power_models(hdr, n_nodes, seed)
    mask = mask_of(*plugins)
    with Engine(0) as e:
        if form == "plain":
            e.set_option("COMMIT_FROM_MEMORY", 1)
        if form == "reference":
            e.force_reference_kernels(TLP, LVRB, LROC)
        if lroc == "float64":
            e.set_option("LROC_FLOAT64", 1)
        e.load_trimaran_objects(node_t, rc, pod_t, met_t, O.build_assigned_objects(hdr, res, n_nodes, {}))
        e.set_lroc()
        e.load_lroc_objects(node_t, O.build_node_pods_objects(hdr, res, n_nodes, on0), pod_t)
        e.load_peaks_objects(node_t, met_t, pm, pod_t)
        e.set_plugin_weights(weights)
        scorers = [p for p in (LROC, PEAKS) if p in plugins]
        before = {}
        for p in scorers:   # the frozen-snapshot tables before the loop
            e.eval(mask_of(p))
            e.sync()
            before[p] = e.all_scores(p).copy()
        got_node, got_score, got_ties, got_missing = e.commit_sequential(mask)
        assert e.commit_path() == 2
        if LROC in plugins:
            assert e.kernel_path(LROC) == (1 if lroc == "float32" and form != "reference" else 0)
        rows = {p: e.all_scores(p).copy() for p in plugins}
        again = e.commit_sequential(mask)   # a second call: the snapshot was restored, identical outputs
        for a, b in zip((got_node, got_score, got_ties, got_missing), again):
            assert np.array_equal(a, b)
        for p in scorers:   # and the frozen-snapshot tables are byte-identical
            e.eval(mask_of(p))
            e.sync()
            assert np.array_equal(e.all_scores(p), before[p]), p
        alloc_params = e.alloc_params
        cpu_real = e.peaks_soa["cpu_milli"] > 0
        alloc = e.flatten_trimaran_nodes(node_t, met_t, None)
        cap = {"cpu": alloc["lv_alloc_cpu_milli"], "mem": alloc["lv_alloc_mem"]}
        on = {n: list(v) for n, v in on0.items()}
        bound = {}
        feasible = np.ones(n_nodes, bool)
        crossed, capped, lroc_seen = set(), set(), {}
        for i in range(n_pods):
            np_t = O.build_node_pods_objects(hdr, res, n_nodes, on)
            osnap = oracle.Snapshot(node_t, pod_t, rc=rc, metrics=met_t, assigned=O.build_assigned_objects(hdr, res, n_nodes, bound),
                                    alloc_params=alloc_params, tlp_params=tlp_params(hdr), lvrb_params=lvrb_params(hdr), node_pods=np_t,
                                    lroc_params=lroc_params(hdr), power_models=pm)
            total = np.zeros(n_nodes, np.int64)
            for p in plugins:
                raw, norm = osnap.score_rows(p, i, i + 1, want_norm=(p in (ALLOCATABLE, PEAKS)))
                want = (norm if p in (ALLOCATABLE, PEAKS) else raw)[0].clip(0, 255)
                if p == LROC:
                    _cells_close(p, rows[p][i], want, feasible, i)
                    lroc_seen[i] = want
                elif p == PEAKS:
                    if cpu_real[i]:
                        _cells_close(p, rows[p][i], want, feasible, i)
                else:
                    assert np.array_equal(rows[p][i], want), (p, i)
                total += weights[p] * rows[p][i].astype(np.int64)
            assert (got_node[i], got_score[i], got_ties[i]) == _argmax(total, feasible), (i, got_node[i], got_score[i], got_ties[i])
            n = int(got_node[i])
            if check_crossing:
                c0 = e.flatten_lroc_nodes(node_t, np_t)
            on.setdefault(n, []).append(pods[i])
            bound.setdefault(n, []).append((WINDOW_END + 1, pods[i]))
            if check_crossing:
                c1 = e.flatten_lroc_nodes(node_t, O.build_node_pods_objects(hdr, res, n_nodes, on))
                for r, lim, req in (("cpu", "lim_cpu_milli", "req_cpu_milli"), ("mem", "lim_mem", "req_mem")):
                    if c0[lim][n] <= cap[r][n] < c1[lim][n]:
                        crossed.add((n, i))   # `over` went from <= 0 to > 0 on this node with this commit
                    if c1[req][n] >= cap[r][n]:
                        capped.add(n)         # the summed requests reach the setMin cap (resourcestats.go:208-211)
                assert all(np.array_equal(c0[k][np.arange(n_nodes) != n], c1[k][np.arange(n_nodes) != n]) for k in c0)
    assert len(set(got_node.tolist())) > 1
    if check_crossing:
        assert crossed and capped, (crossed, capped)
        # ... and the oracle's rows show it: on some such node the best score seen after the crossing is below the best one before
        real = [i for i in range(n_pods) if lroc_seen[i].any()]
        moved = [n for n, i in crossed if [j for j in real if j <= i] and [j for j in real if j > i] and
                 max(lroc_seen[j][n] for j in real if j > i) < max(lroc_seen[j][n] for j in real if j <= i)]
        assert moved, crossed
    return got_node


W2 = {TLP: 2, LROC: 3}
W5 = {ALLOCATABLE: 1, TLP: 2, LVRB: 1, LROC: 3, PEAKS: 2}
SHAPES = [(5, 40, 1), (23, 60, 2), (70, 60, 3), (300, 40, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["graph", "plain"])
@pytest.mark.parametrize("n_nodes,n_pods,seed", SHAPES)
@pytest.mark.parametrize("plugins,weights", [((TLP, LROC), W2), ((ALLOCATABLE, TLP, LVRB, LROC, PEAKS), W5)], ids=["tlp-lroc", "trimaran5"])
def test_commit_trimaran_masks(gpu_required, hdr, oracle, plugins, weights, n_nodes, n_pods, seed, form):
    """5 x 40: most nodes win several times, so later pods see re-prepared Beta fits and grown sums; 23 nodes: less than a wave;
    70: a partial second wave; 300: more nodes than a workgroup of the commit kernels has dword slots per step (not 1024 x 4: the
    loops' tails).  The two small shapes must cross a capacity with the summed limits and reach the cap with the summed requests."""
    got = _run_trimaran(hdr, oracle, plugins, weights, n_nodes, n_pods, seed, form=form, check_crossing=(n_nodes <= 23))
    if n_nodes == 5:
        assert (np.bincount(got[got >= 0], minlength=5) >= 2).sum() >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes,n_pods,seed", SHAPES[:2])
def test_commit_trimaran_masks_reference_kernels(gpu_required, hdr, oracle, n_nodes, n_pods, seed):
    _run_trimaran(hdr, oracle, (ALLOCATABLE, TLP, LVRB, LROC, PEAKS), W5, n_nodes, n_pods, seed, form="reference")


@pytest.mark.gpu
@pytest.mark.parametrize("lroc", ["float32", "float64", "int64"])
def test_commit_lroc_three_forms(gpu_required, hdr, oracle, lroc):
    """the batch's form: float32 by default, float64 with SPX_OPT_LROC_FLOAT64, int64 forced by one memory column at 2^53"""
    _run_trimaran(hdr, oracle, (TLP, LROC), W2, 70, 40, 7, lroc=lroc)


@pytest.mark.gpu
def test_commit_scorers_errors(gpu_required, hdr):
    snap = synth.trimaran_snapshot(hdr, 10, 5)
    with Engine(0) as e:
        e.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])
        with pytest.raises(Exception, match=r"supports Peaks only with its node and pod tables uploaded \(spx_upload_peaks_nodes / spx_upload_peaks_pods\)"):
            e.commit_sequential(mask_of(TLP, PEAKS))
        with pytest.raises(Exception, match=r"supports LowRiskOverCommitment only with its node and pod tables uploaded"):
            e.commit_sequential(mask_of(TLP, LROC))
        with pytest.raises(Exception, match=r"supports Allocatable / TargetLoadPacking / LoadVariationRiskBalancing / NodeResourceTopologyMatch / NetworkOverhead / CapacityScheduling"):
            e.commit_sequential(mask_of(TLP, SYSCHED))


# ------------------------------------------------------------------ the full profile plus LROC and Peaks
@pytest.mark.gpu
@pytest.mark.parametrize("form,n_nodes,n_pods,seed", [(f, *sh) for f in ("graph", "plain") for sh in SHAPES] + [("reference", *sh) for sh in SHAPES[:2]])
def test_commit_full_profile_with_scorers(gpu_required, hdr, oracle, form, n_nodes, n_pods, seed):
    """test_gpu_commit.py's full scenario (NRT + NetworkOverhead + CapacityScheduling + Allocatable + TLP + LVRB) with LROC and Peaks:
    Peaks is normalised per pod over the pod's feasible nodes, LROC sees the pods bound before.  A pod that binds nowhere leaves
    the state as it was (the next pod's oracle rows are built from the unchanged Python state)."""
    from test_gpu_commit import GROUPS, REGION_COSTS, ZONE_COSTS, _full_scenario
    nrts, nodes, node_labels, pods, meta, metrics, quotas, nominated = _full_scenario(hdr, n_nodes, n_pods, seed)
    res = O.Resources()
    res.id("vendor.io/gpu")
    regions, zones = O.Interner(), O.Interner()
    nt_t = O.build_nettopo_objects(hdr, regions, zones, REGION_COSTS, ZONE_COSTS)
    for i, (rg, zn) in enumerate(node_labels):
        nodes[i]["region"], nodes[i]["zone"] = regions.id(rg), zones.id(zn)
    sel = O.Interner(["a", "b", "c", "d"])
    sel.freeze_sorted()
    pod_dicts = [O.pod(p["containers"], priority=p["priority"], queue_ts=p["queue_ts"], ns=p["ns"], appgroup=g, selector=sel.id(s))
                 for p, (g, s) in zip(pods, meta)]
    node_t, pod_t, rc = O.build_node_objects(hdr, res, nodes), O.build_pod_objects(hdr, res, pod_dicts), res.table(hdr)
    met_t = O.build_metrics_objects(hdr, n_nodes, metrics, window_end=WINDOW_END)
    pm = synth.synth_power_models(hdr, n_nodes, seed)
    params = O.nrt_params(hdr, res, "LeastAllocated")
    names = {f"n{i}": i for i in range(n_nodes)}

    def tables(assumed, placed, used, nom):
        nrt_t = O.build_nrt_objects(hdr, res, nrts, assumed=assumed)
        ag_t = O.build_appgroup_objects(hdr, sel, [dict(g, placed=[(s, f"n{n}") for s, n in placed[gi]]) for gi, g in enumerate(GROUPS)], names)
        q = [None if qq is None else dict(qq, used=used[k]) for k, qq in enumerate(quotas)]
        quota_t = O.build_quota_objects(hdr, res, q, nominated=[(pods[j]["ns"], pods[j]["priority"], j, pod_dicts[j]) for j in nom])
        return nrt_t, ag_t, quota_t

    used0 = [None if q is None else q["used"] for q in quotas]
    nrt_t, ag_t, quota_t = tables({}, [[], []], used0, nominated)
    weights = {ALLOCATABLE: 1, TLP: 2, LVRB: 1, NRT: 3, NETOVERHEAD: 2, LROC: 3, PEAKS: 2}
    plugins = (ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD, CAPACITY, LROC, PEAKS)
    with Engine(0) as e:
        if form == "reference":
            e.force_reference_kernels(TLP, LVRB, NRT, NETOVERHEAD, LROC)
        if form == "plain":
            e.set_option("COMMIT_FROM_MEMORY", 1)
        e.load_trimaran_objects(node_t, rc, pod_t, met_t, O.build_assigned_objects(hdr, res, n_nodes, {}))
        e.load_nrt_objects(node_t, nrt_t, rc, pod_t, params)
        e.load_network_objects(node_t, pod_t, ag_t, nt_t)
        e.load_quota_objects(pod_t, rc, quota_t)
        e.set_lroc()
        e.load_lroc_objects(node_t, O.build_node_pods_objects(hdr, res, n_nodes, {}), pod_t)
        e.load_peaks_objects(node_t, met_t, pm, pod_t)
        e.set_plugin_weights(weights)
        before = {}
        for p in (LROC, PEAKS):
            e.eval(mask_of(p))
            e.sync()
            before[p] = e.all_scores(p).copy()
        got_node, got_score, got_ties, _ = e.commit_sequential(mask_of(*plugins))
        assert e.commit_path() == 2   # the cooperative kernel declines a mask with either scorer
        rows = {p: e.all_scores(p).copy() for p in (TLP, LVRB, NRT, NETOVERHEAD, LROC, PEAKS)}
        status = {p: e.all_status(p).copy() for p in (NRT, NETOVERHEAD)}
        again = e.commit_sequential(mask_of(*plugins))
        assert np.array_equal(again[0], got_node) and np.array_equal(again[1], got_score) and np.array_equal(again[2], got_ties)
        for p in (LROC, PEAKS):
            e.eval(mask_of(p))
            e.sync()
            assert np.array_equal(e.all_scores(p), before[p]), p
        alloc_params = e.alloc_params
        cpu_real = e.peaks_soa["cpu_milli"] > 0
        pod_req = e.nrt_soa["pods"]["pod_req"].reshape(n_pods, -1)
        pod_present = e.nrt_soa["pods"]["pod_present"]
        slot_res = e.nrt_soa["slots"].array("slot_res")
        qcols = e.flatten_quota(pod_t, rc, quota_t)["cols"]
    res_name = {v: k for k, v in res.ids.items()}
    scalar_names = [res_name[int(r)] for r in quota_t.array("scalar_res")[: quota_t.struct.n_scalar_slots]]

    def effective_request(i):  # GetPodEffectiveRequest as a resource list (the reserve store's entry)
        rl = {}
        for s in range(pod_req.shape[1]):
            if (pod_present[i] >> s) & 1:
                name = res_name[int(slot_res[s])]
                rl[name] = f"{int(pod_req[i, s])}m" if name == "cpu" else int(pod_req[i, s])
        return rl

    def add_used(u, i):  # reserveResource elasticquota.go:89-98, on framework.Resource fields
        v = qcols["pod_req"][i * 8:(i + 1) * 8]
        base, _ = O._resource_vec(res, [res.ids[n] for n in scalar_names], u)
        out = {"MilliCPU": base[0] + int(v[0]), "Memory": base[1] + int(v[1]), "EphemeralStorage": base[2] + int(v[2]), "AllowedPodNumber": base[3] + int(v[3]),
               "ScalarResources": {}}
        keys = dict((u or {}).get("ScalarResources", {})) if u and "ScalarResources" in u else {k: None for k in (u or {}) if O.is_scalar_resource_name(k)}
        for si, name in enumerate(scalar_names):
            if name in keys or (qcols["pod_req_present"][i] >> (4 + si)) & 1:
                out["ScalarResources"][name] = base[4 + si] + int(v[4 + si])
        return out

    assumed, placed, used, nom, bound, on = {}, [[], []], list(used0), list(nominated), {}, {}
    n_unsched = 0
    for i in range(n_pods):
        nrt_i, ag_i, quota_i = tables(assumed, placed, used, nom)
        osnap = oracle.Snapshot(node_t, pod_t, rc=rc, metrics=met_t, assigned=O.build_assigned_objects(hdr, res, n_nodes, bound), alloc_params=alloc_params,
                                tlp_params=tlp_params(hdr), lvrb_params=lvrb_params(hdr), nrt=nrt_i, nrt_params=params, appgroups=ag_i, nettopo=nt_t,
                                node_pods=O.build_node_pods_objects(hdr, res, n_nodes, on), lroc_params=lroc_params(hdr), power_models=pm)
        pre = oracle.lib().orc_capacity_prefilter(pod_t.ref(), rc.ref(), quota_i.ref(), i)
        nrt_st = osnap.filter_rows(NRT, i, i + 1)[0]
        net_st = osnap.filter_rows(NETOVERHEAD, i, i + 1)[0]
        feasible = (nrt_st == 0) & (net_st == 0)
        if pre != 0:   # PreFilter rejection: no sweep's row is defined for this pod
            assert got_node[i] == -1 and got_ties[i] == 0, (i, pre, got_node[i])
            n_unsched += 1
            continue
        assert np.array_equal(status[NRT][i], nrt_st), i
        assert np.array_equal(status[NETOVERHEAD][i][nrt_st == 0], net_st[nrt_st == 0]), i
        full = lambda m: np.concatenate([np.zeros((i, n_nodes), np.uint8), m[None, :].astype(np.uint8)])
        total = np.zeros(n_nodes, np.int64)
        for p in (TLP, LVRB, NRT):
            want = osnap.score_rows(p, i, i + 1, want_norm=False)[0][0].clip(0, 255)
            cmp = feasible if p == NRT else np.ones(n_nodes, bool)   # (upstream scores only nodes that passed Filter)
            assert np.array_equal(rows[p][i][cmp], want[cmp]), (p, i)
            total += weights[p] * rows[p][i].astype(np.int64)
        want = osnap.score_rows(NETOVERHEAD, i, i + 1, mask=full(nrt_st == 0), want_raw=False)[1][0]
        assert np.array_equal(rows[NETOVERHEAD][i][feasible], want[feasible]), i
        total += weights[NETOVERHEAD] * rows[NETOVERHEAD][i].astype(np.int64)
        # Allocatable's byte is not kept with Filter plugins in the mask (folded into the argmax kernel): the oracle's
        total += weights[ALLOCATABLE] * osnap.score_rows(ALLOCATABLE, i, i + 1, mask=full(feasible), want_raw=False)[1][0]
        _cells_close(LROC, rows[LROC][i], osnap.score_rows(LROC, i, i + 1, want_norm=False)[0][0].clip(0, 255), feasible, i)
        total += weights[LROC] * rows[LROC][i].astype(np.int64)
        if cpu_real[i]:
            _cells_close(PEAKS, rows[PEAKS][i], osnap.score_rows(PEAKS, i, i + 1, mask=full(feasible), want_raw=False)[1][0], feasible, i)
        assert not rows[PEAKS][i][~feasible].any(), i   # infeasible cells are 0, as the table sweep writes them
        total += weights[PEAKS] * rows[PEAKS][i].astype(np.int64)
        node, best, ties = _argmax(total, feasible)
        if node < 0:
            assert got_node[i] == -1 and got_ties[i] == 0, (i, got_node[i])
            n_unsched += 1
            continue
        assert (got_node[i], got_score[i], got_ties[i]) == (node, best, ties), (i, got_node[i], got_score[i], got_ties[i], node, best, ties)
        n = int(got_node[i])
        if nrts[n] is not None:
            assumed.setdefault(n, []).append(effective_request(i))
        g, s = meta[i]
        if g >= 0:
            placed[g].append((s, n))
        k = pods[i]["ns"]
        if quotas[k] is not None:
            used[k] = add_used(used[k], i)
        nom = [j for j in nom if j != i]
        bound.setdefault(n, []).append((WINDOW_END + 1, pod_dicts[i]))
        on.setdefault(n, []).append(pod_dicts[i])
    assert 0 < n_unsched < n_pods and len(set(got_node.tolist())) > 2
