"""Engine-lifetime differential tests: one long-lived engine driven the way a scheduler drives it — new node or pod tables, node
deltas, parameter and strategy changes, option flips, row ranges, feasibility masks, the commit loop — held after every evaluation
to (a) byte equality with a freshly built engine given the same final state and options and (b) where the state is a whole object
snapshot, the CPU oracle with each plugin's stated tolerance.

The engine keeps derived device tables across calls (trimaran's ambiguity tables, LowRiskOverCommitment's per-node table, the NRT
packed-Score table, window sort, LeastNUMANodes tables and the fused walk's packed items, pod classes), each guarded by a flag every
writer clears.  A stale table does not crash: it returns plausible bytes.  The results depend on state and options only, never on
history — that is what the fresh engine checks, byte for byte, where the oracle's +-1 tolerance of LROC / Peaks would let a stale
table through."""
import time

import numpy as np
import pytest

from helpers import ALLOCATABLE, CAPACITY, LROC, LVRB, NETOVERHEAD, NRT, PEAKS, TLP, lroc_params, lvrb_params, tlp_params
from scheduler_plugins_amd import objects as O
from scheduler_plugins_amd import synth
from scheduler_plugins_amd.engine import Engine, mask_of

pytestmark = pytest.mark.gpu

FILTERS = (NRT, NETOVERHEAD)
RAW = (ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD, PEAKS)  # (spx_fetch_raw has no LROC row)
STRATEGIES = ("LeastAllocated", "MostAllocated", "BalancedAllocation", "LeastNUMANodes")
BIG_CPU_MILLI = ((1 << 24) + 1) * 1000  # a zone cpu capacity whose Value() (cores) float32 does not hold exactly


# ------------------------------------------------------------------ the model of the engine's inputs
class Model:
    """What the engine was told, as final state: options, parameters, flat tables (after deltas), the caller's feasibility mask.
    fresh() builds a new Engine(0) from it; `snap` is the object snapshot while the state is a whole one (None after deltas)."""

    def __init__(self, hdr):
        self.hdr = hdr
        self.options = {}
        self.alloc = ("Least", None)
        self.tlp_target = 40
        self.lvrb = (1.0, 1.0)
        self.lroc = (5, 0.5, 0.5)
        self.weights = {}
        self.tables = {}
        self.nrt_params = None
        self.placed = []
        self.ext = None
        self.snap = None

    def set_option(self, e, name, value):
        e.set_option(name, value)
        self.options[name] = value

    def apply_params(self, e):
        e.set_allocatable(*self.alloc)
        e.set_tlp(self.tlp_target)
        e.set_lvrb(*self.lvrb)
        e.set_lroc(*self.lroc)
        e.set_plugin_weights(self.weights)

    def fresh(self) -> Engine:
        f = Engine(0)
        for k, v in self.options.items():
            f.set_option(k, v)
        self.apply_params(f)
        t = self.tables
        if "alloc" in t:
            f.upload_alloc_nodes(t["alloc"])
        if "tri_nodes" in t:
            f.upload_trimaran_nodes(t["tri_nodes"])
            f.upload_trimaran_pods(t["tri_pods"])
        if "lroc_nodes" in t:
            f.upload_lroc_nodes(t["lroc_nodes"])
            f.upload_lroc_pods(t["lroc_pods"])
        if "peaks" in t:
            f.upload_peaks(t["peaks"])
        if "nrt" in t:
            f.upload_nrt(dict(t["nrt"], params=self.nrt_params))
        if "net" in t:
            f.upload_network(t["net"])
            for ent in self.placed:
                f.update_net_placed(ent)
        if "quota" in t:
            f.upload_quota(t["quota"])
        if self.ext is not None:
            f.upload_feasible_mask(self.ext)
        return f


def flatten_all(e, snap, nrt_params, families):
    """the flat tables of `snap` for the listed families (what fresh() uploads)"""
    t = {}
    if "tri" in families:
        t["alloc"] = e.flatten_alloc_nodes(snap["nodes"], snap["rc"])
        t["tri_nodes"] = e.flatten_trimaran_nodes(snap["nodes"], snap["metrics"], snap["assigned"])
        t["tri_pods"] = e.flatten_trimaran_pods(snap["pods"])
    if "lroc" in families:
        t["lroc_nodes"] = e.flatten_lroc_nodes(snap["nodes"], snap["node_pods"])
        t["lroc_pods"] = e.flatten_lroc_pods(snap["pods"])
    if "peaks" in families:
        t["peaks"] = e.flatten_peaks(snap["nodes"], snap["metrics"], snap["power_models"], snap["pods"])
    if "nrt" in families:
        t["nrt"] = e.flatten_nrt(snap["nodes"], snap["nrt"], snap["rc"], snap["pods"], nrt_params)
    if "net" in families:
        t["net"] = e.flatten_network(snap["nodes"], snap["pods"], snap["appgroups"], snap["nettopo"])
    if "quota" in families:
        t["quota"] = e.flatten_quota(snap["pods"], snap.get("quota_rc", snap["rc"]), snap["quota"])
    return t


def upload_all(e, m):
    """the long-lived engine's full upload of the model's tables (the Python loaders)"""
    t = m.tables
    if "alloc" in t:
        e.upload_alloc_nodes(t["alloc"])
        e.upload_trimaran_nodes(t["tri_nodes"])
        e.upload_trimaran_pods(t["tri_pods"])
    if "lroc_nodes" in t:
        e.upload_lroc_nodes(t["lroc_nodes"])
        e.upload_lroc_pods(t["lroc_pods"])
    if "peaks" in t:
        e.upload_peaks(t["peaks"])
    if "nrt" in t:
        e.upload_nrt(dict(t["nrt"], params=m.nrt_params))
    if "net" in t:
        e.upload_network(t["net"])
    if "quota" in t:
        e.upload_quota(t["quota"])


def plugins_of(mask):
    return [p for p in range(9) if (mask >> p) & 1]


def run(e, how, mask, b, end):
    if how == "eval_best":  # (the argmax over the tables an evaluation just wrote)
        e.eval(mask, b, end)
    {"eval": e.eval, "eval_best": e.eval_best, "decide": e.decide}[how](mask, b, end)
    e.sync()


def check_fresh(e, m, mask, b=0, end=None, how="eval", ctx=""):
    """e has just run `how`(mask, b, end): a fresh engine built from the model must hold the same bytes"""
    end = e.n_pods if end is None else end
    with m.fresh() as f:
        run(f, how, mask, b, end)
        if how != "eval":
            for x, y in zip(e.best(b, end), f.best(b, end)):
                assert np.array_equal(x, y), ("best", ctx)
            return
        for p in plugins_of(mask):
            if p == CAPACITY:
                assert np.array_equal(e.prefilter(CAPACITY, b, end), f.prefilter(CAPACITY, b, end)), ("prefilter", ctx)
                continue
            if p in FILTERS:
                assert np.array_equal(e.all_status(p, b, end), f.all_status(p, b, end)), ("status", p, ctx)
            got, want = e.all_scores(p, b, end), f.all_scores(p, b, end)
            bad = np.argwhere(got != want)
            assert bad.size == 0, ("scores", p, ctx, len(bad), [(int(r) + b, int(c), int(got[r, c]), int(want[r, c])) for r, c in bad[:5]])
            if p in RAW:
                for r in (b, end - 1):
                    assert np.array_equal(e.raw(p, r), f.raw(p, r)), ("raw", p, r, ctx)


def check_oracle(e, m, oracle, mask, rows, ctx=""):
    """the whole-snapshot state against the CPU oracle on sampled rows (tolerances as the plugins' own tests)"""
    s, hdr = m.snap, m.hdr
    alloc_tab = e.alloc_params
    osnap = oracle.Snapshot(s["nodes"], s["pods"], rc=s["rc"], metrics=s.get("metrics"), assigned=s.get("assigned"), alloc_params=alloc_tab,
                            tlp_params=tlp_params(hdr, m.tlp_target), lvrb_params=lvrb_params(hdr, *m.lvrb), nrt=s.get("nrt"),
                            nrt_params=m.nrt_params, node_pods=s.get("node_pods"), lroc_params=lroc_params(hdr, *m.lroc),
                            power_models=s.get("power_models"))
    for r in rows:
        for p in plugins_of(mask):
            if p in (TLP, LVRB):
                raw, norm = osnap.score_rows(p, r, r + 1)
                assert np.array_equal(e.all_scores(p, r, r + 1)[0].astype(np.int64), norm[0].clip(0, 255)), (p, r, ctx)
                assert np.array_equal(e.raw(p, r), raw[0]), (p, r, ctx)
            elif p == ALLOCATABLE and not (mask & mask_of(NRT, NETOVERHEAD)) and m.ext is None:
                _, norm = osnap.score_rows(p, r, r + 1)
                assert np.array_equal(e.all_scores(p, r, r + 1)[0].astype(np.int64), norm[0]), (p, r, ctx)
            elif p == NRT:
                assert np.array_equal(e.all_status(NRT, r, r + 1)[0], osnap.filter_rows(NRT, r, r + 1)[0]), (p, r, ctx)
                want, _ = osnap.score_rows(NRT, r, r + 1, want_norm=False)
                assert np.array_equal(e.all_scores(NRT, r, r + 1)[0].astype(np.int64), want[0].clip(0, 255)), (p, r, ctx)
            elif p == LROC:
                _, norm = osnap.score_rows(LROC, r, r + 1)
                assert np.abs(e.all_scores(LROC, r, r + 1)[0].astype(np.int64) - norm[0]).max() <= 1, (p, r, ctx)
            elif p == PEAKS and not (mask & mask_of(NRT, NETOVERHEAD)) and m.ext is None and e.peaks_soa["cpu_milli"][r] > 0:
                _, norm = osnap.score_rows(PEAKS, r, r + 1)
                assert np.abs(e.all_scores(PEAKS, r, r + 1)[0].astype(np.int64) - norm[0]).max() <= 1, (p, r, ctx)


# ------------------------------------------------------------------ snapshots
def nrt_snap(hdr, n_nodes, n_pods, seed, wide=False, big_cpu=False, permute=False, cost_over_255=False):
    s = synth.nrt_snapshot(hdr, n_nodes, n_pods, seed=seed, wide=wide)
    nrt = s["nrt"]
    if big_cpu:  # one zone's cpu of every 50th node: BalancedAllocation's float32 walk declines
        res, avail, zp = nrt.array("zone_ptr"), nrt.array("zres_avail"), nrt.array("zres_ptr")
        rr = nrt.array("zres_res")
        for i in range(0, n_nodes, 50):
            if res[i + 1] > res[i]:
                z = res[i]
                for k in range(zp[z], zp[z + 1]):
                    if rr[k] == 0:
                        avail[k] = BIG_CPU_MILLI
    if permute:  # NUMA ids that are not list positions (the generic kernel); the costs relabelled with them
        ids, ptr = nrt.array("zone_numa_id"), nrt.array("zone_ptr")
        cp, cid = nrt.array("zcost_ptr"), nrt.array("zcost_numa_id")
        for i in range(0, n_nodes, 3):
            a, b = ptr[i], ptr[i + 1]
            if b - a > 1:
                old = ids[a:b].copy()
                new = old[::-1].copy()
                ids[a:b] = new
                relabel = {int(o): int(n) for o, n in zip(old, new)}
                for zc in range(a, b):
                    for k in range(cp[zc], cp[zc + 1]):
                        cid[k] = relabel.get(int(cid[k]), int(cid[k]))
    if cost_over_255:  # no LeastNUMANodes tables
        cv = nrt.array("zcost_value")
        cv[cv > 10] = 300
    return s


def full_snap(hdr, n_nodes, n_pods, seed, flavour="regular"):
    s = synth.full_snapshot(hdr, n_nodes, n_pods, seed=seed, pods_per_group=50, n_namespaces=20)
    s["metrics"] = synth.synth_metrics(hdr, n_nodes, seed, round_frac=1.0 if flavour == "ties" else 0.1)
    s["node_pods"] = synth.synth_node_pods(hdr, n_nodes, seed)
    s["power_models"] = synth.synth_power_models(hdr, n_nodes, seed)
    if flavour in ("big_cpu", "permute", "cost_over_255", "wide"):
        extra = nrt_snap(hdr, n_nodes, n_pods, seed, wide=flavour == "wide", big_cpu=flavour == "big_cpu", permute=flavour == "permute",
                         cost_over_255=flavour == "cost_over_255")
        s["nrt"] = extra["nrt"]
        if flavour == "wide":  # the six-slot batch needs its own node scalars, pods and classes
            s["quota_rc"] = s["rc"]  # (the quota's slots hold the four-slot classes: spx_load_quota is not used with this flavour)
            s["nodes"], s["rc"] = extra["nodes"], extra["rc"]
            s["pods"] = synth.synth_pods(hdr, n_pods, seed, device_res=synth.RES_DEVICE, hugepage_res=synth.RES_HUGEPAGES_2MI,
                                         device2_res=synth.RES_DEVICE2, hugepage2_res=synth.RES_HUGEPAGES_1GI,
                                         n_appgroups=max(1, n_pods // 50), n_namespaces=20)
            s["appgroups"], s["nettopo"] = synth.synth_network(hdr, s["nodes"], max(1, n_pods // 50), seed)
            s["quota"] = synth.synth_quota(hdr, s["pods"], seed, n_namespaces=20, device_res=synth.RES_DEVICE, hugepage_res=synth.RES_HUGEPAGES_2MI)
    if flavour == "lroc_lim_below_req":  # a node table whose pods' limits sit below their requests: the float32 sweep steps aside
        running = s["node_pods"].array("pods")
        lq, lr = running.array("lim_qty"), running.array("lim_res")
        cpu = np.flatnonzero(lr == 0)
        assert cpu.size > 0
        lq[cpu] = 1
    if flavour == "peaks_negative":
        q, r = s["pods"].array("req_qty"), s["pods"].array("req_res")
        cpu = np.flatnonzero(r == 0)
        q[cpu[:3]] = -500
    if flavour in ("dups", "unique"):
        n_groups = max(1, n_pods // 50)
        pool = synth.synth_pods(hdr, 8 * n_pods, seed, device_res=synth.RES_DEVICE, hugepage_res=synth.RES_HUGEPAGES_2MI, n_appgroups=n_groups,
                                n_namespaces=20)
        s["pods"] = batch(hdr, pool, n_pods, flavour, seed)
        s["appgroups"], s["nettopo"] = synth.synth_network(hdr, s["nodes"], n_groups, seed)
        s["quota"] = synth.synth_quota(hdr, s["pods"], seed, n_namespaces=20, device_res=synth.RES_DEVICE, hugepage_res=synth.RES_HUGEPAGES_2MI)
    return s


def batch(hdr, pods, n_pods, kind, seed):
    """a pod batch of n_pods rows drawn from `pods`: "dups" = copies of eight templates (both plugins' pod classes on), "unique" =
    Guaranteed pods with pairwise different NRT records and container cpu requests (both off)"""
    rng = np.random.default_rng(seed + 77)
    if kind == "dups":
        return synth.take_pods(hdr, pods, rng.integers(0, 8, n_pods))
    q, r, ptr = pods.array("req_qty"), pods.array("req_res"), pods.array("req_ptr")
    cptr = pods.array("ctr_ptr")
    lq, lr, lptr = pods.array("lim_qty"), pods.array("lim_res"), pods.array("lim_ptr")
    seen, pick = set(), []
    for i in range(pods.struct.n_pods):
        key = []
        ok = True
        for c in range(cptr[i], cptr[i + 1]):
            req = {int(r[k]): int(q[k]) for k in range(ptr[c], ptr[c + 1])}
            lim = {int(lr[k]): int(lq[k]) for k in range(lptr[c], lptr[c + 1])}
            if 0 not in req or 1 not in req or req.get(0) != lim.get(0) or req.get(1) != lim.get(1):
                ok = False
            key.append(tuple(sorted(req.items())))
        cpu = sum(int(q[k]) for c in range(cptr[i], cptr[i + 1]) for k in range(ptr[c], ptr[c + 1]) if r[k] == 0)
        if ok and cpu not in seen:
            seen.add(cpu)
            pick.append(i)
        if len(pick) == n_pods:
            break
    assert len(pick) == n_pods, len(pick)
    return synth.take_pods(hdr, pods, np.array(pick))


def nrt_params(hdr, strategy):
    return O.nrt_params(hdr, O.Resources(), strategy)


# ------------------------------------------------------------------ 1. fused walk declined, then eligible (nrt_fz_key)
def test_balanced_fused_walk_declined_then_eligible(gpu_required, hdr, oracle):
    """BalancedAllocation's one-launch walk declines while a zone cpu capacity is not exact in float32 (the pack does not run
    either); after a node-only re-upload with exact capacities the next sweep is fused and must pack the items it walks"""
    n_nodes, n_pods = 700, 400
    big = nrt_snap(hdr, n_nodes, n_pods, seed=51, big_cpu=True)
    exact = nrt_snap(hdr, n_nodes, n_pods, seed=51)
    params = nrt_params(hdr, "BalancedAllocation")
    m = Model(hdr)
    m.nrt_params = params
    with Engine(0) as e:
        m.tables = flatten_all(e, big, params, ("nrt",))
        m.snap = big
        upload_all(e, m)
        e.eval(mask_of(NRT))
        e.sync()
        assert e.nrt_filter_path() == 2  # the rank-space Filter + the two-launch Score: the walk declined
        check_fresh(e, m, mask_of(NRT), ctx="declined")
        check_oracle(e, m, oracle, mask_of(NRT), range(0, n_pods, 23), ctx="declined")
        f_exact = e.flatten_nrt(exact["nodes"], exact["nrt"], exact["rc"], exact["pods"], params)
        e.upload_nrt_nodes(f_exact["nodes"], f_exact["R"])
        m.tables["nrt"] = dict(m.tables["nrt"], nodes=f_exact["nodes"])
        m.snap = exact
        e.eval(mask_of(NRT))
        e.sync()
        assert e.nrt_filter_path() == 3
        check_fresh(e, m, mask_of(NRT), ctx="eligible")
        check_oracle(e, m, oracle, mask_of(NRT), list(range(0, n_pods, 7)) + [n_pods - 1], ctx="eligible")


# ------------------------------------------------------------------ 2. the preemption dry run: node-only re-uploads
@pytest.mark.parametrize("kernel", ["fast", "reference"])
def test_preemption_dry_run_node_reuploads(gpu_required, hdr, oracle, kernel):
    n_nodes, n_pods = 600, 300
    snap = nrt_snap(hdr, n_nodes, n_pods, seed=61)
    rng = np.random.default_rng(61)
    with Engine(0) as e:
        m = Model(hdr)
        if kernel == "reference":
            m.set_option(e, "REFERENCE_KERNELS", mask_of(NRT))
        for si, strategy in enumerate(STRATEGIES):
            m.nrt_params = nrt_params(hdr, strategy)
            f = e.flatten_nrt(snap["nodes"], snap["nrt"], snap["rc"], snap["pods"], m.nrt_params)
            m.tables = {"nrt": f}
            upload_all(e, m)
            nodes = f["nodes"]
            for step in range(3):
                # availabilities raised on a few candidate nodes, as spx_nrt_post_eviction raises them
                nodes = {k: v.copy() for k, v in nodes.items()}
                av = nodes["zone_avail"].reshape(n_nodes, 8, f["R"])
                cand = rng.choice(n_nodes, 40, replace=False)
                av[cand] += rng.integers(0, 4, (40, 8, f["R"])) * np.where(av[cand] > 0, av[cand] // 4, 0)
                e.upload_nrt_nodes(nodes, f["R"])
                m.tables["nrt"] = dict(f, nodes=nodes)
                e.eval(mask_of(NRT))
                e.sync()
                assert e.kernel_path(NRT) == (1 if kernel == "fast" else 0)
                check_fresh(e, m, mask_of(NRT), ctx=(strategy, step))
            if strategy != "LeastNUMANodes":  # the state is the snapshot again: its own tables back, oracle on sampled rows
                e.upload_nrt_nodes(f["nodes"], f["R"])
                m.tables["nrt"] = f
                m.snap = snap
                e.eval(mask_of(NRT))
                e.sync()
                check_oracle(e, m, oracle, mask_of(NRT), range(si, n_pods, 37), ctx=strategy)
                m.snap = None


# ------------------------------------------------------------------ 3. strategy switch through spx_set_nrt_params alone
@pytest.mark.parametrize("wide", [False, True], ids=["4slots", "6slots"])
def test_strategy_switch_without_reupload(gpu_required, hdr, oracle, wide):
    n_nodes, n_pods = 700, 400
    snap = nrt_snap(hdr, n_nodes, n_pods, seed=71, wide=wide)
    small = nrt_snap(hdr, 130, 50, seed=72, wide=wide)  # LeastNUMANodes against the oracle at its size
    with Engine(0) as e, Engine(0) as s:
        m, ms = Model(hdr), Model(hdr)
        m.nrt_params = ms.nrt_params = nrt_params(hdr, "LeastAllocated")
        m.tables = flatten_all(e, snap, m.nrt_params, ("nrt",))
        ms.tables = flatten_all(s, small, ms.nrt_params, ("nrt",))
        m.snap, ms.snap = snap, small
        upload_all(e, m), upload_all(s, ms)
        paths = set()
        slots = set()
        for strategy in STRATEGIES + ("BalancedAllocation", "LeastAllocated", "LeastNUMANodes", "MostAllocated", "LeastAllocated"):
            m.nrt_params = ms.nrt_params = nrt_params(hdr, strategy)
            e.set_nrt_params(m.nrt_params)
            s.set_nrt_params(ms.nrt_params)
            e.eval(mask_of(NRT))
            s.eval(mask_of(NRT))
            e.sync(), s.sync()
            paths.add((strategy, e.nrt_filter_path()))
            slots.add(e.nrt_packed_score_slots())
            check_fresh(e, m, mask_of(NRT), ctx=strategy)
            check_fresh(s, ms, mask_of(NRT), ctx=("small", strategy))
            if strategy == "LeastNUMANodes":
                check_oracle(s, ms, oracle, mask_of(NRT), range(0, 50, 3), ctx=strategy)
            else:
                check_oracle(e, m, oracle, mask_of(NRT), range(0, n_pods, 41), ctx=strategy)
        assert ("BalancedAllocation", 3) in paths
        assert len(slots) >= 2  # the packed Score's table slot changed between evaluations


# ------------------------------------------------------------------ 4. pod batches across the class thresholds
def test_pod_batches_cross_the_class_thresholds(gpu_required, hdr, oracle):
    n_nodes, n_pods = 640, 320
    base = full_snap(hdr, n_nodes, n_pods, seed=81)
    many = synth.synth_pods(hdr, 8 * n_pods, 81, device_res=synth.RES_DEVICE, hugepage_res=synth.RES_HUGEPAGES_2MI)
    params = nrt_params(hdr, "LeastAllocated")
    with Engine(0) as e:
        m = Model(hdr)
        m.nrt_params = params
        m.tables = flatten_all(e, base, params, ("nrt", "peaks"))
        upload_all(e, m)
        seen = []
        for kind in ("dups", "unique", "dups", "unique"):
            snap = dict(base, pods=batch(hdr, many, n_pods, kind, 81))
            t = flatten_all(e, snap, params, ("nrt", "peaks"))
            e.upload_nrt_pods(t["nrt"]["pods"], t["nrt"]["R"])
            e.upload_peaks(t["peaks"])
            m.tables["nrt"] = dict(m.tables["nrt"], pods=t["nrt"]["pods"])
            m.tables["peaks"] = t["peaks"]
            m.snap = snap
            nu, nd = e.nrt_pod_classes()
            pu, pd = e.peaks_pod_classes()
            assert nu + nd == n_pods and pu + pd == n_pods
            if kind == "dups":
                assert nd * 32 >= n_pods and pd * 8 >= n_pods
            else:
                assert nd * 32 < n_pods and pd * 8 < n_pods  # below both thresholds: the sweeps walk every row
            seen.append((nd, pd))
            for mask in (mask_of(NRT), mask_of(PEAKS)):
                e.eval(mask)
                e.sync()
                check_fresh(e, m, mask, ctx=(kind, mask))
                check_oracle(e, m, oracle, mask, range(0, n_pods, 29), ctx=(kind, mask))
        assert seen[0] == seen[2] and seen[1] == seen[3]


# ------------------------------------------------------------------ 5. option flips between evaluations on unchanged tables
FLIPS = [("NRT_POD_CLASSES", None), ("NRT_RANK_FILTER", None), ("NRT_RANK_NARROW", None), ("NRT_FUSED", None), ("NRT_PACKED_SCORE", None),
         ("NRT_SINGLE_LAUNCH", None), ("NRT_LN_LIST_PERMILLE", 1), ("TLP_AMB_TABLE", None), ("LROC_FLOAT64", None), ("PEAKS_POD_CLASSES", None),
         ("PEAKS_ESTIMATE", 0), ("PEAKS_ESTIMATE", 8), ("PEAKS_TILE", 88), ("PEAKS_TILE", 44), ("NET_ALLOC_FUSED", None), ("ROW_WORKGROUP", None),
         ("DECIDE_UNFUSED", None)]


def _profile_engine(hdr, e, m, snap, strategy):
    m.nrt_params = nrt_params(hdr, strategy)
    m.tables = flatten_all(e, snap, m.nrt_params, ("tri", "lroc", "peaks", "nrt", "net", "quota"))
    m.snap = snap
    m.apply_params(e)
    upload_all(e, m)


@pytest.mark.parametrize("strategy", ["LeastAllocated", "BalancedAllocation", "LeastNUMANodes"])
def test_option_flips_between_evals(gpu_required, hdr, strategy):
    n_nodes, n_pods = 600, 300
    snap = full_snap(hdr, n_nodes, n_pods, seed=91, flavour="dups")
    full = mask_of(ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD, CAPACITY, LROC, PEAKS)
    unmasked = mask_of(ALLOCATABLE, TLP, LVRB, LROC, PEAKS)
    with Engine(0) as e:
        m = Model(hdr)
        _profile_engine(hdr, e, m, snap, strategy)
        for mask in (full, unmasked):
            e.eval(mask)
            e.sync()
            base = {p: e.all_scores(p).copy() for p in plugins_of(mask) if p != CAPACITY}
            flips = [(k, v) for k, v in FLIPS] + [("REFERENCE_KERNELS", mask_of(p)) for p in plugins_of(mask) if p != CAPACITY]
            for name, value in flips:
                old = e.get_option(name)
                new = (1 - old) if value is None else value
                if new == old:
                    continue
                m.set_option(e, name, new)
                for how in ("eval", "decide"):
                    run(e, how, mask, 0, n_pods)
                    check_fresh(e, m, mask, how=how, ctx=(name, new, how))
                m.set_option(e, name, old)
                e.eval(mask)
                e.sync()
                for p, want in base.items():
                    assert np.array_equal(e.all_scores(p), want), (name, "back", p)


# ------------------------------------------------------------------ 6. parameter changes without re-upload
def test_params_change_without_reupload(gpu_required, hdr, oracle):
    n_nodes, n_pods = 700, 300
    snap = full_snap(hdr, n_nodes, n_pods, seed=101, flavour="ties")
    mask = mask_of(ALLOCATABLE, TLP, LVRB, LROC, PEAKS)
    with Engine(0) as e:
        m = Model(hdr)
        m.tables = flatten_all(e, snap, None, ("tri", "lroc", "peaks"))
        m.snap = snap
        m.apply_params(e)
        upload_all(e, m)
        lroc_paths, amb = set(), []
        steps = [("tlp", 40), ("tlp", 57), ("tlp", 57), ("tlp", 100), ("tlp", 40), ("lvrb", (0.5, 2.0)), ("lvrb", (1.0, 1.0)),
                 ("alloc", ("Most", None)), ("alloc", ("Least", {1: 3, 0: 1 << 20})), ("alloc", ("Least", None)),
                 ("lroc", (1, 0.0, 1.0)), ("lroc", (12, 0.9, 0.2)), ("lroc_nodes", "lim_below_req"), ("lroc", (5, 0.5, 0.5)), ("lroc_nodes", "snapshot"),
                 ("ref_lroc", 1), ("lroc", (3, 0.3, 0.7)), ("ref_lroc", 0),
                 ("weights", {ALLOCATABLE: 3, TLP: 2, LROC: 5}), ("weights", {})]
        for kind, v in steps:
            if kind == "tlp":
                m.tlp_target = v
                e.set_tlp(v)
            elif kind == "lvrb":
                m.lvrb = v
                e.set_lvrb(*v)
            elif kind == "alloc":
                m.alloc = v
                e.set_allocatable(*v)
            elif kind == "lroc":
                m.lroc = v
                e.set_lroc(*v)
            elif kind == "lroc_nodes":  # a node table with limits below requests (the float32 sweep's precondition fails), then back
                cols = e.flatten_lroc_nodes(snap["nodes"], snap["node_pods"])
                if v == "lim_below_req":
                    low = np.flatnonzero(cols["req_cpu_milli"] > 0)[::5]
                    cols["lim_cpu_milli"][low] = cols["req_cpu_milli"][low] - 1
                m.tables["lroc_nodes"] = cols
                e.upload_lroc_nodes(cols)
                m.snap = snap if v == "snapshot" else None
            elif kind == "ref_lroc":
                m.set_option(e, "REFERENCE_KERNELS", mask_of(LROC) if v else 0)
            else:
                m.weights = v
                e.set_plugin_weights(v)
            e.stats(reset=True)
            how = "eval_best" if kind == "weights" else "eval"
            run(e, how, mask, 0, n_pods)
            amb.append(int(e.stats()[TLP]))
            lroc_paths.add((e.kernel_path(LROC), e.get_option("REFERENCE_KERNELS") != 0))
            check_fresh(e, m, mask, how=how, ctx=(kind, v))
            if how == "eval" and m.snap is not None:
                check_oracle(e, m, oracle, mask, range(0, n_pods, 31), ctx=(kind, v))
        assert {(1, False), (0, False), (0, True)} <= lroc_paths  # k_lroc_fast, k_lroc<true> (limits below requests), the int64 form
        assert 0 in amb[1:] and max(amb) > 0  # the TLP ambiguity table rebuilt on some evaluations and reused on others


# ------------------------------------------------------------------ 7. masks and row ranges
def test_masks_and_row_ranges(gpu_required, hdr):
    n_nodes, n_pods = 600, 300
    snap = full_snap(hdr, n_nodes, n_pods, seed=111)
    rng = np.random.default_rng(111)
    with Engine(0) as e:
        m = Model(hdr)
        _profile_engine(hdr, e, m, snap, "LeastAllocated")
        A, AN, AW = mask_of(ALLOCATABLE), mask_of(ALLOCATABLE, NRT), mask_of(ALLOCATABLE, NETOVERHEAD)
        full = mask_of(ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD, CAPACITY, LROC, PEAKS)
        seq = [(full, 17, 140), (full, 0, n_pods), (full, 200, 201), (full, 0, n_pods), (A, 0, n_pods), (AN, 0, n_pods), (A, 0, n_pods),
               (AW, 0, n_pods), (AW, 30, 90), (A, 0, n_pods), (mask_of(TLP, PEAKS), 5, 260), (mask_of(TLP, PEAKS), 0, n_pods)]
        for mask, b, end in seq:
            e.eval(mask, b, end)
            e.sync()
            check_fresh(e, m, mask, b, end, ctx=(mask, b, end))
        for ext in (rng.random((n_pods, n_nodes)) < 0.7, None, rng.random((n_pods, n_nodes)) < 0.4):
            e.upload_feasible_mask(ext)
            m.ext = None if ext is None else ext.astype(np.uint8)
            for mask in (A, full, mask_of(PEAKS, TLP)):
                for how in ("eval", "decide"):
                    run(e, how, mask, 0, n_pods)
                    check_fresh(e, m, mask, how=how, ctx=("ext", ext is None, mask, how))


# ------------------------------------------------------------------ 8. after the commit loop
def test_eval_after_commit_loop(gpu_required, hdr):
    n_nodes, n_pods = 600, 300
    snap = full_snap(hdr, n_nodes, n_pods, seed=121)
    new = full_snap(hdr, n_nodes, n_pods, seed=122)
    full = mask_of(ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD, CAPACITY, LROC, PEAKS)
    commits = [mask_of(ALLOCATABLE, TLP), mask_of(ALLOCATABLE, LVRB), mask_of(NRT), mask_of(ALLOCATABLE, NRT, NETOVERHEAD),
               mask_of(NETOVERHEAD, CAPACITY), mask_of(ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD, CAPACITY)]
    with Engine(0) as e:
        m = Model(hdr)
        _profile_engine(hdr, e, m, snap, "LeastAllocated")
        for i, cm in enumerate(commits):
            if i == 2:  # a trimaran node delta before this commit
                idx = np.random.default_rng(5).choice(n_nodes, 31, replace=False)
                cols_new = e.flatten_trimaran_nodes(snap["nodes"], new["metrics"], new["assigned"])
                e.update_trimaran_nodes(idx, cols_new)
                for k in m.tables["tri_nodes"]:
                    m.tables["tri_nodes"][k] = m.tables["tri_nodes"][k].copy()
                    m.tables["tri_nodes"][k][idx] = cols_new[k][idx]
            if i == 4:  # a parameter change before this commit
                m.tlp_target = 63
                e.set_tlp(63)
            e.commit_sequential(cm, 0, 48)
            other = full if i % 2 else mask_of(ALLOCATABLE, TLP, LVRB, NRT, LROC)
            e.eval(other)
            e.sync()
            check_fresh(e, m, other, ctx=("commit", cm))


# ------------------------------------------------------------------ spx_load_profile: errors
def test_load_profile_errors(gpu_required, hdr):
    import ctypes as C

    from scheduler_plugins_amd import SpxError
    snap = synth.full_snapshot(hdr, 64, 32, seed=3)
    with Engine(0) as e:
        with pytest.raises(SpxError) as ex:  # nrt without nrt_params
            e.load_c(snap, None, concurrent=True)
        assert ex.value.code == hdr.consts["SPX_ERR_ARG"] and "nrt_params" in ex.value.msg
        with pytest.raises(SpxError):  # a failure of this thread on this engine first: its message must not come back below
            e.set_option("PEAKS_TILE", 3)
        # a loader that fails on a worker thread (spx_load_nrt: an illegal strategy)
        params = nrt_params(hdr, "LeastAllocated")
        params.struct.strategy = 7
        with pytest.raises(SpxError) as ex:
            e.load_c(snap, params, concurrent=True)
        msg = ex.value.msg
        assert ex.value.code == hdr.consts["SPX_ERR_ARG"] and "strategy" in msg and "PEAKS_TILE" not in msg, msg
        assert e._lib.spx_last_error(e._h).decode() == msg
        # through the C ABI with an explicit NULL
        t = e._hdr.structs["spx_profile_objects"]()
        t.nodes, t.pods, t.nrt = C.pointer(snap["nodes"].struct), C.pointer(snap["pods"].struct), C.pointer(snap["nrt"].struct)
        assert e._lib.spx_load_profile(e._h, C.byref(t)) == hdr.consts["SPX_ERR_ARG"]


# ------------------------------------------------------------------ seeded walks over the full profile
FLAVOURS = ["regular", "ties", "big_cpu", "wide", "permute", "cost_over_255", "lroc_lim_below_req", "peaks_negative", "dups", "unique"]
OPS = ["reload", "reload_c", "reload_concurrent", "nrt_nodes", "tri_delta", "nrt_delta", "strategy", "option", "params", "range",
       "ext", "commit", "net_placed", "quota_used", "decide"]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_walk(gpu_required, hdr, oracle, seed):
    t0 = time.time()
    rng = np.random.default_rng(1000 + seed)
    n_nodes, n_pods = 512 + 128 * seed, 240 + 40 * seed
    full = mask_of(ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD, CAPACITY, LROC, PEAKS)
    masks = [full, mask_of(ALLOCATABLE, TLP, LVRB, LROC, PEAKS), mask_of(NRT), mask_of(ALLOCATABLE, NRT, PEAKS), mask_of(TLP, LVRB),
             mask_of(NETOVERHEAD, CAPACITY, ALLOCATABLE)]
    snaps = {}

    def snap_of(fl):
        if fl not in snaps:
            snaps[fl] = full_snap(hdr, n_nodes, n_pods, seed=200 + seed * 10 + FLAVOURS.index(fl), flavour=fl)
        return snaps[fl]

    history = []
    cov = {"filter_path": set(), "bal_fused": False, "nrt_kp": set(), "tlp_kp": set(), "nrt_cls": set(), "pk_cls": set(), "lroc": set(), "amb": set()}
    with Engine(0) as e:
        m = Model(hdr)
        strategy = "BalancedAllocation"
        _profile_engine(hdr, e, m, snap_of("regular"), strategy)
        steps = ["reload"] + list(rng.choice(OPS, 29))
        # the coverage the walk exists for is drawn on purpose at fixed steps: the fused walk after a declined one, the generic kernel
        steps[3], steps[5], steps[9], steps[12], steps[15], steps[18], steps[21] = (
            "reload_dups", "big_cpu_then_exact", "reload_unique", "reload_permute", "ref_on", "lroc_params", "ref_off")
        try:
            for i, op in enumerate(steps):
                mask, b, end, how = full, 0, n_pods, "eval"
                whole = False
                if op.startswith("reload"):
                    fl = op[7:] if op.count("_") == 1 and op[7:] in FLAVOURS else FLAVOURS[int(rng.integers(len(FLAVOURS)))]
                    strategy = STRATEGIES[int(rng.integers(3))] if fl != "permute" else "LeastAllocated"
                    s = snap_of(fl)
                    m.nrt_params = nrt_params(hdr, strategy)
                    m.tables = flatten_all(e, s, m.nrt_params, ("tri", "lroc", "peaks", "nrt", "net", "quota"))
                    m.placed, m.snap, whole = [], s, True
                    if op not in ("reload_c", "reload_concurrent") or "quota_rc" in s:
                        upload_all(e, m)
                    else:
                        e.load_c(s, m.nrt_params, concurrent=op == "reload_concurrent")
                        e.upload_lroc_nodes(m.tables["lroc_nodes"]), e.upload_lroc_pods(m.tables["lroc_pods"])
                        e.upload_peaks(m.tables["peaks"])
                    op = f"{op}:{fl}:{strategy}"
                elif op == "big_cpu_then_exact":
                    strategy = "BalancedAllocation"
                    m.nrt_params = nrt_params(hdr, strategy)
                    base = snap_of("regular")  # its tables in full first, then its zone tables with big cpu capacities and back
                    m.tables = flatten_all(e, base, m.nrt_params, ("tri", "lroc", "peaks", "nrt", "net", "quota"))
                    m.placed, m.snap = [], base
                    upload_all(e, m)
                    big = full_snap(hdr, n_nodes, n_pods, seed=200 + seed * 10, flavour="big_cpu")  # (the same nodes as base)
                    for fl, s in (("big_cpu", big), ("regular", base)):
                        f = e.flatten_nrt(s["nodes"], s["nrt"], s["rc"], base["pods"], m.nrt_params)
                        e.upload_nrt_nodes(f["nodes"], f["R"])
                        m.tables["nrt"] = dict(m.tables["nrt"], nodes=f["nodes"])
                        m.snap = None
                        run(e, "eval", mask_of(NRT), 0, n_pods)
                        cov["filter_path"].add(e.nrt_filter_path())
                        check_fresh(e, m, mask_of(NRT), ctx=(i, op, fl))
                    if e.nrt_filter_path() == 3:
                        cov["bal_fused"] = True
                    mask = mask_of(NRT)
                elif op in ("ref_on", "ref_off"):  # the reference-arithmetic sweeps (kernel_path 0) and back
                    m.set_option(e, "REFERENCE_KERNELS", mask_of(TLP, NRT, LROC) if op == "ref_on" else 0)
                elif op == "nrt_nodes":
                    f = m.tables["nrt"]
                    nodes = {k: v.copy() for k, v in f["nodes"].items()}
                    av = nodes["zone_avail"].reshape(f["N"], 8, f["R"])
                    cand = rng.choice(f["N"], 25, replace=False)
                    av[cand] += np.where(av[cand] > 0, av[cand] // 3, 0)
                    e.upload_nrt_nodes(nodes, f["R"])
                    m.tables["nrt"] = dict(f, nodes=nodes)
                    m.snap = None
                elif op == "tri_delta":
                    idx = rng.choice(n_nodes, 20, replace=False)
                    cols = {k: v.copy() for k, v in m.tables["tri_nodes"].items()}
                    cols["tlp_cpu_util"][idx] = rng.choice([0.0, 12.5, 40.0, 62.5, 99.5], idx.size)
                    cols["lv_cpu_avg"][idx] = cols["lv_cpu_avg"][idx][::-1]
                    if rng.random() < 0.5:
                        e.update_trimaran_nodes(idx, cols)
                    else:
                        e.update_trimaran_node_rows(idx, {k: np.ascontiguousarray(v[idx]) for k, v in cols.items()})
                    m.tables["tri_nodes"] = cols
                    m.snap = None
                elif op == "nrt_delta":
                    other = snap_of("regular")
                    f = m.tables["nrt"]
                    if other["nrt"].struct.n_nodes == f["N"] and f["R"] == 4:
                        idx = rng.choice(n_nodes, 15, replace=False)
                        rows = e.flatten_nrt_node_rows(m.snap["nodes"] if m.snap else other["nodes"], other["nrt"], f["slots"], idx)
                        nodes = {k: v.copy() for k, v in f["nodes"].items()}
                        for k, v in rows.items():
                            w = v.size // idx.size
                            nodes[k].reshape(n_nodes, w)[idx] = v.reshape(idx.size, w)
                        if rng.random() < 0.5:
                            e.update_nrt_node_rows(idx, rows, f["R"])
                        else:
                            e.update_nrt_nodes(idx, dict(f, nodes=nodes))
                        m.tables["nrt"] = dict(f, nodes=nodes)
                        m.snap = None
                elif op == "strategy":
                    strategy = STRATEGIES[int(rng.integers(4))]
                    m.nrt_params = nrt_params(hdr, strategy)
                    e.set_nrt_params(m.nrt_params)
                    whole = m.snap is not None
                elif op == "option":
                    name, value = FLIPS[int(rng.integers(len(FLIPS)))]
                    old = e.get_option(name)
                    m.set_option(e, name, (1 - old) if value is None else (value if old != value else {"PEAKS_ESTIMATE": 1, "PEAKS_TILE": 84}.get(name, 1000)))
                    if rng.random() < 0.3:
                        m.set_option(e, "REFERENCE_KERNELS", int(rng.integers(0, 256)) & ~mask_of(CAPACITY))
                    op = f"option:{name}"
                elif op in ("params", "lroc_params"):
                    which = "lroc" if op == "lroc_params" else ["tlp", "lvrb", "alloc", "lroc", "weights"][int(rng.integers(5))]
                    if which == "tlp":
                        m.tlp_target = int(rng.choice([20, 40, 57, 85]))
                    elif which == "lvrb":
                        m.lvrb = (float(rng.choice([0.5, 1.0, 2.0])), float(rng.choice([0.5, 1.0, 3.0])))
                    elif which == "alloc":
                        m.alloc = (["Least", "Most"][int(rng.integers(2))], {1: int(rng.integers(1, 4)), 0: 1 << 20})
                    elif which == "lroc":
                        m.lroc = (int(rng.integers(1, 12)), float(rng.random()), float(rng.random()))
                    else:
                        m.weights = {int(p): int(rng.integers(1, 5)) for p in (ALLOCATABLE, TLP, NRT, LROC)}
                    m.apply_params(e)
                    whole = m.snap is not None
                    op = f"params:{which}"
                elif op == "range":
                    b = int(rng.integers(0, n_pods - 2))
                    end = int(rng.integers(b + 1, n_pods + 1))
                    mask = masks[int(rng.integers(len(masks)))]
                elif op == "ext":
                    m.ext = None if (m.ext is not None and rng.random() < 0.5) else (rng.random((n_pods, n_nodes)) < 0.8).astype(np.uint8)
                    e.upload_feasible_mask(m.ext)
                elif op == "commit":
                    cm = [mask_of(ALLOCATABLE, TLP), mask_of(NRT), mask_of(ALLOCATABLE, NRT, NETOVERHEAD, CAPACITY)][int(rng.integers(3))]
                    e.commit_sequential(cm, 0, 24)
                    mask = masks[int(rng.integers(len(masks)))]
                elif op == "net_placed":
                    s = m.snap
                    if s is not None and not m.placed:  # (entries are relative to the AppGroups last flattened)
                        ag = s["appgroups"]
                        group = rng.integers(0, ag.struct.n_groups, 12).astype(np.int32)
                        wl_ptr, wl_sel = ag.array("wl_ptr"), ag.array("wl_selector")
                        selector = np.array([wl_sel[rng.integers(wl_ptr[g], wl_ptr[g + 1])] for g in group], np.int32)
                        ent = e.flatten_net_placed(s["pods"], ag, group, selector, rng.integers(0, n_nodes, 12).astype(np.int32))
                        if len(ent["key"]):
                            e.update_net_placed(ent)
                            m.placed.append(ent)
                            m.snap = None
                elif op == "quota_used":
                    q = m.tables["quota"]
                    ns = np.array([0, 1], np.int32)
                    used = q["ns"]["used"].reshape(-1, 8)[ns] + 1000
                    up = np.ones(2, np.uint8)
                    agg = q["cols"]["agg_used"] + 2000
                    e.update_quota_used(ns, used, up, agg, np.ones(1, np.uint8))
                    q = dict(q, ns=dict(q["ns"]), cols=dict(q["cols"]))
                    q["ns"]["used"] = q["ns"]["used"].copy().reshape(-1, 8)
                    q["ns"]["used"][ns] = used
                    q["ns"]["used"] = q["ns"]["used"].reshape(-1)
                    q["ns"]["used_present"] = q["ns"]["used_present"].copy()
                    q["ns"]["used_present"][ns] = 1
                    q["cols"]["agg_used"], q["cols"]["agg_used_present"] = agg, np.ones(1, np.uint8)
                    m.tables["quota"] = q
                    m.snap = None
                elif op == "decide":
                    how = ["decide", "eval_best"][int(rng.integers(2))]
                    mask = masks[int(rng.integers(len(masks)))]
                history.append((i, op, hex(mask), b, end, how))
                e.stats(reset=True)
                run(e, how, mask, b, end)
                st = e.stats()
                if mask & mask_of(NRT):
                    cov["filter_path"].add(e.nrt_filter_path())
                    if strategy == "BalancedAllocation" and e.nrt_filter_path() == 3:
                        cov["bal_fused"] = True
                    cov["nrt_cls"].add(e.nrt_pod_classes()[1] * 32 >= n_pods)
                cov["nrt_kp"].add(e.kernel_path(NRT))
                cov["tlp_kp"].add(e.kernel_path(TLP))
                cov["pk_cls"].add(e.peaks_pod_classes()[1] * 8 >= n_pods)
                if mask & mask_of(LROC):
                    cov["lroc"].add(e.kernel_path(LROC))
                if mask & mask_of(TLP) and end - b >= 256 and how == "eval":
                    cov["amb"].add(int(st[TLP]) > 0)
                check_fresh(e, m, mask, b, end, how=how, ctx=(i, op))
                if whole and how == "eval" and m.ext is None and (strategy != "LeastNUMANodes"):
                    check_oracle(e, m, oracle, mask, range(i % 7, n_pods, 53), ctx=(i, op))
        except AssertionError:
            print("walk history:", *history, sep="\n  ")
            raise
    assert {1, 2, 3} <= cov["filter_path"] and cov["bal_fused"], cov
    assert {0, 1} <= cov["nrt_kp"] and {0, 1} <= cov["tlp_kp"], cov
    assert {True, False} <= cov["nrt_cls"] and {True, False} <= cov["pk_cls"], cov
    assert {0, 1} <= cov["lroc"], cov
    print(f"walk {seed}: {len(steps)} steps in {time.time() - t0:.1f} s, coverage {cov}")
