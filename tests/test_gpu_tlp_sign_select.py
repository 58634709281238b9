"""The streamlined cell of k_tlp_fast2 picks its branch by u's sign bit (v_ashrrev_i32 + v_bitop3_b32 / v_bfi_b32) where the checked
cell compares `u > 0`: the two differ for u = +0.0 only, and +0.0 must never reach the streamlined path (k_tlp_amb_build lists the
pod value -b of every node for the node's tile, a listed row takes the checked cell).  Aimed at exactly that: snapshots whose
`b = util * cap / 100 + missing - T * cap / 100` is an integer (dyadic utilisations: the float64 product is exact) or an integer give
or take one rounding of the product (whole-percent utilisations: u a few float32 ulps of `b2l` either side of 0), and pods at -b - 1,
-b and -b + 1 of many nodes — more than 256 rows (the table form), three node tiles, targets 1 / 40 / 73, with Allocatable in the
launch and without, tables and spx_decide.  Every cell against the oracle and against an engine with TLP_AMB_TABLE off."""
import numpy as np
import pytest

from helpers import ALLOCATABLE, TLP, tlp_params
from scheduler_plugins_amd import synth
from scheduler_plugins_amd.engine import Engine, mask_of

pytestmark = pytest.mark.gpu

N_NODES, N_PODS = 2_500, 700   # 3 tiles of 1024 nodes, 11 chunks of 64 rows
TILE = 1024                    # nodes per wave of k_tlp_fast2 (64 lanes x 16)
AMB_SIZE = 1 << 16             # pod values k_tlp_amb_build's table covers
TARGETS = (1, 40, 73)


def _crafted_snapshot(hdr, target):
    """config #2's synthetic snapshot with the CPU utilisations replaced: 45 % dyadic percentages (util / 100 * cap exact for the
    synthetic capacities, multiples of 1000), 45 % whole percentages (exact or one ulp off), 10 % left continuous"""
    snap = synth.trimaran_snapshot(hdr, N_NODES, N_PODS, seed=500 + target)
    m = snap["metrics"]
    val, typ, op = m.array("m_value"), m.array("m_type"), m.array("m_op")
    rng = np.random.default_rng(900 + target)
    cpu = (typ == 0) & (op != 1)   # CPU AVG / Latest: what TLP reads
    kind = rng.random(len(val))
    dyadic = rng.choice(np.array([0.0, 12.5, 25.0, 37.5, 50.0, 62.5, 75.0]), len(val))
    val[...] = np.where(cpu & (kind < 0.45), dyadic, np.where(cpu & (kind < 0.9), np.round(val), val))
    return snap


def _node_b(cols, target):
    """b of k_tlp_prepare_fast, in its float64 operation order; NaN for a node the sweep never sees as a number"""
    cap = cols["cap_cpu_milli"].astype(np.float64)
    um = (cols["tlp_cpu_util"] / 100.0) * cap
    miss = cols["tlp_missing_milli"].astype(np.float64)
    ok = (cols["tlp_valid"] != 0) & (cap > 0) & (um >= 0) & (miss >= 0)
    with np.errstate(invalid="ignore"):
        return np.where(ok, (um + miss) - target * cap / 100.0, np.nan)


def _aim_pods(e, snap, target):
    """patches the cpu of the first pods to -b - 1, -b, -b + 1 of nodes with (nearly) integer b; returns (tlp_pod_milli, b)"""
    b = _node_b(e.flatten_trimaran_nodes(snap["nodes"], snap["metrics"], snap["assigned"]), target)
    near = np.flatnonzero(np.isfinite(b) & (np.abs(b - np.rint(b)) < 1e-9) & (-b >= 2) & (-b < 60_000))
    assert len(near) >= 20, len(near)
    rng = np.random.default_rng(7 + target)
    pick = rng.permutation(near)[:200]
    vals = np.unique(np.concatenate([(-np.rint(b[pick])).astype(np.int64) + d for d in (-1, 0, 1)]))
    vals = rng.permutation(vals)[:N_PODS - 100]  # the last 100 pods stay as drawn
    pods = snap["pods"]
    cp, qp, lp = pods.array("ctr_ptr"), pods.array("req_ptr"), pods.array("lim_ptr")
    for i, m in enumerate(vals):   # as tests/test_gpu_trimaran.py does: the first container carries the value, the others 0
        for c in range(cp[i], cp[i + 1]):
            for ptr, rs, qt in ((qp, pods.array("req_res"), pods.array("req_qty")), (lp, pods.array("lim_res"), pods.array("lim_qty"))):
                for k in range(ptr[c], ptr[c + 1]):
                    if rs[k] == 0:
                        qt[k] = int(m) if c == cp[i] else 0
    return e.flatten_trimaran_pods(pods)["tlp_pod_milli"], b


def _zero_cells(pod_milli, b):
    """(cells with p + b exactly 0, cells with 0 < |p + b| < 1e-9) over the whole table, in float64 (p + rint(b) is exact)"""
    fin = np.flatnonzero(np.isfinite(b))
    u = pod_milli[:, None].astype(np.float64) + b[None, fin]
    return int((u == 0).sum()), int(((u != 0) & (np.abs(u) < 1e-9)).sum())


def _slow_share(cols, pod_milli, target):
    """share of (row, tile) pairs that take the checked cell in the table form, from the semantics of k_tlp_prepare_fast (a node
    without float32 constants makes its whole tile checked), k_tlp_amb_build (bit per (pod value, tile)) and k_tlp_fast2 (pods
    outside the table or outside float32's integers)"""
    t = float(target)
    c1, c2 = t / (100.0 - t), (100.0 - t) / t
    cap = cols["cap_cpu_milli"].astype(np.float64)
    um = (cols["tlp_cpu_util"] / 100.0) * cap
    miss = cols["tlp_missing_milli"].astype(np.float64)
    valid = cols["tlp_valid"] != 0
    n_tiles = (len(cap) + TILE - 1) // TILE
    tile = np.arange(len(cap)) // TILE
    sane = (um >= 0) & (miss >= 0) & (cap > 0) & (um < 1e15) & (miss < 1e15)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = 100.0 / cap
        b = (um + miss) - t * cap / 100.0
        split = (np.abs(b) < 8388607.0) & (c1 * k >= 2.5 * 4e-5) & (c2 * k >= 2.5 * 4e-5)
        tile_nan = np.zeros(n_tiles, bool)
        np.logical_or.at(tile_nan, tile, valid & (cap != 0) & ~(sane & split))
        amb = np.zeros((AMB_SIZE, n_tiles), bool)
        live = valid & sane
        j = np.arange(100) + 0.5
        for p_star, slope in (((t - j[None, :]) / (c1 * k)[:, None] - b[:, None], np.broadcast_to((c1 * k)[:, None], (len(cap), 100))),
                              ((j[None, :] - 100.0) / (c2 * k)[:, None] - b[:, None], np.broadcast_to((c2 * k)[:, None], (len(cap), 100))),
                              (-b[:, None], np.full((len(cap), 1), 2e-6 / (4e-5 * 1.25)))):
            pn = np.rint(p_star)
            hit = live[:, None] & (np.abs(p_star - pn) * slope < 4e-5 * 1.25) & (pn >= 0) & (pn < AMB_SIZE)
            nn, _ = np.nonzero(hit)
            amb[pn[hit].astype(np.int64), tile[nn]] = True
    p = pod_milli
    outside = (p < 0) | (p >= AMB_SIZE)
    slow = tile_nan[None, :] | outside[:, None] | amb[np.clip(p, 0, AMB_SIZE - 1)]
    return float(slow.mean())


def _run(e, with_alloc):
    mask = mask_of(ALLOCATABLE, TLP) if with_alloc else mask_of(TLP)
    e.stats(reset=True)
    e.eval(mask)
    e.sync()
    table = e.all_scores(TLP)
    n_re = int(e.stats()[TLP])
    e.decide(mask)
    e.sync()
    return table, e.best(), n_re


@pytest.mark.parametrize("with_alloc", [True, False], ids=["alloc+tlp", "tlp"])
@pytest.mark.parametrize("target", TARGETS)
def test_sign_select_equals_compare_at_the_branch_point(gpu_required, hdr, oracle, target, with_alloc):
    snap = _crafted_snapshot(hdr, target)
    got = {}
    with Engine(0) as e:
        e.set_tlp(target_utilization=target)
        pod_milli, b = _aim_pods(e, snap, target)
        n_zero, n_near = _zero_cells(pod_milli, b)
        share = _slow_share(e.flatten_trimaran_nodes(snap["nodes"], snap["metrics"], snap["assigned"]), pod_milli, target)
        print(f"target {target}: {n_zero} cells with p + b == 0, {n_near} within 1e-9 of it, checked (row, tile) share {share:.3f}")
        # the inputs do hold the branch point, exactly and nearly (target 1: only utilisation 0 lies below the target, and 0 x cap is exact)
        assert n_zero >= 100 and (n_near >= 1 or target == 1), (n_zero, n_near)
        e.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])
        for opt in (1, 0):
            e.set_option("TLP_AMB_TABLE", opt)
            got[opt] = _run(e, with_alloc)
        osnap = oracle.Snapshot(snap["nodes"], snap["pods"], rc=snap["rc"], metrics=snap["metrics"], assigned=snap["assigned"],
                                alloc_params=e.alloc_params, tlp_params=tlp_params(hdr, target_utilization=target))
    want = osnap.score_rows(TLP, threads=oracle.usable_cpus(), want_norm=False)[0]
    for opt in (1, 0):
        bad = got[opt][0].astype(np.int64) != want
        assert not bad.any(), (opt, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert np.array_equal(got[1][0], got[0][0])
    for x, y in zip(got[1][1], got[0][1]):   # spx_decide: node, score, ties, feasible
        assert np.array_equal(x, y)
    assert got[1][2] > 0 and got[0][2] > 0   # the exact path ran in both forms


def test_the_crafted_rows_do_reach_the_streamlined_path(gpu_required, hdr):
    """the cases above cannot pass by sending every row down the checked path: for at least one target fewer than half of the (row,
    tile) pairs carry the ambiguity bit (target 1: the u > 0 slope T / (100 - T) x 100 / cap is below kAmbMinSlope for all but the
    smallest nodes, so every tile is checked there — that parametrisation covers the table form's all-checked case instead)"""
    shares = {}
    with Engine(0) as e:
        for target in TARGETS:
            snap = _crafted_snapshot(hdr, target)
            e.set_tlp(target_utilization=target)
            pod_milli, _ = _aim_pods(e, snap, target)
            shares[target] = _slow_share(e.flatten_trimaran_nodes(snap["nodes"], snap["metrics"], snap["assigned"]), pod_milli, target)
    print("checked (row, tile) share per target:", shares)
    assert min(shares.values()) < 0.5, shares
