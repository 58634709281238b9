"""SySched's sweep beside Peaks' default sweep at the headline shape, in one process on one device.

Both are sweeps of the same structure — one normalised row per class of pods, copied to the rest of the class, 1 B per cell — so
both should sit at the write floor of the 1 GB table; the SySched sweep (spx_last_eval_ms, median of the steady steps) is asked
to take no more than 1.25 x the Peaks time of the same run.  The two are timed alternately, after a warm-up of each.  Also
reported, not gated: with a caller feasibility mask in play, SySched's per-row pass (k_sysched_rows) next to Allocatable's
feasibility-aware row pass on the same engine.

    python tools/sysched_ab.py [--nodes 10000] [--pods 100000] [--steps 30] [--warmup 5] [--no-mask] [--out FILE.json]

Prints one JSON line; exit status 1 when the ratio is above 1.25."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import scheduler_plugins_amd as spx  # noqa: E402
from scheduler_plugins_amd import synth  # noqa: E402
from scheduler_plugins_amd.engine import ALLOCATABLE, PEAKS, SYSCHED, Engine, mask_of  # noqa: E402


def timed(e, mask, steps, warmup):
    out = []
    for i in range(warmup + steps):
        e.eval(mask)
        e.sync()
        if i >= warmup:
            out.append(e.last_eval_ms())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--pods", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profiles", type=int, default=32)
    ap.add_argument("--no-mask", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    hdr = spx.header()
    tri = synth.trimaran_snapshot(hdr, a.nodes, a.pods, seed=synth.SEED, round_frac=0.1)
    pm = synth.synth_power_models(hdr, a.nodes, synth.SEED)
    sy = synth.sysched_snapshot(hdr, a.nodes, a.pods, seed=synth.SEED, n_profiles=a.profiles)
    res = {"shape": [a.nodes, a.pods], "steps": a.steps, "warmup": a.warmup}
    with Engine(0) as e:
        e.load_trimaran_objects(tri["nodes"], tri["rc"], tri["pods"], tri["metrics"], tri["assigned"])
        e.load_peaks_objects(tri["nodes"], tri["metrics"], pm, tri["pods"])
        e.load_sysched_objects(sy["objects"])
        res["sysched_classes"], res["peaks_classes"] = e.sysched_pod_classes()[0], e.peaks_pod_classes()[0]
        timed(e, mask_of(SYSCHED), 0, a.warmup)
        timed(e, mask_of(PEAKS), 0, a.warmup)
        s_ms, p_ms = [], []
        for _ in range(a.steps):  # alternating: what else runs on the machine hits both alike
            s_ms += timed(e, mask_of(SYSCHED), 1, 0)
            p_ms += timed(e, mask_of(PEAKS), 1, 0)
        res["sysched_ms"], res["peaks_ms"] = statistics.median(s_ms), statistics.median(p_ms)
        res["sysched_min_max"], res["peaks_min_max"] = [min(s_ms), max(s_ms)], [min(p_ms), max(p_ms)]
        res["ratio"] = res["sysched_ms"] / res["peaks_ms"]
        res["sysched_chunks"] = e.kernel_path(SYSCHED)
        if not a.no_mask:
            rng = np.random.default_rng(1)
            mask = rng.integers(0, 2, (a.pods, a.nodes), dtype=np.uint8)
            e.upload_feasible_mask(mask)
            del mask
            timed(e, mask_of(SYSCHED), 0, 2)
            timed(e, mask_of(ALLOCATABLE), 0, 2)
            sm, am = [], []
            for _ in range(max(5, a.steps // 3)):
                sm += timed(e, mask_of(SYSCHED), 1, 0)
                am += timed(e, mask_of(ALLOCATABLE), 1, 0)
            res["masked_sysched_rows_ms"], res["masked_allocatable_rows_ms"] = statistics.median(sm), statistics.median(am)
    res["gate"] = "ok" if res["ratio"] <= 1.25 else "above 1.25"
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0 if res["ratio"] <= 1.25 else 1


if __name__ == "__main__":
    sys.exit(main())
