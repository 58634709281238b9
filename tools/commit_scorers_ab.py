#!/usr/bin/env python3
"""Sequential commit, per-pod route: the present full mask against the same mask with LROC and PEAKS added.

Runs the loop on config #5's share shape (bench.py's config5_leg: 8 192 pods x 20 000 nodes) with SPX_OPT_COMMIT_COOP off, three
alternating runs of each mask on one engine, and reports microseconds per pod for both.  With --trace it re-runs itself once
under `rocprofv3 --kernel-trace --stats` (the program after `--`) and prints the per-kernel split of that run.

    python tools/commit_scorers_ab.py [--pods 8192] [--trace] [--out DIR]

The first mask is the yardstick: run the same script on the parent commit (it skips the second mask there) and compare the first
mask's spread between the two builds."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(n_pods, repeats):
    import bench
    import scheduler_plugins_amd as spx
    from scheduler_plugins_amd import synth
    from scheduler_plugins_amd.engine import Engine
    hdr = spx.header()
    w = dict(bench.WORKLOADS["config5_share"], n_pods=n_pods)
    snap = bench.build_snapshot(hdr, w, n_pods, bench.synth_seed())
    base = 0
    for p in w["plugins"]:
        base |= 1 << bench.PID[p]
    LROC, PEAKS = 7, 8
    out = {"n_nodes": w["n_nodes"], "n_pods": n_pods, "base_us_per_pod": [], "scorers_us_per_pod": []}
    with Engine(0) as e:
        bench.load_tables(e, w, snap)
        e.set_option("COMMIT_COOP", 0)
        masks = [("base", base)]
        try:
            e.set_lroc()
            e.load_lroc_objects(snap["nodes"], synth.synth_node_pods(hdr, w["n_nodes"], bench.synth_seed()), snap["pods"])
            e.load_peaks_objects(snap["nodes"], snap["metrics"], synth.synth_power_models(hdr, w["n_nodes"], bench.synth_seed()), snap["pods"])
            e.commit_sequential(base | (1 << LROC) | (1 << PEAKS), 0, 64, want_ties=False)
            masks.append(("scorers", base | (1 << LROC) | (1 << PEAKS)))
        except Exception as ex:  # a build whose loop rejects the two plugins: the first mask alone
            out["scorers_error"] = str(ex)[:200]
        for _, m in masks:
            e.commit_sequential(m, 0, 256, want_ties=False)  # first call allocates
        for _ in range(repeats):
            for name, m in masks:
                t0 = time.perf_counter()
                node, _, _, _ = e.commit_sequential(m, want_ties=False)
                out[f"{name}_us_per_pod"].append((time.perf_counter() - t0) * 1e6 / n_pods)
                out[f"{name}_path"] = e.commit_path()
                out[f"{name}_bound"] = int((node >= 0).sum())
    if out["scorers_us_per_pod"]:
        out["added_us_per_pod"] = sorted(out["scorers_us_per_pod"])[len(out["scorers_us_per_pod"]) // 2] - sorted(out["base_us_per_pod"])[len(out["base_us_per_pod"]) // 2]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="one more run of this script under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=os.path.join(tempfile.gettempdir(), "commit_scorers"), help="directory for the trace run's files")
    a = ap.parse_args()
    print(json.dumps(run(a.pods, a.repeats)), flush=True)
    if a.trace:
        os.makedirs(a.out, exist_ok=True)
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", a.out, "-o", "trace", "--output-format", "csv", "--",
                        sys.executable, os.path.abspath(__file__), "--pods", str(min(a.pods, 2048)), "--repeats", "1"], check=True, timeout=900)
        for root, _, files in os.walk(a.out):
            for f in files:
                if f.endswith("kernel_stats.csv"):
                    print(open(os.path.join(root, f)).read()[:6000])


if __name__ == "__main__":
    main()
