"""CapacityScheduling's dry run with NRT's Filter in the refit at a realistic size, beside the fit-only dry run on the same upload.

tools/preempt_time.py's snapshot (synth.preempt_model, seed 41, quotas on) decorated with containers, two NUMA zones per node and placement
info (tests/ptol_nrt_cases.decorate) goes through the object builders and the flatteners to the device.  Each timed step runs one entry
point for all preemptors x all nodes (row records, cells, pick) and spx_last_eval_ms of that call is reported (median, min, max), in one
process:

    fit_only        spx_preempt_dry_run
    mode_enabled    spx_preempt_nrt_dry_run, preemption mode on
    mode_disabled   the same, preemption mode off (the Filter on the live table)
    best_effort     the same on a second upload whose preemptors are all BestEffort without non-native requests (the Filter passes unseen)

    python tools/preempt_nrt_time.py [--nodes 10000] [--pods-per-node 30] [--preemptors 1024] [--steps 10] [--warmup 2] [--out FILE.json]

Prints one JSON line.  A number for the record, not a gate."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import preempt_nrt_cases as CC  # noqa: E402
import ptol_nrt_cases as NC  # noqa: E402
from ptol_nrt_time import best_effort  # noqa: E402
from ptol_time import timed  # noqa: E402
from scheduler_plugins_amd import synth  # noqa: E402
from scheduler_plugins_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--pods-per-node", type=float, default=30.0)
    ap.add_argument("--preemptors", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    say = lambda *x: print(*x, file=sys.stderr, flush=True)
    rows = np.arange(a.preemptors)
    out = {"shape": {"nodes": a.nodes, "preemptors": a.preemptors}, "steps": a.steps, "warmup": a.warmup}

    t0 = time.perf_counter()
    m = NC.decorate(synth.preempt_model(a.nodes, a.preemptors, seed=41, pods_per_node=a.pods_per_node), 41, zones=(2,), max_ctrs=3)
    t = CC.build_tables(m)
    say(f"model drawn, decorated and object tables built in {time.perf_counter() - t0:.1f} s")

    def counts(e):
        st, _, _ = e.preempt_cells(0, min(64, a.preemptors))
        return dict(status_counts_first_rows=np.bincount(st.ravel(), minlength=8).tolist(), rows_with_a_pick=int((e.preempt_pick()["node"] >= 0).sum()))

    with Engine(0) as e:
        f = CC.load(e, t)
        g = f["nrt"]
        out["shape"].update(assigned_pods=int(f["pod_ptr"][-1]), longest_list=int(np.diff(f["pod_ptr"]).max()), slots=g["R"], zones_per_node=2,
                            nodes_with_nrt=int((g["node_flags"] & 1).astype(bool).sum()), nodes_simulating=int((g["node_flags"] & 16).astype(bool).sum()),
                            contributing_pods=int(g["pod_contributes"].sum()), releases=len(g["rel_qty"]))
        runs = {"fit_only": lambda: e.preempt_dry_run(rows), "mode_enabled": lambda: e.preempt_nrt_dry_run(rows, None, True),
                "mode_disabled": lambda: e.preempt_nrt_dry_run(rows, None, False)}
        for name, step in runs.items():
            out[name] = dict(timed(e, step, a.warmup, a.steps), **counts(e))
            say(name, json.dumps(out[name]))
    t = CC.build_tables(best_effort(m))
    with Engine(0) as e:
        CC.load(e, t)
        out["best_effort"] = dict(timed(e, lambda: e.preempt_nrt_dry_run(rows, None, True), a.warmup, a.steps), **counts(e))
        out["best_effort_fit_only"] = dict(timed(e, lambda: e.preempt_dry_run(rows), a.warmup, a.steps), **counts(e))
    for name in ("mode_enabled", "mode_disabled"):
        out[name]["ratio_to_fit_only"] = round(out[name]["median_ms"] / out["fit_only"]["median_ms"], 3)
    out["best_effort"]["ratio_to_fit_only"] = round(out["best_effort"]["median_ms"] / out["best_effort_fit_only"]["median_ms"], 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
