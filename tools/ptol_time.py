"""PreemptionToleration's dry run at a realistic size, beside CapacityScheduling's on the same box.

A seeded snapshot (synth.ptol_model: synth.preempt_model without quotas, decorated with PriorityClasses) goes through the object
builders and the flatteners to the device; each timed step runs spx_preempt_toleration_dry_run for all preemptors x all nodes (row
records, cells, pick) and spx_last_eval_ms of that call is reported (median, min, max).  Then the quota'd variant of the same snapshot
(synth.preempt_model with the same seed and shape) is timed the same way through spx_preempt_dry_run, in the same process.

    python tools/ptol_time.py [--nodes 10000] [--pods-per-node 30] [--preemptors 1024] [--steps 10] [--warmup 2] [--out FILE.json]

Prints one JSON line.  A number for the record, not a gate."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import scheduler_plugins_amd as spx  # noqa: E402
from scheduler_plugins_amd import objects, synth  # noqa: E402
from scheduler_plugins_amd.engine import Engine  # noqa: E402


def timed(e, step, warmup, steps):
    ms = []
    for i in range(warmup + steps):
        step()
        e.sync()
        if i >= warmup:
            ms.append(e.last_eval_ms())
    return {"median_ms": statistics.median(ms), "min_max_ms": [min(ms), max(ms)]}


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
    shape = dict(seed=41, pods_per_node=a.pods_per_node)
    rows = np.arange(a.preemptors)
    out = {"shape": {"nodes": a.nodes, "preemptors": a.preemptors}, "steps": a.steps, "warmup": a.warmup}

    t0 = time.perf_counter()
    t = objects.build_preempt_toleration_tables(spx.header(), synth.ptol_model(a.nodes, a.preemptors, **shape))
    say(f"toleration model drawn and object tables built in {time.perf_counter() - t0:.1f} s")
    with Engine(0) as e:  # never sees a quota table
        f = e.load_preempt_toleration_objects(t)
        out["shape"].update(assigned_pods=int(f["pod_ptr"][-1]), longest_list=int(np.diff(f["pod_ptr"]).max()), priority_classes=len(t["class_names"]),
                            pods_with_class=int((f["toleration"]["flags"] != 0).sum()))
        out["toleration"] = timed(e, lambda: e.preempt_toleration_dry_run(rows, t["priority"], t["never"], t["now"]), a.warmup, a.steps)
        st, _, _ = e.preempt_cells(0, min(64, a.preemptors))
        out["toleration"].update(status_counts_first_rows=np.bincount(st.ravel(), minlength=8).tolist(), rows_with_a_pick=int((e.preempt_pick()["node"] >= 0).sum()))
    say(json.dumps(out["toleration"]))

    t0 = time.perf_counter()
    t = objects.build_preempt_tables(spx.header(), synth.preempt_model(a.nodes, a.preemptors, **shape))
    say(f"capacity model drawn and object tables built in {time.perf_counter() - t0:.1f} s")
    with Engine(0) as e:
        e.load_preempt_objects(t)
        out["capacity"] = timed(e, lambda: e.preempt_dry_run(rows), a.warmup, a.steps)
        st, _, _ = e.preempt_cells(0, min(64, a.preemptors))
        out["capacity"].update(status_counts_first_rows=np.bincount(st.ravel(), minlength=8).tolist(), rows_with_a_pick=int((e.preempt_pick()["node"] >= 0).sum()))
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
