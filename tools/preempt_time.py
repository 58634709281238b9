"""The preemption dry run at a realistic size, beside the literal Python oracle on the same host.

A seeded snapshot (synth.preempt_model) goes through the object builders and the flatteners to the device; each timed step runs
spx_preempt_dry_run for all preemptors x all nodes (row records, cells, pick; the per-snapshot marks are part of the first step only)
and spx_last_eval_ms of that call is reported (median, min, max).  The oracle (tests/preempt_oracle.py: SelectVictimsOnNode cell by
cell, with a clone of the quotas per cell) is timed on a slice of the preemptors and scaled to all of them.

    python tools/preempt_time.py [--nodes 10000] [--pods-per-node 30] [--preemptors 1024] [--steps 10] [--warmup 2] [--oracle-rows 2] [--out FILE.json]

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
sys.path.insert(0, str(ROOT / "tests"))

import preempt_oracle as PO  # noqa: E402
import scheduler_plugins_amd as spx  # noqa: E402
from scheduler_plugins_amd import objects, synth  # noqa: E402
from scheduler_plugins_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--pods-per-node", type=float, default=30.0)
    ap.add_argument("--preemptors", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--oracle-rows", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    say = lambda *x: print(*x, file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    model = synth.preempt_model(a.nodes, a.preemptors, seed=41, pods_per_node=a.pods_per_node)
    say(f"model drawn in {time.perf_counter() - t0:.1f} s")
    t0 = time.perf_counter()
    tables = objects.build_preempt_tables(spx.header(), model)
    say(f"object tables built in {time.perf_counter() - t0:.1f} s")
    out = {"shape": {"nodes": a.nodes, "preemptors": a.preemptors, "assigned_pods": len(tables["assigned_at"])}, "steps": a.steps, "warmup": a.warmup}
    with Engine(0) as e:
        t0 = time.perf_counter()
        f = e.load_preempt_objects(tables)
        out["flatten_and_upload_s"] = time.perf_counter() - t0
        out["shape"].update(pdb_budgets=int(f["pdb_ptr"][-1]), nominated=int(f["nom_ptr"][-1]), longest_list=int(np.diff(f["pod_ptr"]).max()))
        rows, ms = np.arange(a.preemptors), []
        for i in range(a.warmup + a.steps):
            e.preempt_dry_run(rows)
            e.sync()
            if i >= a.warmup:
                ms.append(e.last_eval_ms())
        out["dry_run_ms"], out["dry_run_min_max_ms"] = statistics.median(ms), [min(ms), max(ms)]
        out["cell_record_bytes"] = int(a.nodes * ((a.preemptors + 63) // 64 * 64) * 32)
        st, _, _ = e.preempt_cells(0, min(64, a.preemptors))
        out["status_counts_first_rows"] = np.bincount(st.ravel(), minlength=7).tolist()
        out["rows_with_a_pick"] = int((e.preempt_pick()["node"] >= 0).sum())
    sample = model["pending"][:: max(1, a.preemptors // max(1, a.oracle_rows))][: a.oracle_rows]
    t0 = time.perf_counter()
    PO.dry_run(model, sample)
    dt = time.perf_counter() - t0
    out["oracle"] = {"rows_timed": len(sample), "seconds_timed": dt, "seconds_scaled_to_all": dt * a.preemptors / max(1, len(sample))}
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
