"""CapacityScheduling's sequential preemption loop with NRT's Filter in the refit at a realistic size, beside the fit-only loop and the
frozen NRT dry run on the same upload.

tools/preempt_nrt_time.py's snapshot (synth.preempt_model, seed 41, quotas on, decorated with containers, two NUMA zones per node and
placement info by tests/ptol_nrt_cases.decorate) goes through the object builders and the flatteners to the device.  Each timed step runs
one entry point for all preemptors and spx_last_eval_ms of that call is reported (median, min, max over --steps runs after --warmup), in
one process:

    nrt_dry_run       spx_preempt_nrt_dry_run, preemption mode on: the frozen batch
    fit_only_loop     spx_preempt_sequential
    loop              spx_preempt_nrt_sequential, preemption mode on
    loop_mode_off     the same, preemption mode off (the ordinary Filter on the uploaded table at every step)

Neither loop sweeps ahead, so a loop's time per step is its whole time over the rows: the row record, the marks, the column, the pick
and the apply.  With each entry go its rows with a pick, the distinct nodes picked and the victims, and with `loop` the rows whose node
differs from the three other runs'.

    python tools/preempt_nrt_seq_time.py [--nodes 10000] [--pods-per-node 30] [--preemptors 1024] [--steps 10] [--warmup 2] [--out FILE.json]

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

    def picks(e):
        pick = e.preempt_pick()
        on = pick["node"] >= 0
        return pick["node"].copy(), dict(rows_with_a_pick=int(on.sum()), distinct_picked_nodes=int(len(set(pick["node"][on].tolist()))), victims=int(pick["n_victims"].sum()))

    with Engine(0) as e:
        f = CC.load(e, t)
        g = f["nrt"]
        out["shape"].update(assigned_pods=int(f["pod_ptr"][-1]), longest_list=int(np.diff(f["pod_ptr"]).max()), nominated_records=int(f["nom_ptr"][-1]), slots=g["R"],
                            zones_per_node=2, nodes_with_nrt=int((g["node_flags"] & 1).astype(bool).sum()), nodes_simulating=int((g["node_flags"] & 16).astype(bool).sum()))
        runs = {"nrt_dry_run": lambda: e.preempt_nrt_dry_run(rows, None, True),
                "fit_only_loop": lambda: e.preempt_sequential(rows),
                "loop": lambda: e.preempt_nrt_sequential(rows, None, None, True),
                "loop_mode_off": lambda: e.preempt_nrt_sequential(rows, None, None, False)}
        node = {}
        for name, step in runs.items():
            out[name] = timed(e, step, a.warmup, a.steps)
            node[name], counts = picks(e)
            out[name].update(counts)
            if name != "nrt_dry_run":
                out[name]["us_per_step"] = out[name]["median_ms"] * 1e3 / a.preemptors
            say(name, json.dumps(out[name]))
        for other in ("nrt_dry_run", "fit_only_loop", "loop_mode_off"):
            out["loop"]["rows_whose_node_differs_from_" + other] = int((node["loop"] != node[other]).sum())
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
