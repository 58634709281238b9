"""Coscheduling's PreFilter gate at a realistic size, beside the literal Python oracle on the same host.

The gate (scan, both gate kernels, the pods' status bytes) is per snapshot: every upload makes it stale, so each timed step uploads
the tables again and evaluates the COSCHED bit alone; spx_last_eval_ms of that evaluation is reported (median, min, max).  The
oracle (tests/cosched_oracle.py: CheckClusterResource node by node with a clone per node) is timed on a sample of the groups that
reach the resource check and scaled to all of them.

    python tools/cosched_time.py [--nodes 20000] [--groups 4096] [--walk-frac 0.25] [--steps 10] [--warmup 2] [--oracle-groups 48] [--out FILE.json]

Prints one JSON line.  A number to improve on, not a gate."""
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

import cosched_cases as CC  # noqa: E402
import cosched_oracle as CO  # noqa: E402
import scheduler_plugins_amd as spx  # noqa: E402
from scheduler_plugins_amd.engine import COSCHED, Engine, mask_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=20_000)
    ap.add_argument("--groups", type=int, default=4096)
    ap.add_argument("--walk-frac", type=float, default=0.25)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--oracle-groups", type=int, default=48)
    ap.add_argument("--out")
    a = ap.parse_args()
    hdr = spx.header()
    snap = CC.draw_snapshot(seed=31, n_nodes=a.nodes, n_groups=a.groups, n_walk=int(a.groups * a.walk_frac))
    res_names, nodes, objects = CC.build(hdr, snap)
    out = {"shape": {"nodes": a.nodes, "groups": a.groups}, "steps": a.steps, "warmup": a.warmup}
    with Engine(0) as e:
        f = e.flatten_cosched(nodes, objects)
        out["shape"].update(pods=f["P"], slots=f["S"], steps_total=int(f["step_ptr"][-1]), groups_with_assigned_pods=int((np.diff(f["step_ptr"]) > 0).sum()))
        ms = []
        for i in range(a.warmup + a.steps):
            e.upload_cosched(f)
            e.eval(mask_of(COSCHED))
            e.sync()
            if i >= a.warmup:
                ms.append(e.last_eval_ms())
        out["gate_ms"], out["gate_min_max_ms"] = statistics.median(ms), [min(ms), max(ms)]
        out["walked"] = e.kernel_path(COSCHED)
        status = e.prefilter(COSCHED)
        out["status_counts"] = np.bincount(status, minlength=5).tolist()
    checked = [g for g in snap["groups"] if g.get("exists", True) and g["min_resources"] is not None]
    sample = checked[:: max(1, len(checked) // max(1, a.oracle_groups))][: a.oracle_groups]
    for n in snap["nodes"]:
        CO.node_resource(n, "nobody/nothing")  # the per-node image is built once per snapshot, outside the timed part
    t0 = time.perf_counter()
    for g in sample:
        CO.check_cluster_resource(snap["nodes"], CO.min_resources_request(g), CC.group_key(g))
    dt = time.perf_counter() - t0
    out["oracle"] = {"groups_timed": len(sample), "groups_checked": len(checked), "seconds_timed": dt, "ms_scaled_to_all": 1e3 * dt * len(checked) / max(1, len(sample))}
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
