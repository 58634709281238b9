"""NodeMetadata's and PodState's sweeps beside Allocatable's at the headline shape, in one process on one device (event times).

Without a Filter in play all three write the same bytes: one normalised row broadcast into every pod row, 1 B per cell.  The new
broadcast (k_node_broadcast) is set beside Allocatable's own table write — mask ALLOCATABLE alone, SPX_OPT_ALLOC_TABLE_KEEP off —
and is asked to take, by its median run, no more than Allocatable's slowest run.  With a caller's feasibility mask in play the
per-row pass (k_node_rows) is set beside Allocatable's (k_alloc_masked) at the same mask density: reported, not gated (the new
kernel reads 8 B of raw score per node where Allocatable's compact path reads 4 B).  The legs are timed alternately, three runs each,
a run being the median of --steps steady steps.

    python tools/node_columns_time.py [--nodes 10000] [--pods 100000] [--steps 20] [--warmup 5] [--runs 3] [--density 0.5] [--no-mask] [--out FILE.json]

Prints one JSON line; exit status 1 when a broadcast median is above Allocatable's slowest run."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import scheduler_plugins_amd as spx  # noqa: E402
from scheduler_plugins_amd import synth  # noqa: E402
from scheduler_plugins_amd.engine import ALLOCATABLE, NODEMETA, PODSTATE, Engine, mask_of  # noqa: E402

LEGS = (("allocatable", ALLOCATABLE), ("nodemeta", NODEMETA), ("podstate", PODSTATE))


def run(e, mask, steps, warmup):
    out = []
    for i in range(warmup + steps):
        e.eval(mask)
        e.sync()
        if i >= warmup:
            out.append(e.last_eval_ms())
    return statistics.median(out) if out else None


def legs(e, a):
    """{leg: [median of run 1, run 2, ...]}, the legs alternating inside every run"""
    for _, p in LEGS:
        run(e, mask_of(p), 0, a.warmup)
    res = {name: [] for name, _ in LEGS}
    for _ in range(a.runs):
        for name, p in LEGS:
            res[name].append(round(run(e, mask_of(p), a.steps, 1), 4))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--pods", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--no-mask", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    hdr = spx.header()
    tri = synth.trimaran_snapshot(hdr, a.nodes, a.pods, seed=synth.SEED, round_frac=0.1)
    cols = synth.node_column_snapshot(a.nodes, seed=synth.SEED)
    res = {"shape": [a.nodes, a.pods], "steps": a.steps, "warmup": a.warmup, "runs": a.runs}
    with Engine(0) as e:
        e.set_option("ALLOC_TABLE_KEEP", 0)  # Allocatable's sweep writes its table in every step
        e.load_trimaran_objects(tri["nodes"], tri["rc"], tri["pods"], tri["metrics"], tri["assigned"])
        e.upload_nodemeta(cols["nodemeta"])
        e.upload_podstate(cols["podstate"])
        res["table_bytes"] = e.score_table(NODEMETA)[1] * a.pods
        res["broadcast_ms"] = legs(e, a)
        slowest = max(res["broadcast_ms"]["allocatable"])
        res["broadcast_gate"] = {k: ("ok" if statistics.median(res["broadcast_ms"][k]) <= slowest else "above Allocatable's slowest run") for k in ("nodemeta", "podstate")}
        if not a.no_mask:
            rng = np.random.default_rng(1)
            mask = (rng.random((a.pods, a.nodes), dtype=np.float32) < a.density).astype(np.uint8)
            e.upload_feasible_mask(mask)
            del mask
            res["mask_density"] = a.density
            res["masked_ms"] = legs(e, a)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0 if all(v == "ok" for v in res["broadcast_gate"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
