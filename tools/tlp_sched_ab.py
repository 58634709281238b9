"""SPX_OPT_TLP_CHUNK_SCHED on and off in one process: config #2's steady-state step (Allocatable + TargetLoadPacking, whole batch; the
class form with Allocatable's table kept) on two engines that hold the same snapshot, one whose order was built with the chunk schedule
and one in value order, timed alternately — `steps` evaluations on one, then on the other, `rounds` times — so that whatever else runs
on the machine hits both alike.  On a build without the option (an older tree) one engine is timed the same way.

    python tools/tlp_sched_ab.py [--nodes 10000] [--pods 100000] [--rounds 6] [--steps 50] [--warmup 20] [--out FILE.json]

Prints one JSON line: per engine the median of spx_last_eval_ms of every round, and the median / min / max over all steps."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import scheduler_plugins_amd as spx  # noqa: E402
from scheduler_plugins_amd import synth  # noqa: E402
from scheduler_plugins_amd.engine import ALLOCATABLE, TLP, Engine, mask_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--pods", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    hdr = spx.header()
    snap = synth.trimaran_snapshot(hdr, a.nodes, a.pods, seed=synth.SEED)
    mask = mask_of(ALLOCATABLE, TLP)
    variants = [("chunk_sched_1", 1), ("chunk_sched_0", 0)] if "SPX_OPT_TLP_CHUNK_SCHED" in hdr.consts else [("no_option", None)]
    engines, res = [], {"shape": [a.nodes, a.pods], "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup, "variants": {}}
    try:
        for name, opt in variants:
            e = Engine(0)
            engines.append(e)
            if opt is not None:
                e.set_option("TLP_CHUNK_SCHED", opt)  # read when the order is built, i.e. by the load below
            e.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])
            for _ in range(a.warmup):
                e.eval(mask)
            e.sync()
            res["variants"][name] = {"form": e.tlp_form(), "rows_evaluated": e.tlp_pod_classes()[0], "round_medians": [], "all": []}
        for _ in range(a.rounds):
            for (name, _), e in zip(variants, engines):
                ms = []
                for _ in range(a.steps):
                    e.eval(mask)
                    e.sync()
                    ms.append(e.last_eval_ms())
                res["variants"][name]["round_medians"].append(statistics.median(ms))
                res["variants"][name]["all"] += ms
        for v in res["variants"].values():
            ms = v.pop("all")
            v.update(median=statistics.median(ms), min=min(ms), max=max(ms))
    finally:
        for e in engines:
            e.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
