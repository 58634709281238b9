"""TargetLoadPacking's class form (SPX_OPT_TLP_POD_CLASSES) beside the plain form, on batches whose share of copied rows is controlled.

The batch is config #2's pod column with a fraction of the rows replaced by values no other row has (drawn from the unused values
inside the ambiguity table, so that the replaced rows still take the streamlined cell); per fraction the sweep of TLP alone — the
steady-state step of the headline — is timed in both forms, alternately, on one engine: option 0 (plain) and option 2 (the class form
whenever a row is a copy).  Reported per fraction: rows evaluated / copied, the share of copies, median and min–max of
spx_last_eval_ms of both forms.  --upload-only times spx_upload_trimaran_pods alone (wall clock; the call ends in a stream
synchronise) and touches nothing a build without the option lacks, so the same command measures the cost of building the order
against an older build.

    python tools/tlp_classes_ab.py [--nodes 10000] [--pods 100000] [--fractions 0,0.25,0.5,0.75,1] [--steps 30] [--warmup 5] [--out FILE.json]

Prints one JSON line."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import scheduler_plugins_amd as spx  # noqa: E402
from scheduler_plugins_amd import synth  # noqa: E402
from scheduler_plugins_amd.engine import TLP, Engine, mask_of  # noqa: E402

AMB_SIZE = 1 << 16


def with_unique(values, fraction, rng):
    """`fraction` of the rows get a value of their own; as many as there are unused values inside the table"""
    v = values.copy()
    n = int(round(fraction * len(v)))
    if n == 0:
        return v
    rows = rng.permutation(len(v))[:n]
    keep = np.ones(len(v), bool)
    keep[rows] = False
    free = np.setdiff1d(np.arange(1, AMB_SIZE, dtype=np.int64), v[keep])
    rows = rows[:len(free)]
    v[rows] = rng.permutation(free)[:len(rows)]
    return v


def timed(e, option, steps):
    e.set_option("TLP_POD_CLASSES", option)
    out = []
    for _ in range(steps):
        e.eval(mask_of(TLP))
        e.sync()
        out.append(e.last_eval_ms())
    return out, e.tlp_form()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--pods", type=int, default=100_000)
    ap.add_argument("--fractions", default="0,0.25,0.5,0.75,1")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--upload-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    hdr = spx.header()
    snap = synth.trimaran_snapshot(hdr, a.nodes, a.pods, seed=synth.SEED)
    rng = np.random.default_rng(10)
    res = {"shape": [a.nodes, a.pods], "steps": a.steps, "warmup": a.warmup}
    with Engine(0) as e:
        e.load_trimaran_objects(snap["nodes"], snap["rc"], snap["pods"], snap["metrics"], snap["assigned"])
        cols = e.flatten_trimaran_pods(snap["pods"])
        base = cols["tlp_pod_milli"].copy()
        ups = []
        for _ in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            e.upload_trimaran_pods(cols)
            ups.append((time.perf_counter() - t0) * 1e3)
        ups = ups[a.warmup:]
        res["upload_ms"] = {"median": statistics.median(ups), "min": min(ups), "max": max(ups)}
        if not a.upload_only:
            res["curve"] = []
            for f in (float(x) for x in a.fractions.split(",")):
                cols["tlp_pod_milli"] = with_unique(base, f, rng)
                e.upload_trimaran_pods(cols)
                ev, cp = e.tlp_pod_classes()
                timed(e, 0, a.warmup)
                timed(e, 2, a.warmup)
                plain, cls, form = [], [], 0
                for _ in range(a.steps):  # alternating: what else runs on the machine hits both alike
                    plain += timed(e, 0, 1)[0]
                    got, form = timed(e, 2, 1)
                    cls += got
                res["curve"].append({"unique_fraction": f, "distinct": int(len(np.unique(cols["tlp_pod_milli"]))), "rows_evaluated": ev, "rows_copied": cp,
                                     "copy_share": cp / a.pods, "form_at_2": form,
                                     "plain_ms": {"median": statistics.median(plain), "min": min(plain), "max": max(plain)},
                                     "classes_ms": {"median": statistics.median(cls), "min": min(cls), "max": max(cls)}})
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
