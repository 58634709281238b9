"""Times NodeResourceTopologyMatch's wide kernel (kernels_nrt_wide.hip) against the reference-arithmetic kernel, one box, one run.

Legs, each a whole-batch LeastAllocated sweep of config #3's shape (5 000 nodes x 50 000 pods):
  ref4   the dense reference-arithmetic kernel (SPX_OPT_REFERENCE_KERNELS) on the 4-slot snapshot
  wide4  k_nrt_wide (SPX_OPT_NRT_WIDE) on the same snapshot
  wide12 k_nrt_wide on a 12-slot variant (synth.nrt_snapshot(extra_res=8))
Prints the median event time of --reps sweeps per leg and one JSON line.  For per-kernel device times run it under
`rocprofv3 --kernel-trace --stats -- python tools/nrt_wide_timing.py`."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

import scheduler_plugins_amd as spx  # noqa: E402
from scheduler_plugins_amd import objects as O  # noqa: E402
from scheduler_plugins_amd import synth  # noqa: E402
from scheduler_plugins_amd.engine import NRT, Engine, mask_of  # noqa: E402


def leg(snap, params, wide: bool, reference: bool, reps: int, expect_wide: bool) -> float:
    """median eval time; `wide` sets SPX_OPT_NRT_WIDE, `expect_wide` is the route the load must have taken"""
    with Engine(0) as e:
        if wide:
            e.set_option("NRT_WIDE", 1)
        e.load_c(snap, params)
        if reference:
            e.force_reference_kernels(NRT)
        e.eval(mask_of(NRT))  # warm-up
        e.sync()
        ms = []
        for _ in range(reps):
            e.eval(mask_of(NRT))
            e.sync()
            ms.append(e.last_eval_ms())
        assert e.nrt_wide() == expect_wide
        return float(np.median(ms))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--pods", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    hdr = spx.header()
    params = O.nrt_params(hdr, O.Resources(), "LeastAllocated")
    s4 = synth.nrt_snapshot(hdr, args.nodes, args.pods, seed=synth.SEED)
    s12 = synth.nrt_snapshot(hdr, args.nodes, args.pods, seed=synth.SEED, extra_res=8)
    out = {"ref4_ms": leg(s4, params, False, True, args.reps, False), "wide4_ms": leg(s4, params, True, False, args.reps, True),
           "wide12_ms": leg(s12, params, False, False, args.reps, True)}
    out["wide4_over_ref4"] = out["wide4_ms"] / out["ref4_ms"]
    out["wide12_over_wide4"] = out["wide12_ms"] / out["wide4_ms"]
    for k, v in out.items():
        print(f"{k:20s} {v:9.3f}", flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
