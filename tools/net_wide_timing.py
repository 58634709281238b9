"""Times NetworkOverhead's 64-bit sweep (kernels_network_wide.hip) against the 32-bit one, one box, one run.

Legs, each a whole-batch sweep of config #4's shape (10 000 nodes x 200 000 pods):
  narrow     k_net_cls on the snapshot as synthesised
  wide31     k_net_cls_wide on the same snapshot with every cost shifted left by 31 bits (kernel_path 2)
  wide_same  k_net_cls_wide on the unshifted values uploaded as int64 tables (the same arithmetic work as `narrow`)
Prints the median event time of --reps sweeps per leg and one JSON line.  For per-kernel device times run it under
`rocprofv3 --kernel-trace --stats -- python tools/net_wide_timing.py`."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

import scheduler_plugins_amd as spx  # noqa: E402
from scheduler_plugins_amd import synth  # noqa: E402
from scheduler_plugins_amd.engine import NETOVERHEAD, Engine, mask_of  # noqa: E402


def leg(snap, reps: int, as_int64: bool, expect_path: int) -> float:
    with Engine(0) as e:
        f = e.flatten_network(snap["nodes"], snap["pods"], snap["appgroups"], snap["nettopo"])
        if as_int64:
            f = dict(f, rcost=f["rcost"].astype(np.int64), zcost=f["zcost"].astype(np.int64))
        e.upload_network(f)
        assert e.kernel_path(NETOVERHEAD) == expect_path
        e.eval(mask_of(NETOVERHEAD))  # warm-up
        e.sync()
        ms = []
        for _ in range(reps):
            e.eval(mask_of(NETOVERHEAD))
            e.sync()
            ms.append(e.last_eval_ms())
        return float(np.median(ms))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--pods", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    hdr = spx.header()
    plain = synth.network_snapshot(hdr, args.nodes, args.pods)
    shifted = synth.network_snapshot(hdr, args.nodes, args.pods)
    for col in ("rc_cost", "zc_cost"):
        c = shifted["nettopo"].array(col)
        c[:] = (c << 31) + c % 7
    d = shifted["appgroups"].array("dep_max_cost")
    d[:] = (d << 31) + 6
    out = {"narrow_ms": leg(plain, args.reps, False, 1), "wide31_ms": leg(shifted, args.reps, False, 2), "wide_same_ms": leg(plain, args.reps, True, 2)}
    out["wide31_over_narrow"] = out["wide31_ms"] / out["narrow_ms"]
    out["wide_same_over_narrow"] = out["wide_same_ms"] / out["narrow_ms"]
    for k, v in out.items():
        print(f"{k:24s} {v:9.3f}", flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
