"""Times NodeResourceTopologyMatch's tall-node kernel (kernels_nrt_tall.hip) beside the long-row kernel, one box, one run.

Shape: config #3's (5 000 nodes x 50 000 pods) with 1 % of the nodes tall at 16 zones, and 3 % of the pods long (so that k_nrt_long
runs in the same session).  Per strategy (LeastAllocated, LeastNUMANodes) a whole-batch sweep of
  plain  the snapshot with the tall nodes' NRT objects removed (the control: what the dense path costs alone)
  tall   the snapshot with its tall nodes
Prints the median event time of --reps sweeps per leg, the work of the two side kernels (tall: zone-container cells = containers
of the batch x zones of the tall nodes; long: container cells = containers of the long rows x nodes) and one JSON line.  The event
times hold the dense sweep too; for the device time of k_nrt_tall and k_nrt_long per launch run it under a kernel trace, with no
counters in the same run:
`rocprofv3 --kernel-trace --stats -- python tools/nrt_tall_timing.py`."""
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


def leg(snap, params, reps: int, n_tall: int):
    """(median eval ms, long rows) of whole-batch sweeps through spx_load_nrt's tables"""
    with Engine(0) as e:
        e.load_c(snap, params)
        e.eval(mask_of(NRT))  # warm-up
        e.sync()
        ms = []
        for _ in range(reps):
            e.eval(mask_of(NRT))
            e.sync()
            ms.append(e.last_eval_ms())
        assert e.nrt_tall_nodes() == n_tall
        return float(np.median(ms)), e.nrt_long_rows()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--pods", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tall-frac", type=float, default=0.01)
    ap.add_argument("--zones", type=int, default=16)
    ap.add_argument("--long-frac", type=float, default=0.03)
    args = ap.parse_args()
    hdr = spx.header()
    kw = dict(seed=synth.SEED, long_frac=args.long_frac, tall_frac=args.tall_frac, tall_zones=(args.zones, args.zones))
    tall = synth.nrt_snapshot(hdr, args.nodes, args.pods, **kw)
    plain = synth.nrt_snapshot(hdr, args.nodes, args.pods, tall_control=True, **kw)
    zp = tall["nrt"].array("zone_ptr")
    cnt = zp[1:] - zp[:-1]
    n_tall = int((cnt > 8).sum())
    cp = tall["pods"].array("ctr_ptr")
    per_pod = cp[1:] - cp[:-1]
    out = {"nodes": args.nodes, "pods": args.pods, "tall_nodes": n_tall, "zones": args.zones, "containers": int(per_pod.sum()),
           "long_rows": int((per_pod > 8).sum()), "long_containers": int(per_pod[per_pod > 8].sum())}
    out["tall_zone_container_cells"] = out["containers"] * int(cnt[cnt > 8].sum())
    out["long_container_cells"] = out["long_containers"] * args.nodes
    for strategy in ("LeastAllocated", "LeastNUMANodes"):
        params = O.nrt_params(hdr, O.Resources(), strategy)
        p_ms, n_long = leg(plain, params, args.reps, 0)
        t_ms, _ = leg(tall, params, args.reps, n_tall)
        assert n_long == out["long_rows"]
        out[strategy] = {"plain_ms": p_ms, "tall_ms": t_ms, "tall_minus_plain_ms": t_ms - p_ms}
        print(f"{strategy:16s} plain {p_ms:9.3f} ms   tall {t_ms:9.3f} ms   difference {t_ms - p_ms:9.3f} ms", flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
