"""Inputs of tools/micro/wcls.hip: the value-sorted row order of config #2's pod batch and the value at each position, as
np.argsort(kind="stable") of the engine's flattened tlp_pod_milli gives them (host only: no GPU needed).

    python tools/wcls_inputs.py OUT [--nodes 10000] [--pods 100000]

File: int64 rows | int32 order[rows] | int64 value[rows]."""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import ctypes as C  # noqa: E402

import scheduler_plugins_amd as spx  # noqa: E402
from scheduler_plugins_amd import synth  # noqa: E402
from scheduler_plugins_amd.objects import Table  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--pods", type=int, default=100_000)
    a = ap.parse_args()
    hdr = spx.header()
    snap = synth.trimaran_snapshot(hdr, a.nodes, a.pods, seed=synth.SEED)
    # the engine's defaults (engine.py); the flattener is host code, so no engine — and no GPU — is needed
    params = Table(hdr, "spx_tlp_params", target_utilization=40, default_requests_milli=1000, requests_multiplier=1.5)
    cols = [np.zeros(a.pods, np.int64) for _ in range(3)]  # tlp_pod_milli, lv_req_cpu_milli, lv_req_mem
    rc = spx.lib().spx_flatten_trimaran_pods(snap["pods"].ref(), params.ref(), *[c.ctypes.data_as(C.POINTER(C.c_int64)) for c in cols])
    if rc != 0:
        raise SystemExit(f"spx_flatten_trimaran_pods: {rc}")
    v = cols[0]
    order = np.argsort(v, kind="stable").astype(np.int32)
    with open(a.out, "wb") as f:
        np.array([len(v)], np.int64).tofile(f)
        order.tofile(f)
        v[order].astype(np.int64).tofile(f)
    p = np.arange(len(v))
    s = v[order]
    print(f"{len(v)} rows, {len(np.unique(v))} distinct values, {int(((p % 64 == 0) | (s != np.roll(s, 1))).sum())} evaluated")


if __name__ == "__main__":
    main()
