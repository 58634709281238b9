#!/usr/bin/env python3
"""The launch sequence of the evaluation paths as evidence: a fixed list of engine calls on a seeded 70 x 300 snapshot, and the
comparison of two kernel traces of it (profiles/eval_stages/ab.md).
  calls:    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/variant.py run <name> tools/eval_stages.py calls
  compare:  python tools/eval_stages.py compare DIR_A DIR_B      (prints the summary; exit 1 when the ordered lists differ)"""
import csv
import sys
from pathlib import Path


def calls():
    import scheduler_plugins_amd as spx
    from scheduler_plugins_amd import objects as O
    from scheduler_plugins_amd import synth
    from scheduler_plugins_amd.engine import ALLOCATABLE, CAPACITY, LROC, LVRB, NETOVERHEAD, NRT, PEAKS, SYSCHED, TLP, Engine, mask_of

    hdr = spx.header()
    n_nodes, n_pods, seed = 70, 300, 5  # 300 rows: TargetLoadPacking's class form applies from 256
    s = synth.full_snapshot(hdr, n_nodes, n_pods, seed=seed, pods_per_group=50, n_namespaces=20)
    full = mask_of(ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD, CAPACITY, LROC, PEAKS)
    config2 = mask_of(ALLOCATABLE, TLP)
    with Engine(0) as e:
        e.load_c(s, O.nrt_params(hdr, O.Resources(), "LeastAllocated"))
        e.load_lroc_objects(s["nodes"], synth.synth_node_pods(hdr, n_nodes, seed), s["pods"])
        e.load_peaks_objects(s["nodes"], s["metrics"], synth.synth_power_models(hdr, n_nodes, seed), s["pods"])
        e.load_sysched_objects(synth.sysched_snapshot(hdr, n_nodes, n_pods, seed=seed)["objects"])
        e.eval(full)
        e.eval(config2)
        e.eval(config2)  # the second keeps Allocatable's table
        assert e._lib.spx_alloc_table_path(e._h) == 2
        e.eval(mask_of(NRT, PEAKS, SYSCHED))
        e.eval(mask_of(SYSCHED))
        e.decide(full)  # with Filter plugins
        e.decide(mask_of(ALLOCATABLE, TLP, LVRB, PEAKS))
        e.commit_sequential(full, 0, 8)
        for p in (ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD, PEAKS, SYSCHED):
            e.raw(p, 7)
        e.sync()


def dispatches(directory):
    files = sorted(Path(directory).rglob("*kernel_trace.csv"))
    if len(files) != 1:
        sys.exit(f"{directory}: expected one kernel trace, found {len(files)}")
    with open(files[0], newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"), tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ")) for r in rows]


def compare(dir_a, dir_b):
    a, b = dispatches(dir_a), dispatches(dir_b)
    print(f"{len(a)} dispatches in {dir_a}, {len(b)} in {dir_b}, {len({d[0] for d in a})} distinct kernels")
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
    if first is None and len(a) == len(b):
        print("ordered (kernel, grid, workgroup) lists: identical")
        return 0
    i = min(len(a), len(b)) if first is None else first
    print(f"first difference at dispatch {i}:\n  {a[i] if i < len(a) else None}\n  {b[i] if i < len(b) else None}")
    return 1


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "calls":
        calls()
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
