"""CapacityScheduling's sequential preemption loop with NodeResourceTopologyMatch's Filter in the refit as the literal
loop: test infrastructure, nothing of the product.  It is preempt_seq_oracle.run with the one-preemptor dry run replaced by
preempt_nrt_oracle.dry_run: for every row, in list order, that dry run on a mutable copy of the model (preempt_seq_oracle.mutable_copy:
the node lists, the quotas' `used` and `pods` sets), then T4, T1, T3 and T2 on the dicts (preempt_seq_oracle.apply_step), counters
included.

T5 needs no line of its own here.  The node's "nrt" and "placement" are never changed (the reference's NRT caches have no pod-delete
path: pkg/noderesourcetopology/cache/passthrough.go, discardreserved.go, overreserve.go), and an evicted pod is deleted from the node's
list, so preempt_nrt_oracle never puts it on the Filter's stack again.  A victim the Filter alone kept leaves its quota through
apply_step like any other.  Nothing here knows the device's overlay.
"""
from __future__ import annotations

import preempt_nrt_oracle as CO
import preempt_oracle as PO
from preempt_seq_oracle import COUNTERS, apply_step, mutable_copy


def run(snap, preemptors, node_mask=None, eligible=None, mode=True, counters=None, frozen=None):
    """as preempt_seq_oracle.run; mode: NRT's preemption mode.  frozen: the batch dry run with the Filter of the same rows on the
    untouched model, for the last two counters"""
    state = mutable_copy(snap)
    counters = {} if counters is None else counters
    counters.update({k: 0 for k in COUNTERS})
    touched = set()
    out = []
    for i, pre in enumerate(preemptors):
        got = CO.dry_run(state, [pre], None if node_mask is None else [node_mask[i]], mode)[0]
        node = got["pick"][0]
        victims = list(got["cells"][node]["victims"]) if node >= 0 else []
        for nd, c in zip(state["nodes"], got["cells"]):
            c["victims"] = [nd["at"][k] for k in c["victims"]]
        out.append(got)
        if frozen is not None:
            if pre["ns"] in state["quotas"]:
                branch = lambda s: PO.used_over_min_with(s["quotas"][pre["ns"]], PO.prefilter_state(s, pre)[0])
                counters["branch_flips"] += branch(state) != branch(snap)
            key = lambda c: (c["status"], c["victims"], c["n_violations"])
            counters["untouched_cells_differ"] += sum(n not in touched and key(a) != key(b) for n, (a, b) in enumerate(zip(got["cells"], frozen[i]["cells"])))
        if eligible is not None and not eligible[i]:
            continue
        counters["applied"] += 1
        apply_step(state, pre, node, victims, counters, touched)
    return out
