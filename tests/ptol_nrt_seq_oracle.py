"""PreemptionToleration's sequential preemption loop with NodeResourceTopologyMatch's Filter in the refit as the
literal loop: test infrastructure, nothing of the product.  It is ptol_seq_oracle.run with the one-preemptor dry run replaced by
ptol_nrt_oracle.dry_run: for every row, in list order, that dry run on a mutable copy of the model, then T1-T4 on the dicts
(ptol_seq_oracle.apply_step).  A PreemptNever row is answered on the untouched model.

T5 needs no line of its own here.  The node's "nrt" and "placement" are never changed (the reference's NRT caches have no pod-delete
path: pkg/noderesourcetopology/cache/passthrough.go, discardreserved.go, overreserve.go), and an evicted pod is deleted from the node's
list, so ptol_nrt_oracle never puts it on the Filter's stack again.  Nothing here knows the device's overlay.
"""
from __future__ import annotations

import ptol_nrt_oracle as NO
from ptol_seq_oracle import apply_step, mutable_copy


def run(snap, preemptors, node_mask=None, eligible=None, mode=True, counters=None):
    """as ptol_seq_oracle.run; mode: NRT's preemption mode"""
    state = mutable_copy(snap)
    counters = {} if counters is None else counters
    counters.update(t3_cleared=0, t4_moved=0, t4_dropped=0, applied=0)
    out = []
    for i, pre in enumerate(preemptors):
        mask = None if node_mask is None else [node_mask[i]]
        if pre["never"]:
            out.append(NO.dry_run(snap, [pre], mask, mode)[0])
            continue
        got = NO.dry_run(state, [pre], mask, mode)[0]
        node = got["pick"][0]
        victims = list(got["cells"][node]["victims"]) if node >= 0 else []
        for nd, c in zip(state["nodes"], got["cells"]):
            c["victims"] = [nd["at"][k] for k in c["victims"]]
        out.append(got)
        if eligible is not None and not eligible[i]:
            continue
        counters["applied"] += 1
        apply_step(state, pre, node, victims, counters)
    return out
