"""The sequential preemption loop of PreemptionToleration as the literal loop: test infrastructure, nothing of the
product.  For every row, in list order, ptol_oracle.dry_run for that one preemptor on a mutable copy of the model, then the scheduler's
cache once the events of the step have been observed, applied to the dicts:

    T1  the victims of the picked cell leave the node                        NodeInfo.RemovePod
    T2  the preemptor becomes a pod nominated to the picked node             the nominator's AddNominatedPod
    T3  nominated pods of that node with a lower priority lose theirs        prepareCandidate / getLowerPriorityNominatedPods
    T4  a nomination the preemptor came with is dropped, wherever it was     the nominator moves it, or clears it without a candidate

(restated from upstream kube-scheduler, unpinned by a reference test).  PDB budgets stay as the model has them.  Two kinds of row
apply nothing: a PreemptNever row, which upstream never lets into PostFilter's preemption, is answered on the untouched model (what the
batch dry run gives for it); a row that is not eligible is evaluated at its own step like any other and its pick is reported.  Nothing
here knows the device's overlay: pods are deleted from lists, nominations are list entries.

Victim positions are reported as positions in the node's list as the model has it, whatever left the node before.
"""
from __future__ import annotations

import ptol_oracle as TO


def mutable_copy(snap):
    """the model with node lists of its own; "at" = position of each remaining pod in the model's list"""
    nodes = [dict(n, pods=list(n["pods"]), nominated=list(n["nominated"]), at=list(range(len(n["pods"])))) for n in snap["nodes"]]
    return dict(snap, nodes=nodes)


def apply_step(state, pre, node, victims, counters):
    """T1-T4 for the preemptor `pre` whose pick is `node` (-1 = no candidate) with `victims` (positions in the node's current list)"""
    for nd in state["nodes"]:  # T4
        mine = [p for p in nd["nominated"] if p["row"] == pre["row"]]
        if mine:
            nd["nominated"] = [p for p in nd["nominated"] if p["row"] != pre["row"]]
            counters["t4_moved" if node >= 0 else "t4_dropped"] += len(mine)
    if node < 0:
        return
    nd = state["nodes"][node]
    gone = set(victims)
    nd["pods"] = [p for k, p in enumerate(nd["pods"]) if k not in gone]  # T1
    nd["at"] = [a for k, a in enumerate(nd["at"]) if k not in gone]
    lower = [p for p in nd["nominated"] if p["prio"] < pre["prio"]]  # T3
    nd["nominated"] = [p for p in nd["nominated"] if p["prio"] >= pre["prio"]]
    counters["t3_cleared"] += len(lower)
    nd["nominated"].append({"key": pre["key"], "prio": pre["prio"], "row": pre["row"], "fit": pre["fit"]})  # T2


def run(snap, preemptors, node_mask=None, eligible=None, counters=None):
    """-> per preemptor what ptol_oracle.dry_run gives for it at its own step, the victims of every cell as positions in the model's
    lists; counters: a dict that receives "t3_cleared", "t4_moved", "t4_dropped" and "applied" """
    state = mutable_copy(snap)
    counters = {} if counters is None else counters
    counters.update(t3_cleared=0, t4_moved=0, t4_dropped=0, applied=0)
    out = []
    for i, pre in enumerate(preemptors):
        mask = None if node_mask is None else [node_mask[i]]
        if pre["never"]:
            out.append(TO.dry_run(snap, [pre], mask)[0])
            continue
        got = TO.dry_run(state, [pre], mask)[0]
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
