"""The sequential preemption loop of CapacityScheduling as the literal loop: test infrastructure, nothing of the
product.  For every row, in list order, preempt_oracle.dry_run for that one preemptor on a mutable copy of the model (the node lists, the
quotas' `used` and `pods` sets), then the scheduler's cache once the events of the step have been observed, applied to the dicts:

    T4  a nomination the preemptor came with is dropped, wherever it was     the nominator moves it, or clears it without a candidate
    T1  the victims of the picked cell leave the node                        NodeInfo.RemovePod; and their quota: deletePodIfPresent
                                                                             (capacity_scheduling.go:778-792, elasticquota.go:172-187)
    T3  nominated pods of that node with a lower priority lose theirs        prepareCandidate / getLowerPriorityNominatedPods
    T2  the preemptor becomes a pod nominated to the picked node             the nominator's AddNominatedPod; it does not enter Used

(restated from upstream kube-scheduler, unpinned by a reference test).  PDB budgets stay as the model has them.  A row that is not
eligible is evaluated at its own step like any other, its pick is reported and nothing is applied.  Nothing here knows the device's
overlay: pods are deleted from lists and sets, nominations are list entries, and PreFilter's sums walk those lists.

Victim positions are reported as positions in the node's list as the model has it, whatever left the node before.
"""
from __future__ import annotations

import preempt_oracle as PO

COUNTERS = ("applied", "used_moved", "over_min_flips", "branch_flips", "t3_cleared", "t4_moved", "t4_dropped", "untouched_cells_differ")


def mutable_copy(snap):
    """the model with node lists, quota `used` and `pods` sets of its own; "at" = position of each remaining pod in the model's list"""
    nodes = [dict(n, pods=list(n["pods"]), nominated=list(n["nominated"]), at=list(range(len(n["pods"])))) for n in snap["nodes"]]
    quotas = {ns: {"min": q["min"], "max": q["max"], "used": PO.resource(q["used"]["v"], q["used"]["p"]), "pods": set(q["pods"])} for ns, q in snap["quotas"].items()}
    return dict(snap, nodes=nodes, quotas=quotas)


def apply_step(state, pre, node, victims, counters, touched):
    """T4, then T1, T3, T2 for the preemptor `pre` whose pick is `node` (-1 = no candidate) with `victims` (positions in the node's
    current list); touched: the nodes whose own lists a step has changed"""
    for n, nd in enumerate(state["nodes"]):  # T4
        mine = [p for p in nd["nominated"] if p["row"] == pre["row"]]
        if mine:
            nd["nominated"] = [p for p in nd["nominated"] if p["row"] != pre["row"]]
            counters["t4_moved" if node >= 0 else "t4_dropped"] += len(mine)
            touched.add(n)
    if node < 0:
        return
    nd = state["nodes"][node]
    touched.add(node)
    quotas = state["quotas"]
    for k in victims:  # T1, the quota side
        p = nd["pods"][k]
        if p["ns"] in quotas:
            eq = quotas[p["ns"]]
            before, over = (list(eq["used"]["v"]), eq["used"]["p"]), PO.used_over_min(eq)
            PO.delete_pod_if_present(eq, p)
            counters["used_moved"] += before != (eq["used"]["v"], eq["used"]["p"])
            counters["over_min_flips"] += over != PO.used_over_min(eq)
    gone = set(victims)
    nd["pods"] = [p for k, p in enumerate(nd["pods"]) if k not in gone]  # T1, the node side
    nd["at"] = [a for k, a in enumerate(nd["at"]) if k not in gone]
    lower = [p for p in nd["nominated"] if p["prio"] < pre["prio"]]  # T3
    nd["nominated"] = [p for p in nd["nominated"] if p["prio"] >= pre["prio"]]
    counters["t3_cleared"] += len(lower)
    nd["nominated"].append({"key": pre["key"], "ns": pre["ns"], "prio": pre["prio"], "row": pre["row"], "fit": pre["fit"], "req": pre["req"]})  # T2


def run(snap, preemptors, node_mask=None, eligible=None, counters=None, frozen=None):
    """-> per preemptor what preempt_oracle.dry_run gives for it at its own step, the victims of every cell as positions in the model's
    lists.  counters: a dict that receives COUNTERS; the last two compare with `frozen`, the batch dry run of the same rows on the
    untouched model: rows whose usedOverMinWith(nominatedPodsReqInEQWithPodReq) differs from the frozen one, and cells on nodes whose
    own lists no earlier step touched that differ all the same"""
    state = mutable_copy(snap)
    counters = {} if counters is None else counters
    counters.update({k: 0 for k in COUNTERS})
    touched = set()
    out = []
    for i, pre in enumerate(preemptors):
        got = PO.dry_run(state, [pre], None if node_mask is None else [node_mask[i]])[0]
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
