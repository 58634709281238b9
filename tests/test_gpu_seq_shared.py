"""What the two sequential preemption loops (spx_preempt_sequential, spx_preempt_toleration_sequential) share
on the host: the order of their refusals, and the overlay, the row lists' CSR and the pick buffer that one engine carries from a call
of one loop to a call of the other.  The reference of every call is a fresh engine that ran that call alone, at tolerance 0."""
import numpy as np
import pytest

import preempt_cases as PC
import preempt_seq_cases as SC
import preempt_seq_oracle as SO
import scheduler_plugins_amd as spx
from scheduler_plugins_amd import SpxError
from scheduler_plugins_amd.engine import Engine
from test_gpu_preempt_seq import snapshot
from test_gpu_ptol import both_plugins_model

ARG = spx.header().consts["SPX_ERR_ARG"]


def load_both(e, t):
    """one node table with the quota tables, the side table and the toleration table: both loops can be asked"""
    f = e.load_preempt_objects(t)
    e.upload_preempt_toleration(e.flatten_preempt_toleration(t["classes"], t["pod_class"], t["pod_scheduled"], t["pod_scheduled_at_ns"], f["pod_src"]))
    return f


def generated():
    """the generator's model for both plugins, 24 nodes x 66 rows, with one row nominated to two nodes: its step of the toleration loop
    has three dirty nodes at the most, so every step has three slots"""
    m = both_plugins_model(n_nodes=24, n_pending=66, seed=7)
    taken = {p["row"] for nd in m["nodes"] for p in nd["nominated"]}
    r = next(p["row"] for p in m["pending"] if p["row"] not in taken and not p["never"])
    a, b = [n for n, nd in enumerate(m["nodes"]) if nd["present"]][:2]
    for n in (a, b):
        m["nodes"][n]["nominated"].append(dict(m["pending"][r]))
    mask = PC.node_mask(66, 24, 11)
    order = (40, 3, 62, 0, 17, 18, 5, 61, 33, 2, 50, 9)
    calls = [("capacity", np.arange(40), SC.eligible_column(40, 21)), ("toleration", np.arange(66), None), ("capacity", np.array(order), None)]
    return m, mask, calls, r


def hand():
    """SC.HAND's T1 model (P0 evicts xa from namespace X's set, X's Used moves under its min, and P1 finds nothing to borrow back on the
    untouched node B), its row list filled up to 66 with rows of a namespace without quota that find no victim on the empty node C"""
    m, mask, eligible, what = SC.HAND["t1_in_set"]()
    assert what["used_moved"] == 1
    fill = [SC._pod(f"F{i}", 2, 5, 100, row=i) for i in range(2, 66)]
    m["pending"] += fill
    mask = np.concatenate([mask, np.tile(np.array([[0, 0, 1]], np.uint8), (len(fill), 1))])
    for p in [p for nd in m["nodes"] for p in nd["pods"]] + m["pending"]:
        p.update(pc="", scheduled_at=None)
    for p in m["pending"]:
        p["never"] = False
    m["classes"], m["now"] = {}, 0
    counters = {}
    SO.run(m, m["pending"][:34], mask[:34], np.concatenate([eligible, np.ones(32, np.uint8)]), counters)
    assert counters["used_moved"] == 1
    calls = [("capacity", np.arange(34), np.concatenate([eligible, np.ones(32, np.uint8)])), ("toleration", np.arange(66), None), ("capacity", np.arange(2), None)]
    return m, mask, calls, None


def run_call(e, t, mask, call):
    loop, rows, eligible = call
    if loop == "capacity":
        e.preempt_sequential(rows, eligible, mask[rows])
    else:
        e.preempt_toleration_sequential(rows, t["priority"][rows], t["never"][rows], t["now"], eligible, mask[rows])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [generated, hand], ids=lambda c: c.__name__)
def test_one_engine_runs_both_loops_in_turn(gpu_required, case):
    """the capacity loop with k rows and an eligible column, the toleration loop with more rows (past 64: the row stride grows and the
    overlay is carved again), the capacity loop with fewer rows and no eligible column: after every call the picks, the cells, the keys
    and the stored victims of every picked cell are those of a fresh engine that ran the call alone"""
    m, mask, calls, twice = case()
    t = spx.objects.build_preempt_toleration_tables(spx.header(), m)
    assert [c[0] for c in calls] == ["capacity", "toleration", "capacity"] and calls[0][2] is not None and calls[2][2] is None
    assert len(calls[0][1]) <= 64 < len(calls[1][1]) and len(calls[2][1]) < len(calls[0][1])
    alone = []
    for call in calls:
        with Engine(0) as e:
            f = load_both(e, t)
            run_call(e, t, mask, call)
            alone.append(snapshot(e))
    if twice is not None:  # two uploaded nominations of one row, on two nodes
        at = np.flatnonzero(np.asarray(f["nom_pending_row"]) == twice)
        assert len(at) == 2 and len(set(np.searchsorted(np.asarray(f["nom_ptr"]), at, side="right"))) == 2
    assert all(any(n >= 0 for n in s[6]) for s in alone)  # every call picks somewhere
    with Engine(0) as e:
        load_both(e, t)
        for k, call in enumerate(calls):
            run_call(e, t, mask, call)
            assert snapshot(e) == alone[k], k


@pytest.mark.gpu
def test_a_row_past_the_batch_is_refused_before_a_row_listed_twice(gpu_required):
    """[P, 3, 3]: both loops name the row that is no row of the batch, and the results of the run before stay in place"""
    m = both_plugins_model(n_nodes=24, n_pending=66, seed=7)
    t = spx.objects.build_preempt_toleration_tables(spx.header(), m)
    P = len(m["pending"])
    with Engine(0) as e:
        load_both(e, t)
        e.preempt_sequential([0, 1])
        before = snapshot(e)
        for run in (lambda: e.preempt_sequential([P, 3, 3]), lambda: e.preempt_toleration_sequential([P, 3, 3], [5, 5, 5], [0, 0, 0], t["now"])):
            with pytest.raises(SpxError) as err:
                run()
            assert err.value.code == ARG and "rows[0] is no row of the batch" in err.value.msg and "listed twice" not in err.value.msg, err.value
        for run in (lambda: e.preempt_sequential([3, 7, 3]), lambda: e.preempt_toleration_sequential([3, 7, 3], [5, 5, 5], [0, 0, 0], t["now"])):
            with pytest.raises(SpxError) as err:
                run()
            assert err.value.code == ARG and "rows[2] is listed twice" in err.value.msg, err.value
        assert snapshot(e) == before
