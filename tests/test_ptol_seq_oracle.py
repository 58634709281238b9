"""The sequential preemption loop's literal oracle (tests/ptol_seq_oracle.py), on the CPU: what it must agree with, each rule of the
state model seen in a later row's cell of a hand-built model, and how far the loop's answer is from the frozen
batch's on the models the GPU suite uses.  The last test is about the ABI: it needs the library, no GPU."""
import numpy as np
import pytest

import ptol_cases as TC
import ptol_oracle as TO
import ptol_seq_cases as SC
import ptol_seq_oracle as SO
import scheduler_plugins_amd as spx

ST = TO.ST


@pytest.mark.parametrize("name", ["1x1", "63x65", "lists"])
def test_one_row_is_the_dry_run(name):
    m = TC.model(**TC.SHAPES[name])
    mask = TC.node_mask(1, len(m["nodes"]), 5)
    for pre in m["pending"][:12]:
        assert SO.run(m, [pre]) == TO.dry_run(m, [pre])
        assert SO.run(m, [pre], mask) == TO.dry_run(m, [pre], mask)


# ---------------------------------------------------------------------------------------------------------------- the hand-built model
def hand_model():
    """Three nodes with cpu alone (A 2000, B 3000, C 3000 milli) and eight rows, each masked to one node.  P0, P1, X, Z and V apply
    what they find; Y, W1 and W2 are probes (eligible = 0) that only look.  Z and V come with a nomination on C."""
    def pod(key, prio, cpu, row=-1, **more):
        req = {"v": [cpu, 0, 0, 0, 0, 0, 0, 0], "p": 0}
        return dict({"key": key, "ns": 0, "prio": prio, "start": 1000, "fit": [cpu, 0, 0, 1, 0, 0, 0, 0], "req": req, "pdbs": [], "terminating": False, "row": row,
                     "pc": "", "scheduled_at": None}, **more)

    pending = [pod(k, prio, cpu, row=i, never=False) for i, (k, prio, cpu) in enumerate(
        [("P0", 50, 1000), ("P1", 50, 1000), ("X", 50, 2000), ("Y", 10, 500), ("Z", 50, 1000), ("W1", 10, 2000), ("V", 50, 1000), ("W2", 10, 3000)])]
    node = lambda cpu, pods, nominated: {"present": True, "alloc": [cpu, 0, 0, 110, 0, 0, 0, 0], "pods": pods, "nominated": nominated}
    nodes = [node(2000, [pod("a0", 0, 1000), pod("a1", 10, 1000)], []),
             node(3000, [pod("b0", 0, 1000), pod("b1", 5, 500)], [pod("nomB", 20, 1000)]),
             node(3000, [pod("c0", 0, 1000)], [dict(pending[4]), dict(pending[6])])]
    A, B, C = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    mask = np.array([A, A, B, B, B, C, A, C], dtype=np.uint8)
    eligible = np.array([1, 1, 1, 0, 1, 0, 1, 0], dtype=np.uint8)
    return {"n_namespaces": 1, "quotas": {}, "pdbs": [], "nodes": nodes, "pending": pending, "classes": {}, "now": 0}, mask, eligible


def test_each_rule_shows_in_a_later_rows_cell():
    m, mask, eligible = hand_model()
    counters = {}
    seq = SO.run(m, m["pending"], mask, eligible, counters)
    frozen = TO.dry_run(m, m["pending"], mask)
    cell = lambda res, row, node: (res[row]["cells"][node]["status"], res[row]["cells"][node]["victims"])
    A, B, C = 0, 1, 2
    # P0 takes a0 on A (a1 is reprieved) and is nominated there
    assert cell(seq, 0, A) == (ST["CANDIDATE"], [0]) and seq[0]["pick"][0] == A
    # T1 and T2 in P1's cell of A.  a0 is gone and P0's 1000 are charged, so a1 has to leave; with a0 still walked the victims would
    # be [1, 0], without P0's charge the node would have room and everyone would be reprieved.  The frozen batch says a0 again.
    # The victim is position 1 of the node's list as the model has it, although a1 is the only pod left.
    assert cell(seq, 1, A) == (ST["CANDIDATE"], [1])
    assert cell(frozen, 1, A) == (ST["CANDIDATE"], [0])
    # X takes b0 on B; T3 clears nomB (20 < 50).  Y (priority 10) would charge nomB: with it, X's 2000 and Y's 500 do not fit into 3000
    # once b1 is removed (NOT_FIT); without it they do and b1 can stay (ALL_REPRIEVED)
    assert cell(seq, 2, B) == (ST["CANDIDATE"], [0])
    assert cell(seq, 3, B) == (ST["ALL_REPRIEVED"], [])
    # Z came nominated to C and picks B: T4 moves the nomination.  W1 asks for 2000 on C: with c0 removed, V's nomination leaves exactly
    # that; with Z's still charged it would be NOT_FIT, which is what the frozen batch says
    assert cell(seq, 4, B) == (ST["CANDIDATE"], [1]) and seq[4]["pick"][0] == B
    assert cell(seq, 5, C) == (ST["CANDIDATE"], [0])
    assert cell(frozen, 5, C) == (ST["NOT_FIT"], [])
    # V finds no candidate (nothing on A is left to evict): T4's other form drops its nomination on C, and W2's 3000 fit an empty C
    assert seq[6]["pick"][0] == -1 and cell(seq, 6, A) == (ST["NO_VICTIMS"], [])
    assert cell(seq, 7, C) == (ST["CANDIDATE"], [0])
    assert cell(frozen, 7, C) == (ST["NOT_FIT"], [])
    assert counters == {"t3_cleared": 1, "t4_moved": 1, "t4_dropped": 1, "applied": 5}
    # the probes moved nothing: c0 is still there for W2 after W1 found it
    assert seq[5]["pick"][0] == C and seq[7]["pick"][0] == C


def test_a_preempt_never_row_is_answered_on_the_untouched_model():
    m, mask, eligible = hand_model()
    m["pending"][1]["never"] = True
    seq = SO.run(m, m["pending"], mask, eligible)
    assert seq[1] == TO.dry_run(m, [m["pending"][1]], mask[1:2])[0]
    assert seq[1]["cells"][0]["victims"] == [0]  # a0, which P0 has taken already
    assert seq[6]["cells"][0]["status"] == ST["CANDIDATE"]  # and it applied nothing: a1 is still there for V


# ---------------------------------------------------------------------------------------------------------------- the reference models
def test_the_loop_differs_from_the_frozen_batch_on_every_shape():
    """the models as they are, rows in table order: rows that end with another node or other victims, and the three counters"""
    seen = {"t3_cleared": 0, "t4_moved": 0, "t4_dropped": 0}
    for name, kw in TC.SHAPES.items():
        if name == "1x1":
            continue
        seq, counters = SC.expected(**kw)
        differ = SC.differing_rows(seq, TC.expected(**kw))
        print(name, "rows that differ:", differ, counters)
        assert differ >= 1, name
        for k in seen:
            seen[k] += counters[k]
    assert all(v > 0 for v in seen.values()), seen


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_header_declares_the_loop_and_null_arguments_are_refused():
    hdr = spx.header()
    assert "spx_preempt_toleration_sequential" in hdr.protos
    assert len(hdr.protos["spx_preempt_toleration_sequential"][1]) == 8
    assert spx.lib().spx_preempt_toleration_sequential(None, None, 0, None, None, None, 0, None) == hdr.consts["SPX_ERR_ARG"]
