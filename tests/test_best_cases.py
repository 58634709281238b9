"""tests/best_cases.py on the CPU: the constructed rows hold what their names say, through the numpy reference, before
tests/test_gpu_best_edges.py holds the argmax kernels to the same reference."""
import numpy as np
import pytest

import best_cases as bc


@pytest.mark.parametrize("pad", [(255, 0), (0xAB, 0xAB)])
@pytest.mark.parametrize("n_tables,n_status", [(3, 1), (5, 3), (3, 0)])
def test_cases_hold_what_they_name(n_tables, n_status, pad):
    n_nodes, stride = 1030, 1152
    c = bc.build(n_nodes, stride, n_tables, n_status, seed=1, pad=pad)
    for t in c.scores + c.statuses:
        assert t.shape == (c.n_rows, stride) and t.dtype == np.uint8
    for t in c.scores:
        assert (t[:, n_nodes:] == pad[0]).all()
    for t in c.statuses:
        assert (t[:, n_nodes:] == pad[1]).all()
    names = [r.name for r in c.rows if r is not None]
    assert len(set(names)) == len(names)
    # every named row of the list is there at this shape
    for k in (0, 3, 4, 15, 16, 255, 256, 1023, 1024, n_nodes - 1):
        assert f"strict maximum at {k}" in names
    for g in bc.PAIRS + bc.TRIPLES + ((0, n_nodes - 1), (0, n_nodes // 2, n_nodes - 1)):
        assert f"equal maxima at {g}" in names
    for want in ("all equal", "equal totals, different bytes", "all bytes 0", f"255 in every table at {n_nodes // 2}"):
        assert want in names
    if n_status:
        for want in ("no feasible node", "only node 0 feasible", f"only node {n_nodes - 1} feasible"):
            assert want in names
        for t in range(n_status):
            for code in bc.CODES:
                assert sum(n.endswith(f"code {code:#x} in status table {t}") for n in names) == 1
    assert sum(r is None for r in c.rows) >= 3

    negative = above_2_53 = False
    for base, kernel in bc.WEIGHT_SETS:
        w = bc.extend(base, n_tables)
        # (with five tables the extension by (1, 0) moves the largest admitted sum across the rule: selects() says which kernel runs)
        assert bc.selects(w) == kernel or (n_tables == 5 and base == (8388607, 32896, 1)), w
        scores = dict(enumerate(c.scores))
        node, score, ties, feas = bc.reference(scores, dict(enumerate(w)), c.statuses, n_nodes)
        # the reference does not read the padding: another padding, the same answers
        other = bc.build(n_nodes, stride, n_tables, n_status, seed=1, pad=(pad[0] ^ 0xFF, pad[1] ^ 0xFF))
        for a, b in zip((node, score, ties, feas), bc.reference(dict(enumerate(other.scores)), dict(enumerate(w)), other.statuses, n_nodes)):
            assert np.array_equal(a, b)
        unit = all(x == 1 for x in w[:3])
        for r, row in enumerate(c.rows):
            if row is None:
                continue
            assert feas[r] == row.feasible, (row.name, w)
            if (row.unit_only and unit) or (not row.unit_only and bc.dominant_holds(w)):
                assert (node[r], ties[r]) == (row.node, row.ties), (row.name, w, node[r], ties[r])
            if not any(w):  # all totals 0: the first feasible node, ties == feasible
                assert score[r] == 0 and ties[r] == feas[r]
            if row.node < 0:
                assert (node[r], score[r], ties[r], feas[r]) == (-1, 0, 0, 0)
        if min(w) < 0:
            negative |= bool((score < 0).any())
        if max(w) >= 2 ** 40:
            above_2_53 |= bool((score > 2 ** 53).any())
    assert negative and above_2_53


def test_selection_rule_at_its_thresholds():
    assert bc.selects(bc.FIVE_TABLE_LARGEST) == bc.FAST and sum(w * 255 for w in bc.FIVE_TABLE_LARGEST) == 2 ** 31 - 128
    assert bc.selects((8388607, 32896, 1)) == bc.FAST and sum(w * 255 for w in (8388607, 32896, 1)) == 2 ** 31 - 128
    assert bc.selects((8388607, 32897, 1)) == bc.GENERAL and sum(w * 255 for w in (8388607, 32897, 1)) == 2 ** 31 + 127
    assert bc.selects((2 ** 23 - 1, 0, 0)) == bc.FAST and bc.selects((2 ** 23, 0, 0)) == bc.GENERAL
    assert bc.selects((0, 0, -1)) == bc.GENERAL


def test_reference_on_a_hand_made_table():
    s0 = np.array([[1, 9, 9, 200], [5, 5, 5, 200]], dtype=np.uint8)
    s1 = np.array([[0, 1, 1, 200], [0, 0, 0, 200]], dtype=np.uint8)
    st = np.array([[0, 0, 0, 0], [1, 0x80, 0xFF, 0]], dtype=np.uint8)
    node, score, ties, feas = bc.reference({0: s0, 4: s1}, {0: 2, 4: -3}, [st], 3)
    assert node.tolist() == [1, -1] and score.tolist() == [15, 0] and ties.tolist() == [2, 0] and feas.tolist() == [3, 0]
    node, score, ties, feas = bc.reference({0: s0, 4: s1}, {0: 2, 4: -3}, [], 3, rejected=np.array([True, False]))
    assert node.tolist() == [-1, 0] and score.tolist() == [0, 10] and ties.tolist() == [0, 3] and feas.tolist() == [0, 3]
