"""Constructed score and status tables for the per-pod weighted argmax (k_best_fast / k_best, kernels_profile.hip), and the
plain numpy int64 reference they are held to.  No GPU is needed here: tests/test_best_cases.py checks that the rows hold what
their names say, tests/test_gpu_best_edges.py writes them into bound tables and runs spx_eval_best over them.

A row of the tables is one pod.  The named rows are built so that their answer holds for EVERY weight vector that is
non-negative with at least one positive weight on a table in play ("dominant" rows: the nodes meant to win carry the larger byte in
every table); a few hold for unit weights only and say so.  Under zero or negative weights the same bytes are still a valid
input — the reference says what the answer is then."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

# ---------------------------------------------------------------------------------------------------------------- weights
# (weights of the three Trimaran-profile tables, the kernel launch_best's rule selects).  The rule (kernels_profile.hip): the
# 32-bit kernel when every weight in play is in [0, 2^23) and sum(weight * 255) < 2^31, the general int64 kernel otherwise.
FAST, GENERAL = "k_best_fast", "k_best"
WEIGHT_SETS: List[Tuple[Tuple[int, ...], str]] = [
    ((1, 1, 1), FAST),
    ((0, 0, 0), FAST),                 # every total is 0: ties == feasible
    ((0, 5, 0), FAST),
    ((8388607, 32896, 1), FAST),       # sum w = 8 421 504, sum w * 255 = 2 147 483 520 < 2^31: the largest admitted sum
    ((8388607, 32897, 1), GENERAL),    # sum w * 255 = 2 147 483 775: the first sum refused
    ((8388608, 0, 0), GENERAL),        # a weight of exactly 2^23
    ((-3, 2, 1), GENERAL),
    ((-1, -1, -1), GENERAL),           # the best node is the one with the smallest bytes; scores are negative
    ((2 ** 40, -2 ** 40, 1), GENERAL),
    ((2 ** 47, 1, 0), GENERAL),
]
EXTRA_WEIGHTS = (1, 0)  # appended to each set for the five tables of the full profile
# the extension takes (8388607, 32896, 1) across the rule (sum w * 255 = 2^31 + 127): the largest admitted sum with five tables
FIVE_TABLE_LARGEST = (8388607, 32895, 1, 1, 0)


def extend(weights: Sequence[int], n_tables: int) -> Tuple[int, ...]:
    """a weight set of WEIGHT_SETS for `n_tables` tables (3, or 5 with EXTRA_WEIGHTS)"""
    w = tuple(weights) + EXTRA_WEIGHTS
    assert 3 <= n_tables <= len(w)
    return w[:n_tables]


def selects(weights: Sequence[int]) -> str:
    """launch_best's documented rule, for rows whose stride is a multiple of 16"""
    ok = all(0 <= w < 2 ** 23 for w in weights)
    return FAST if ok and sum(w * 255 for w in weights) < 2 ** 31 else GENERAL


def dominant_holds(weights: Sequence[int]) -> bool:
    """the "dominant" named rows keep their answer: no negative weight, one positive"""
    return all(w >= 0 for w in weights) and any(w > 0 for w in weights)


# -------------------------------------------------------------------------------------------------------------- reference
def reference(scores: Dict[int, np.ndarray], weights: Dict[int, int], statuses: Sequence[np.ndarray], n_nodes: int,
              rejected: Optional[np.ndarray] = None):
    """(node, score, ties, feasible) per row, int64 arithmetic.  scores: {plugin: uint8[rows][stride]}, weights: {plugin: int},
    statuses: uint8[rows][stride] each (non-zero = the node did not pass that Filter), rejected: bool[rows], rows turned away before
    any node is looked at (a PreFilter).  Columns >= n_nodes are never read."""
    rows = next(iter(scores.values())).shape[0] if scores else statuses[0].shape[0]
    total = np.zeros((rows, n_nodes), dtype=np.int64)
    for p, t in scores.items():
        assert t.dtype == np.uint8 and t.shape[0] == rows
        total += np.int64(weights[p]) * t[:, :n_nodes].astype(np.int64)
    ok = np.ones((rows, n_nodes), dtype=bool)
    for s in statuses:
        assert s.dtype == np.uint8 and s.shape[0] == rows
        ok &= s[:, :n_nodes] == 0
    if rejected is not None:
        ok[np.asarray(rejected, dtype=bool)] = False
    node = np.full(rows, -1, dtype=np.int64)
    score = np.zeros(rows, dtype=np.int64)
    ties = np.zeros(rows, dtype=np.int64)
    feasible = ok.sum(axis=1).astype(np.int64)
    for r in range(rows):
        if feasible[r] == 0:
            continue  # (-1, 0, 0, 0)
        idx = np.flatnonzero(ok[r])
        best = total[r, idx].max()
        at = idx[total[r, idx] == best]
        node[r], score[r], ties[r] = at[0], best, len(at)
    return node, score, ties, feasible


# ---------------------------------------------------------------------------------------------------------------- builder
@dataclass
class Row:
    name: str
    node: int                 # expected best node (-1: none)
    ties: int
    feasible: int
    unit_only: bool = False   # the answer holds for unit weights only (not for every non-negative weight vector)


@dataclass
class Cases:
    n_nodes: int
    stride: int
    scores: List[np.ndarray]      # n_tables x uint8[rows][stride]
    statuses: List[np.ndarray]    # n_status x uint8[rows][stride]
    rows: List[Optional[Row]] = field(default_factory=list)   # None: a random row, no built-in answer

    @property
    def n_rows(self) -> int:
        return len(self.rows)

    def feasible_mask(self, k: int) -> np.ndarray:
        """status table k as a caller's feasibility mask [rows][n_nodes] (non-zero = passed)"""
        return (self.statuses[k][:, :self.n_nodes] == 0).astype(np.uint8)


STRICT_AT = (0, 3, 4, 15, 16, 255, 256, 1023, 1024)   # lane boundaries of both kernels (16 and 4 nodes per lane), tile boundaries
PAIRS = ((3, 4), (15, 16), (255, 256), (1023, 1024))
TRIPLES = ((3, 4, 16), (15, 16, 17), (255, 256, 257), (1023, 1024, 1025))
CODES = (1, 0x80, 0xFF)
LOW, HIGH = 100, 200   # background bytes are <= LOW, the nodes built to win hold HIGH in every table


def build(n_nodes: int, stride: int, n_tables: int, n_status: int, seed: int, pad: Tuple[int, int] = (255, 0)) -> Cases:
    """tables for the named rows (module docstring; the list is in the code below, one `add` per row) at one shape.
    pad = (byte of the score tables', byte of the status tables' columns n_nodes .. stride-1): (255, 0) makes the padding look
    like the best feasible node."""
    assert 1 <= n_nodes <= stride and n_tables >= 1 and n_status >= 0
    rng = np.random.default_rng(seed)
    N = n_nodes
    sc_rows: List[np.ndarray] = []   # each [n_tables][N]
    st_rows: List[np.ndarray] = []   # each [n_status][N]
    rows: List[Optional[Row]] = []

    def background():
        return rng.integers(0, LOW + 1, size=(n_tables, N), dtype=np.uint8)

    def no_status():
        return np.zeros((n_status, N), dtype=np.uint8)

    def knock_out(st, keep, frac=0.2):
        """a random `frac` of the nodes outside `keep` infeasible, each through one random status table with a random code"""
        if n_status == 0:
            return
        out = np.flatnonzero(rng.random(N) < frac)
        out = out[~np.isin(out, keep)]
        st[rng.integers(0, n_status, size=len(out)), out] = rng.choice(CODES, size=len(out)).astype(np.uint8)

    def add(name, sc, st, node, ties, unit_only=False):
        feas = int((st == 0).all(axis=0).sum()) if n_status else N
        sc_rows.append(sc)
        st_rows.append(st)
        rows.append(Row(name, node, ties, feas, unit_only))

    # every node has the same total
    add("all equal", np.full((n_tables, N), 7, dtype=np.uint8), no_status(), 0, N)
    # one strict maximum at node k
    for k in sorted({k for k in STRICT_AT + (N - 1,) if k < N}):
        sc, st = background(), no_status()
        sc[:, k] = HIGH
        knock_out(st, [k])
        add(f"strict maximum at {k}", sc, st, k, 1)
    # two and three equal maxima
    for group in PAIRS + ((0, N - 1),) + TRIPLES + ((0, N // 2, N - 1),):
        if max(group) >= N or len(set(group)) != len(group):
            continue
        sc, st = background(), no_status()
        sc[:, list(group)] = HIGH
        knock_out(st, list(group))
        add(f"equal maxima at {group}", sc, st, min(group), len(group))
    # equal totals through different bytes: under unit weights 10 + 30 == 30 + 10 in the first two tables, 5 in the others
    if N >= 2 and n_tables >= 2:
        a, b = N - 1, N // 3 if N // 3 != N - 1 else 0
        sc, st = np.zeros((n_tables, N), dtype=np.uint8), no_status()
        sc[:, [a, b]] = 5
        sc[:2, a] = (10, 30)
        sc[:2, b] = (30, 10)
        add("equal totals, different bytes", sc, st, min(a, b), 2, unit_only=True)
    # a value above every feasible total on an infeasible node: each code, in each status table in turn
    if N >= 2:
        for t in range(n_status):
            for c, code in enumerate(CODES):
                bad = (0, N // 2, N - 1)[(t + c) % 3]
                good = (N - 1, 0, (N - 1) // 2)[(t + c) % 3]
                if good == bad:
                    good = (bad + 1) % N
                sc, st = background(), no_status()
                sc[:, bad] = 255
                sc[:, good] = HIGH
                st[t, bad] = code
                add(f"infeasible 255 at {bad}, code {code:#x} in status table {t}", sc, st, good, 1)
    if n_status:
        # no feasible node: every node is turned away by one of the status tables
        sc, st = background(), no_status()
        st[rng.integers(0, n_status, size=N), np.arange(N)] = rng.choice(CODES, size=N).astype(np.uint8)
        add("no feasible node", sc, st, -1, 0)
        for only in sorted({N - 1, 0}, reverse=True):
            sc, st = background(), no_status()
            sc[:, np.arange(N) != only] = 255   # everything else looks better
            st[rng.integers(0, n_status, size=N), np.arange(N)] = rng.choice(CODES, size=N).astype(np.uint8)
            st[:, only] = 0
            add(f"only node {only} feasible", sc, st, only, 1)
    # 255 in every table at one node
    sc = background()
    sc[:, N // 2] = 255
    add(f"255 in every table at {N // 2}", sc, no_status(), N // 2, 1)
    add("all bytes 0", np.zeros((n_tables, N), dtype=np.uint8), no_status(), 0, N)
    # random bytes from three values: many ties, no built-in answer
    for i in range(4):
        values = np.array([(0, 1, 255), (100, 99, 98), (0, 128, 255), (7, 7, 9)][i], dtype=np.uint8)
        sc, st = values[rng.integers(0, 3, size=(n_tables, N))], no_status()
        knock_out(st, [], frac=(0.0, 0.3, 0.6, 0.9)[i])
        sc_rows.append(sc)
        st_rows.append(st)
        rows.append(None)

    R = len(rows)
    scores = [np.full((R, stride), pad[0], dtype=np.uint8) for _ in range(n_tables)]
    statuses = [np.full((R, stride), pad[1], dtype=np.uint8) for _ in range(n_status)]
    for r in range(R):
        for t in range(n_tables):
            scores[t][r, :N] = sc_rows[r][t]
        for t in range(n_status):
            statuses[t][r, :N] = st_rows[r][t]
    return Cases(N, stride, scores, statuses, rows)
