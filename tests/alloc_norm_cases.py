"""Constructed node tables, feasibility rows and the plain-integer reference for NodeResourcesAllocatable's feasibility-aware
NormalizeScore: lo / hi of the raw scores over a pod's feasible nodes, then (s - lo) * 100 / (hi - lo) in Go's int64 arithmetic.
No GPU is needed here: tests/test_alloc_norm_cases.py checks that the rows hold what their names say, holds the reference to the
oracle's orc_allocatable_normalize and shows that host models of three wrong kernels are caught;
tests/test_gpu_alloc_norm_edges.py uploads the tables (Engine.set_allocatable("Most", {1: 1}) + Engine.upload_alloc_nodes make the
raw score of node n the uploaded alloc[0][n], "Least" its negation; Engine.upload_feasible_mask gives the feasible sets) and
compares every byte at tolerance 0.

Which copy of the operation the engine runs (kernels_profile.hip, kernels_network.hip):
  * the GLOBAL range of the raw column (k_alloc_prepare) picks the copy: below 2^32 the compact forms (alloc_masked_compact, the
    two fused forms of k_net_cls, k_decide_masked), from 2^32 on k_alloc_masked's int64 passes                    -> selects()
  * in k_alloc_masked the ROW's range picks the branch: below 2^42 one float64 product ("small"), from 2^42 on an integer
    division ("wide"), which from floor(2^63 / 100) + 1 on has to follow the reference's wrapping product ("wrap") -> branch()

All rows of an engine share the raw column and differ in their feasible set, so a table is made of GROUPS (lo, R): group g
contributes the nodes lo + d for d in family(R): {0, 1, R - 1, R} and, for q = 1..100 (a subset at 17 and 1025 nodes that keeps
1, 50, 99 and 100), {c_q - 1, c_q, c_q + 1} with c_q = ceil(q * R / 100): the first cell of every quotient, the last cell of the
one before, and one past.  A group's nodes are scattered by a seeded permutation; the lo and hi nodes of up to five groups are
pinned on the pairs of best_cases.PAIRS and (0, n_nodes - 1) — the lane boundaries of 4 and 16 nodes per lane, the tile boundaries
of 256 and 1024 nodes and the first and last node — and one adversarial cell (c_50 - 1) of each of those groups next to them
(the pairs use up best_cases.STRICT_AT, so the third pin of a group sits one node further); the seed also rotates which groups
are pinned.  Where the groups of a class do not fit n_nodes (17 nodes hold one group), the class is split into several tables
("parts") with the same global range and the same number of rows."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from best_cases import PAIRS, STRICT_AT

M64 = (1 << 64) - 1
WRAP_FROM = (1 << 63) // 100 + 1          # 92 233 720 368 547 759: the first range whose top cell's product d * 100 reaches 2^63
COMPACT, GENERAL = "alloc_masked_compact", "k_alloc_masked"
SMALL, WIDE, WRAP = "small", "wide", "wrap"

# Ranges in [2^42, 2^44) on which the single float64 product floor(d * RN(100 / R) * (1 + 2^-49)) mis-rounds a cell of family(R):
# the first two that tests/test_alloc_norm_cases.py::search_misrounding_ranges finds in [2^42, 2^43) and the first two in
# [2^43, 2^44) (numpy default_rng(42), uniform draws from the interval, every cell of the full family tried), each with its first
# mis-rounded cell d (a c_q - 1: the product lands on q).  The cell is part of the group's family at every node count.  A row with
# such a range fails if the 2^42 threshold is ever moved up — to 2^43 already, for the first two.
SEARCHED_RANGES = ((8174200097211, 7438522088462), (5957268208333, 5778550162083), (16348400194422, 14877044176924), (15710387772861, 6441258986873))

# Ranges R = 100 * k — every quotient q has an exact-integer cell d = q * k — on which the product WITHOUT the (1 + 2^-49) bias,
# floor(d * RN(100 / R)), falls below such a cell's integer: the first that test_alloc_norm_cases.py::search_unbiased_range finds
# with R < 2^32 (class A) and with 2^32 < R < 2^42 (class B2), each with its first such cell (q = 1: d = k, in every family).
UNBIASED_RANGES = ((3347818200, 33478182), (3928447272900, 39284472729))


# -------------------------------------------------------------------------------------------------------------- reference
def wrap64(x: int) -> int:
    """x as Go's int64 holds it"""
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def tdiv(a: int, b: int) -> int:
    """Go's / on integers: truncates toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def normalize(values: Sequence[int]) -> List[int]:
    """Allocatable.NormalizeScore over the list it is handed (allocatable.go:143-168), clamped to the byte the tables hold:
    wrap64((v - lo) * 100) divided, truncating, by wrap64(hi - lo); 0 when hi == lo"""
    if not values:
        return []
    lo, hi = min(values), max(values)
    rng = wrap64(hi - lo)
    if rng == 0:
        return [0] * len(values)
    return [min(255, max(0, tdiv(wrap64((v - lo) * 100), rng))) for v in values]


def reference(raw: Sequence[int], feasible: np.ndarray) -> np.ndarray:
    """the row of bytes for one pod: normalize() over the feasible nodes' raw scores, 0 on every other node"""
    idx = np.flatnonzero(feasible)
    out = np.zeros(len(raw), dtype=np.uint8)
    out[idx] = normalize([raw[i] for i in idx])
    return out


def selects(global_range: int) -> str:
    """k_alloc_prepare's rule on the raw column's range hi - lo (as an unsigned 64-bit number)"""
    return COMPACT if (global_range & M64) < (1 << 32) else GENERAL


def branch(row_range: int) -> str:
    """k_alloc_masked's branch for a row whose feasible raw scores span row_range"""
    return SMALL if row_range < (1 << 42) else WIDE if row_range < WRAP_FROM else WRAP


# ---------------------------------------------------------------------------------------------------- host models of kernels
def model_right(d: int, R: int) -> int:
    """the product of the compact forms and the small branch: floor(d * RN(100 / R) * (1 + 2^-49)), for R < 2^42"""
    assert 0 < R < (1 << 42)
    return int(float(d) * ((100.0 / R) * (1.0 + 2.0 ** -49)))


def model_no_bias(d: int, R: int) -> int:
    """WRONG: the product without the (1 + 2^-49) bias, the multiplier rounded down one ulp"""
    return int(float(d) * math.nextafter(100.0 / R, 0.0))


def model_unbiased(d: int, R: int) -> int:
    """WRONG: the product without the (1 + 2^-49) bias, the multiplier as the division rounds it"""
    return int(float(d) * (100.0 / R))


def model_single_product(d: int, R: int) -> int:
    """WRONG: the single product for every range (no 2^42 threshold)"""
    return min(255, int(float(d) * ((100.0 / float(R)) * (1.0 + 2.0 ** -49))))


def model_unsigned(d: int, R: int) -> int:
    """WRONG: an unsigned 64-bit product and quotient for every range"""
    return min(255, ((d * 100) & M64) // (R & M64))


# ---------------------------------------------------------------------------------------------------------------- families
Q_ALWAYS = (1, 50, 99, 100)


def q_subset(k: int) -> Tuple[int, ...]:
    """k of the quotients 1..100 (all of them from k = 100 on), Q_ALWAYS among them"""
    if k >= 100:
        return tuple(range(1, 101))
    qs = set(Q_ALWAYS)
    for q in np.linspace(2, 98, max(k - len(Q_ALWAYS), 0)).round().astype(int).tolist():
        qs.add(int(q))
    return tuple(sorted(qs))


def c_of(q: int, R: int) -> int:
    """ceil(q * R / 100): the first offset whose quotient is q"""
    return -(-q * R // 100)


def family(R: int, qs: Iterable[int] = tuple(range(1, 101))) -> List[int]:
    ds = {0, 1, R - 1, R}
    for q in qs:
        c = c_of(q, R)
        ds |= {c - 1, c, c + 1}
    return sorted(d for d in ds if 0 <= d <= R)


# ----------------------------------------------------------------------------------------------------------------- classes
@dataclass(frozen=True)
class Group:
    lo: int
    R: int
    extra: Tuple[int, ...] = ()   # cells every family of the group holds, whatever the subset of quotients


@dataclass(frozen=True)
class Klass:
    name: str
    glo: int            # the raw column's minimum
    grange: int         # ... and its range: what picks the copy
    groups: Tuple[Group, ...]

    @property
    def copy(self) -> str:
        return selects(self.grange)


def _klass(name: str, glo: int, grange: int, offs: Sequence[Tuple[int, int]], absolute: bool = False) -> Klass:
    cells = dict(SEARCHED_RANGES)
    groups = tuple(Group(lo if absolute else glo + lo, R, (cells[R],) if R in cells else ()) for lo, R in offs)
    for g in groups:
        # every lo lies strictly above the global minimum — except a group whose range IS the global range, which has no other place
        assert glo <= g.lo and g.lo + g.R <= glo + grange and (g.lo > glo or g.R == grange), (name, g)
    return Klass(name, glo, grange, groups)


P31, P32, P42 = 1 << 31, 1 << 32, 1 << 42
# class A: the last compact global range.  (offset of lo from the global minimum, R); multiples of 100 give exact-integer quotients
A = _klass("A", -3 * P31 - 17, P32 - 1, [
    (5, 1), (P31 + 9, 2), (1000, 99), (P31 + (1 << 30), 100), (77, 101), (P32 - 1000, 200), (12345, 100 << 16), (P31, P31 - 1),
    (P31 - 5, P31), (50, 4294967200), (900000001, UNBIASED_RANGES[0][0]), (0, P32 - 1)])
# class B: the first non-compact global range; every row is still "small".  B2's cells with d >= 2^32 exercise the two-halves fma
B1 = _klass("B1", -(1 << 40) + 3, P32, [(P32 - 1, 1), (P31, 100), (1, P32 - 1), (0, P32)])
B2 = _klass("B2", (1 << 45) + 1, P42 - 1, [(12, P32 + 1), (1 << 41, 100 << 30), (1 << 40, (1 << 41) + 12345), (60, P42 - 100), (7, UNBIASED_RANGES[1][0]), (0, P42 - 1)])
# class C: global range >= 2^42 (here 2^63 + 12345: the column's minimum is negative, its maximum positive, the int64 range wraps)
_C_GLO, _C_RANGE = -(1 << 62) - 7, (1 << 63) + 12345
C = _klass("C", _C_GLO, _C_RANGE, [
    # rows of the small branch: lo far from the global minimum, negative (and one positive)
    (-(1 << 50), 100), (-(1 << 50) - (1 << 43), P32 + 1), (-(1 << 55), P42 - 1), ((1 << 40) + 3, 100 << 30),
    # rows of the wide branch
    (-(1 << 58), P42), ((1 << 57) + 1, P42 + 1), (-(1 << 51), 1 << 50), (-(1 << 56) - 3, 1 << 56), (-(1 << 61), WRAP_FROM - 1),
    # ... on which the single product mis-rounds
    (-(1 << 48) + 1, SEARCHED_RANGES[0][0]), (1 << 47, SEARCHED_RANGES[1][0]), (-5, SEARCHED_RANGES[2][0]), (-(1 << 52) - 11, SEARCHED_RANGES[3][0]),
    # the wrap rows: d * 100 reaches 2^63; the last two ranges are 2^63 - 1 and, with a negative lo and a positive hi, above 2^63
    (-(1 << 60), WRAP_FROM), (-(1 << 56), 1 << 57), (-(1 << 59) - 1, 1 << 60), (-(1 << 61) - 9, (1 << 62) + 12345),
    (_C_GLO + 5, (1 << 63) - 1), (_C_GLO, _C_RANGE)], absolute=True)
CLASSES = {k.name: k for k in (A, B1, B2, C)}


# ------------------------------------------------------------------------------------------------------------------ tables
@dataclass
class Row:
    name: str
    groups: Tuple[int, ...]      # indices into Table.groups of the groups the row is about (none for the generic rows)
    lo: Optional[int]            # of the feasible raw scores (None: no feasible node)
    R: Optional[int]


@dataclass
class Table:
    klass: Klass
    n_nodes: int
    part: int
    seed: int
    groups: List[Group]
    raw: List[int]                       # raw score per node (plain integers)
    group_of: np.ndarray                 # per node: index into groups, -1 for the two nodes that only fix the global range
    d_of: List[int]                      # per node: raw - lo of its group
    pinned: List[Tuple[int, int, int, Optional[int]]]   # (group, node of lo, node of hi, node of the adversarial cell)
    rows: List[Optional[Row]] = field(default_factory=list)   # None: a placeholder row (random feasibility), no name
    masks: Optional[np.ndarray] = None   # uint8[rows][n_nodes], non-zero = feasible
    want: Optional[np.ndarray] = None    # uint8[rows][n_nodes]: reference() per row

    @property
    def n_rows(self) -> int:
        return len(self.rows)

    def alloc(self, mode: str) -> np.ndarray:
        """the [1][n_nodes] int64 column to upload so that the raw scores are self.raw under `mode`"""
        return np.array([[v if mode == "Most" else -v for v in self.raw]], dtype=np.int64)

    def describe(self, r: int) -> str:
        row = self.rows[r]
        gs = [] if row is None else [(self.groups[g].lo, self.groups[g].R) for g in row.groups]
        return (f"class {self.klass.name} ({self.klass.copy}) part {self.part} seed {self.seed}, row {r} "
                f"{'<placeholder>' if row is None else row.name!r}, groups (lo, R) {gs}")

    def mismatches(self, got: np.ndarray, rb: int, re: int, ctx="", limit: int = 6) -> List[str]:
        """messages for the cells of rows rb..re-1 where `got` differs from the reference"""
        out = []
        for r, n in np.argwhere(got != self.want[rb:re])[:limit]:
            g = int(self.group_of[n])
            cell = f"node {n} (group {(self.groups[g].lo, self.groups[g].R) if g >= 0 else None}, d {self.d_of[n]}, raw {self.raw[n]})"
            out.append(f"{ctx} {self.describe(rb + int(r))}, row range {(rb, re)}, {cell}: got {got[r, n]} want {self.want[rb + r, n]}")
        return out


PIN_PAIRS = ((0, -1),) + PAIRS    # (-1: the last node)
assert {n for pair in PIN_PAIRS for n in pair if n >= 0} == set(STRICT_AT)   # the pairs are best_cases.STRICT_AT, two by two
MIN_PER_GROUP = 14      # {0, 1, R - 1, R}, c - 1, c, c + 1 for q = 1, 50, 99 (q = 100 adds nothing to the first four), one extra cell
N_PLACEHOLDERS = 3


def parts_of(klass: Klass, n_nodes: int) -> List[List[Group]]:
    per_part = max(1, min(len(klass.groups), (n_nodes - 2) // MIN_PER_GROUP))
    return [list(klass.groups[i:i + per_part]) for i in range(0, len(klass.groups), per_part)]


def build(name: str, n_nodes: int, seed: int = 0) -> List[Table]:
    """the tables ("parts") of one class at one node count; every part has the same number of rows"""
    klass = CLASSES[name]
    assert n_nodes >= 2 + MIN_PER_GROUP
    tables = [_build_part(klass, n_nodes, p, groups, seed) for p, groups in enumerate(parts_of(klass, n_nodes))]
    n_rows = max(t.n_rows for t in tables)
    for t in tables:
        rng = np.random.default_rng([seed, t.part, 7])
        masks = [t.masks]
        while t.n_rows + len(masks) - 1 < n_rows:   # a short last part: more placeholder rows
            masks.append((rng.random((1, n_nodes)) < 0.5).astype(np.uint8))
        t.rows += [None] * (len(masks) - 1)
        t.masks = np.ascontiguousarray(np.concatenate(masks))
        t.want = np.stack([reference(t.raw, t.masks[r]) for r in range(t.n_rows)])
    return tables


def _build_part(klass: Klass, n_nodes: int, part: int, groups: List[Group], seed: int) -> Table:
    rng = np.random.default_rng([seed, part, n_nodes])
    N, G = n_nodes, len(groups)
    per_group = (N - 2) // G
    qs = q_subset((per_group - 5) // 3)   # 4 fixed cells, one extra, three per quotient
    # (raw, group, d) per node, before the permutation: the two ends of the global range, the families, then repeats of family cells
    items: List[Tuple[int, int, int]] = [(klass.glo, -1, 0), (klass.glo + klass.grange, -1, 0)]
    for g, grp in enumerate(groups):
        fam = sorted(set(family(grp.R, qs)) | set(grp.extra))
        assert len(fam) <= per_group
        items += [(grp.lo + d, g, d) for d in fam]
    full = [family(grp.R) for grp in groups]
    while len(items) < N:
        g = int(rng.integers(0, G))
        d = full[g][int(rng.integers(0, len(full[g])))]
        items.append((groups[g].lo + d, g, d))
    pos = rng.permutation(N)            # pos[i]: the node item i sits on
    at = np.argsort(pos)                # at[n]: the item on node n

    def pin(i: int, n: int) -> None:
        j, old = int(at[n]), int(pos[i])
        pos[i], pos[j] = n, old
        at[n], at[old] = i, j

    def item_of(g: int, d: int) -> Optional[int]:
        return next((i for i, (_, gg, dd) in enumerate(items) if gg == g and dd == d), None)

    pairs, used = [], set()
    for a, b in PIN_PAIRS:
        a, b = a % N, b % N
        if max(a, b) < N and a != b and not {a, b} & used:
            pairs.append((a, b))
            used |= {a, b}
    near = [n for n in (N - 2, 1, 2, 5, 14, 17, 254, 257, 1022, 1025) if 0 <= n < N and n not in used]
    pinned = []
    rot = (seed + part) % G
    for k, (a, b) in enumerate(pairs[:G]):
        g = (rot + k) % G
        if k % 2 == 0:
            a, b = b, a                 # even pairs: hi first — the first pair puts a minimum on the last node, its maximum on node 0
        i_lo, i_hi = item_of(g, 0), item_of(g, groups[g].R)
        pin(i_lo, a)
        pin(i_hi, b)
        adv, i_adv = None, item_of(g, c_of(50, groups[g].R) - 1)
        if i_adv is not None and i_adv not in (i_lo, i_hi) and k < len(near):
            adv = near[k]
            pin(i_adv, adv)
        pinned.append((g, a, b, adv))
    raw = [items[int(at[n])][0] for n in range(N)]
    group_of = np.array([items[int(at[n])][1] for n in range(N)], dtype=np.int64)
    d_of = [items[int(at[n])][2] for n in range(N)]
    t = Table(klass, N, part, seed, groups, raw, group_of, d_of, pinned)

    masks: List[np.ndarray] = []

    def add(name: Optional[str], feasible: np.ndarray, gs: Tuple[int, ...] = ()) -> None:
        vals = [raw[i] for i in np.flatnonzero(feasible)]
        t.rows.append(None if name is None else Row(name, gs, min(vals) if vals else None, max(vals) - min(vals) if vals else None))
        masks.append(feasible.astype(np.uint8))

    def nodes(*idx: int) -> np.ndarray:
        m = np.zeros(N, dtype=bool)
        m[list(idx)] = True
        return m

    add(None, rng.random(N) < 0.5)
    add("all nodes feasible", np.ones(N, dtype=bool))
    for g, grp in enumerate(groups):
        add(f"every cell of group {g}", group_of == g, (g,))
    add(None, rng.random(N) < 0.9)
    for g, a, b, _ in pinned:
        add(f"only lo and hi of group {g}, at nodes {(a, b)}", nodes(a, b), (g,))
    # all feasible values equal (R = 0) at a value that is not the global minimum: the most frequent one
    values, counts = np.unique(np.array([v for v in raw if v != klass.glo], dtype=object), return_counts=True)
    v_eq = values[int(np.argmax(counts))]
    add("all feasible values equal", np.array([v == v_eq for v in raw]))
    add("no feasible node", np.zeros(N, dtype=bool))
    add("only node 0", nodes(0))
    add(f"only node {N - 1}", nodes(N - 1))
    # two groups feasible at once: lo comes from the first, hi from the second (the first and the last such pair of the part)
    two = [(i, j) for i in range(G) for j in range(G)
           if groups[i].lo < groups[j].lo and groups[i].lo + groups[i].R < groups[j].lo + groups[j].R]
    for i, j in ([two[0], two[-1]] if len(two) > 1 else two):
        add(f"groups {i} and {j} feasible", (group_of == i) | (group_of == j), (i, j))
    add(None, rng.random(N) < 0.1)
    t.masks = np.stack(masks)
    return t


# -------------------------------------------------------------------------------------- TargetLoadPacking bytes for spx_decide
TLP_TARGET = 40


def tlp_util_for(score: int) -> float:
    """the cpu utilisation (percent) of a node whose TargetLoadPacking score is `score` for a pod that asks for nothing, at target
    utilisation 40: a score s >= 40 needs a predicted utilisation of (s - 40) / 1.5, s < 40 needs 100 - 1.5 * s; the score formula
    (targetloadpacking.go:169-186) then lands on the integer, half a unit from any rounding edge"""
    assert 0 <= score <= 100
    return (score - 40) / 1.5 if score >= 40 else 100 - 1.5 * score


def tlp_score_model(util: float, cap_milli: int) -> int:
    """TargetLoadPacking.Score in float64 as the oracle restates it, for a pod of zero millicores and nothing missing"""
    cap = float(cap_milli)
    predicted = 100 * ((util / 100) * cap + 0.0 + 0.0) / cap
    t = float(TLP_TARGET)
    if predicted > t:
        return 0 if predicted > 100 else int(math.floor(t * (100 - predicted) / (100 - t) + 0.5))
    return int(math.floor((100 - t) * predicted / t + t + 0.5))


TLP_CAP_MILLI = 100_000


def tlp_bytes(t: Table) -> np.ndarray:
    """per node the TargetLoadPacking byte that makes every total of the node's group row 100: 100 - (its byte in that row);
    0 on the two nodes outside every group"""
    out = np.zeros(t.n_nodes, dtype=np.uint8)
    for r, row in enumerate(t.rows):
        if row is not None and row.name.startswith("every cell of group"):
            m = t.masks[r] != 0
            out[m] = 100 - t.want[r][m]
    return out


def trimaran_columns(t: Table, scores: Optional[np.ndarray] = None):
    """(node columns, pod columns) for Engine.upload_trimaran_nodes / upload_trimaran_pods: every node's TargetLoadPacking score is
    scores[n] (default tlp_bytes(t)) for every pod; LoadVariationRiskBalancing's columns are zero"""
    N, P = t.n_nodes, t.n_rows
    scores = tlp_bytes(t) if scores is None else scores
    z64, zf = np.zeros(N, np.int64), np.zeros(N, np.float64)
    nodes = {"cap_cpu_milli": np.full(N, TLP_CAP_MILLI, np.int64), "tlp_cpu_util": np.array([tlp_util_for(int(s)) for s in scores], np.float64),
             "tlp_missing_milli": z64.copy(), "tlp_valid": np.ones(N, np.uint8), "lv_alloc_cpu_milli": z64.copy(), "lv_alloc_mem": z64.copy(),
             "lv_cpu_avg": zf.copy(), "lv_cpu_std": zf.copy(), "lv_mem_avg": zf.copy(), "lv_mem_std": zf.copy(), "lv_flags": np.zeros(N, np.uint8)}
    pods = {"tlp_pod_milli": np.zeros(P, np.int64), "lv_req_cpu_milli": np.zeros(P, np.int64), "lv_req_mem": np.zeros(P, np.int64)}
    return nodes, pods


# ------------------------------------------------------------------------------- NetworkOverhead snapshots for the fused forms
# seed of synth.network_snapshot per node count for which the oracle's NetworkOverhead Filter leaves the class A rows usable
# (network_conditions: the first of the seeds 1, 2, ... that meets them; tests/test_alloc_norm_cases.py checks it with the oracle)
NET_SEEDS = {17: 2, 1025: 53, 16385: 51}
NET_PODS_PER_GROUP = 5


def network_snapshot(hdr, t: Table, seed: int):
    """synth.network_snapshot with one pod per row of `t`: the pods of even rows belong to no AppGroup (k_net_cls's dependency-free
    form), those of odd rows to one (row 1 is "all nodes feasible")"""
    from scheduler_plugins_amd import synth
    snap = synth.network_snapshot(hdr, t.n_nodes, t.n_rows, seed=seed, pods_per_group=NET_PODS_PER_GROUP)
    n_groups = snap["appgroups"].struct.n_groups
    ag, sel = snap["pods"].array("appgroup"), snap["pods"].array("selector")
    for r in range(t.n_rows):
        if r % 2 == 0:
            ag[r] = sel[r] = -1
        elif ag[r] < 0:
            ag[r], sel[r] = r % n_groups, r % 11
    return snap


def dependency_hosts(snap, r: int) -> set:
    """the nodes that host a placed pod of one of the dependencies of row r's workload"""
    g, s = int(snap["pods"].array("appgroup")[r]), int(snap["pods"].array("selector")[r])
    if g < 0:
        return set()
    a = snap["appgroups"]
    wl = [w for w in range(a.array("wl_ptr")[g], a.array("wl_ptr")[g + 1]) if a.array("wl_selector")[w] == s]
    deps = {int(x) for w in wl for x in a.array("dep_selector")[a.array("dep_ptr")[w]:a.array("dep_ptr")[w + 1]]}
    lo, hi = a.array("placed_ptr")[g], a.array("placed_ptr")[g + 1]
    return {int(n) for n, ps in zip(a.array("placed_node")[lo:hi], a.array("placed_selector")[lo:hi]) if int(ps) in deps}


def network_conditions(t: Table, snap, status: np.ndarray) -> List[str]:
    """what the NetworkOverhead Filter verdicts `status` ([rows][n_nodes], 0 = passed) must leave of `t` (an empty list: all met):
    every row of an ungrouped pod keeps all of its cells; no grouped row loses more than half of its group's cells; at least one
    grouped row keeps a node that hosts one of its dependencies feasible (the exact-path branch of the fused form) — and the
    Filter does take cells from some row"""
    bad, host_kept, lost = [], False, False
    for r in range(t.n_rows):
        m = t.masks[r] != 0
        kept = m & (status[r] == 0)
        if r % 2 == 0:
            if not np.array_equal(kept, m):
                bad.append(f"ungrouped row {r} loses cells")
            continue
        if t.rows[r] is not None and t.rows[r].groups and 2 * kept.sum() < m.sum():
            bad.append(f"grouped row {r} keeps {kept.sum()} of {m.sum()} cells")
        host_kept |= any(kept[n] for n in dependency_hosts(snap, r))
        lost |= bool(kept.sum() < m.sum())
    if not lost:
        bad.append("the Filter takes no cell from any row")
    if not host_kept:
        bad.append("no grouped row keeps a dependency's host feasible")
    return bad
