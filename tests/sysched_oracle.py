"""Plain-Python restatement of pkg/sysched (SySched.Score and NormalizeScore) with Python sets, in the reference's literal form —
the oracle of the SySched kernels.  Test infrastructure: product code never imports it.

  score(P, H, Qs)        sysched.go:234-279: len(P) == 0 -> math.MaxInt64 (before the host lookup); H is None (no HostSyscalls
                         entry) -> 0; else len(H - P) + sum(len((H | P) - Q) for Q in Qs)   (calcScore is the set size, :217-231)
  normalize(scores)      :281-288 = upstream helper.DefaultNormalizeScore(100, reverse=True, scores) in int64 arithmetic:
                         max over the list floored at 0; max == 0 -> all 100; else 100 - 100 * s / max, Go's wrapping multiply
                         and truncating division
"""
import numpy as np

MAX_INT64 = (1 << 63) - 1
MAX_NODE_SCORE = 100


def wrap64(x: int) -> int:
    """a Python int as Go's int64 holds it after an overflowing operation (two's complement wraparound)"""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def quo(a: int, b: int) -> int:
    """Go's integer division: truncated toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def score(P, H, Qs) -> int:
    if len(P) == 0:
        return MAX_INT64
    if H is None:
        return 0
    total = len(H - P)
    new_host = H | P
    for Q in Qs:
        total += len(new_host - Q)
    return total


def normalize(scores):
    """DefaultNormalizeScore(maxPriority=100, reverse=True): the list in, the list out"""
    max_count = 0
    for s in scores:
        if s > max_count:
            max_count = s
    if max_count == 0:
        return [MAX_NODE_SCORE for _ in scores]  # reverse: every score becomes maxPriority
    out = []
    for s in scores:
        v = quo(wrap64(MAX_NODE_SCORE * s), max_count)
        out.append(wrap64(MAX_NODE_SCORE - v))
    return out


def raw_rows(sets, host, residents):
    """raw Score of every distinct pod set on every node: int64 [len(sets)][len(host)].  host[n] = frozenset or None, residents[n] =
    tuple of set ids.  Score is a pure function of (P, H, Qs), so nodes that share their host object and resident tuple share
    the cell."""
    out = np.zeros((len(sets), len(host)), np.int64)
    cache = {}
    for n, (H, res) in enumerate(zip(host, residents)):
        key = (id(H), res)
        col = cache.get(key)
        if col is None:
            Qs = [sets[q] for q in res]
            col = cache[key] = np.array([score(P, H, Qs) for P in sets], np.int64)
        out[:, n] = col
    return out


def normalize_row(raw_row: np.ndarray, feasible=None) -> np.ndarray:
    """NormalizeScore over the feasible nodes of a raw row (upstream scores only the nodes that passed every Filter); infeasible
    cells come out 0, the engine's convention for them.  Applied through the distinct values of the row."""
    raw_row = np.asarray(raw_row, np.int64)
    feas = np.ones(len(raw_row), bool) if feasible is None else np.asarray(feasible, bool)
    out = np.zeros(len(raw_row), np.int64)
    vals = raw_row[feas]
    if len(vals) == 0:
        return out
    uniq, inv = np.unique(vals, return_inverse=True)
    # normalize() reads the maximum from the list it is given: hand it the distinct values, which hold the maximum
    out[feas] = np.array(normalize([int(v) for v in uniq]), np.int64)[inv]
    return out


def tables(snap, feasible=None):
    """(raw int64 [P][N], normalised int64 [P][N]) of a synth.sysched_snapshot; feasible: bool [P][N] or None"""
    per_set = raw_rows(snap["sets"], snap["host"], snap["residents"])
    raw = per_set[snap["pod_set"]]
    if feasible is None:
        norm_set = np.stack([normalize_row(r) for r in per_set])
        return raw, norm_set[snap["pod_set"]]
    return raw, np.stack([normalize_row(raw[p], feasible[p]) for p in range(len(raw))])
