"""NodeMetadata (pkg/nodemetadata/node_metadata.go), PodState (pkg/podstate/pod_state.go) and QOSSort (pkg/qos/queue_sort.go) as plain
Python on plain ints: test infrastructure, nothing of the product.  Go's int64 arithmetic is spelled out (wrap64, go_div); the
ParseFloat grammar is a set of regular expressions, written independently of the flattener's scanner (Python's float() is not that
grammar: it takes blanks, "1_0", "nan(...)"-less NaNs with a sign, and no hexadecimal form).

Also the constructed columns and feasible sets of tests/test_gpu_node_columns*.py (tables), with the reference rows computed once.
"""
from __future__ import annotations

import calendar
import math
import re

import numpy as np

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
INVALID = INT64_MIN  # node_metadata.go:48
META, PODSTATE = "NodeMetadata", "PodState"


def wrap64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def go_div(a: int, b: int) -> int:
    """Go's int64 quotient: truncated toward zero; MinInt64 / -1 wraps"""
    q = abs(a) // abs(b)
    return wrap64(q if (a < 0) == (b < 0) else -q)


def clamp_byte(v: int) -> int:
    return 0 if v < 0 else 255 if v > 255 else v


# ------------------------------------------------------------------ NormalizeScore
def normalize_nodemeta(raw, feasible=None):
    """node_metadata.go:150-210 over the nodes with feasible[n] (None: all).  Returns the int64 the reference leaves per node, for EVERY
    node (an infeasible node's by the same rule, as the device writes it); None where nothing valid was seen and the cell is 0."""
    idx = range(len(raw)) if feasible is None else [n for n in range(len(raw)) if feasible[n]]
    valid = [raw[n] for n in idx if raw[n] != INVALID]
    if not valid:
        return [0] * len(raw)
    lo, hi = min(valid), max(valid)
    if lo == hi:
        return [0 if s == INVALID else 1 for s in raw]
    old = wrap64(hi - lo)
    return [0 if s == INVALID else wrap64(go_div(wrap64(wrap64(s - lo) * 99), old) + 1) for s in raw]


def normalize_podstate(raw, feasible=None):
    """pod_state.go:66-91"""
    idx = range(len(raw)) if feasible is None else [n for n in range(len(raw)) if feasible[n]]
    if len(idx) == 0:
        return [0] * len(raw)
    lo, hi = min(raw[n] for n in idx), max(raw[n] for n in idx)
    old = wrap64(hi - lo)
    return [0 if old == 0 else wrap64(go_div(wrap64(wrap64(s - lo) * 100), old)) for s in raw]


NORMALIZE = {META: normalize_nodemeta, PODSTATE: normalize_podstate}


def rows(kind, raw, masks):
    """uint8 [rows][N]: the bytes of every row under masks [rows][N] (non-zero = feasible)"""
    return np.array([[clamp_byte(v) for v in NORMALIZE[kind](raw, m)] for m in masks], dtype=np.uint8).reshape(len(masks), len(raw))


# ------------------------------------------------------------------ strconv.ParseFloat(s, 64)
_H = r"[0-9a-fA-F]"
_DEC = re.compile(r"[+-]?(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?", re.ASCII)
_HEX = re.compile(rf"[+-]?0[xX](?:(?:_?{_H})+(?:\.(?:{_H}(?:_?{_H})*)?)?|\.{_H}(?:_?{_H})*)[pP][+-]?\d(?:_?\d)*", re.ASCII)
_INF = re.compile(r"[+-]?(?:inf|infinity)", re.I)
_NAN = re.compile(r"nan", re.I)


def parse_float(s: str):
    """the float64, or None where Go returns an error (syntax or range)"""
    if _INF.fullmatch(s):
        return -math.inf if s[0] == "-" else math.inf
    if _NAN.fullmatch(s):
        return math.nan
    if _DEC.fullmatch(s):
        v = float(s)
        return None if math.isinf(v) else v
    if _HEX.fullmatch(s):
        try:
            return float.fromhex(s.replace("_", ""))
        except OverflowError:
            return None
    return None


def go_int64(v: float) -> int:
    """int64(v) on amd64: NaN, +-Inf and |v| >= 2^63 give MinInt64"""
    if math.isnan(v) or math.isinf(v) or v >= 2.0 ** 63 or v < -(2.0 ** 63):
        return INT64_MIN
    return int(v)


def number_score(value, strategy: str) -> int:
    """parseNumericValue (:108-122) behind calculateScore's lookup; value None = key not found"""
    v = None if value is None else parse_float(value)
    if v is None:
        return INVALID
    score = go_int64(v)
    return wrap64(-score) if strategy == "Lowest" else score


# ------------------------------------------------------------------ time.Parse(time.RFC3339, s), time.Since(t).Seconds()
_RFC3339 = re.compile(r"(\d{4})-(\d\d)-(\d\d)T(\d{1,2}):(\d\d):(\d\d)(?:[.,](\d+))?(Z|[+-]\d\d:\d\d)", re.ASCII)


def parse_rfc3339(s: str):
    """Unix nanoseconds, or None where time.Parse returns an error"""
    m = _RFC3339.fullmatch(s)
    if not m:
        return None
    y, mo, d, h, mi, sec = (int(m.group(k)) for k in range(1, 7))
    if not (1 <= mo <= 12 and 1 <= d <= calendar.monthrange(y if y else 400, mo)[1] and h < 24 and mi < 60 and sec < 60):
        return None
    frac = (m.group(7) or "")[:9].ljust(9, "0")
    off = 0
    if m.group(8) != "Z":
        oh, om = int(m.group(8)[1:3]), int(m.group(8)[4:6])
        if oh > 24 or om > 60:
            return None
        off = (oh * 3600 + om * 60) * (-1 if m.group(8)[0] == "-" else 1)
    days = (calendar.timegm((y + 400, mo, d, 0, 0, 0)) // 86400) - 146097  # (timegm wants a year >= 1: shift by one 400-year cycle)
    return ((days * 86400 + h * 3600 + mi * 60 + sec - off) * 10 ** 9) + int(frac)


def age_seconds(now_ns: int, t_ns: int) -> float:
    """time.Duration(now - t).Seconds(): float64(d / 1e9) + float64(d % 1e9) / 1e9, the difference saturated as Time.Sub does"""
    d = max(INT64_MIN, min(INT64_MAX, now_ns - t_ns))
    sec = abs(d) // 10 ** 9 * (1 if d >= 0 else -1)
    return float(sec) + float(d - sec * 10 ** 9) / 1e9


def timestamp_score(value, strategy: str, now_ns: int) -> int:
    t = None if value is None else parse_rfc3339(value)
    if t is None:
        return INVALID
    whole = go_int64(age_seconds(now_ns, t))
    return wrap64(-whole) if strategy == "Newest" else whole


def podstate_counts(n_nodes, assigned_node, assigned_terminating, nominated_node):
    raw = [0] * n_nodes
    for n, t in zip(assigned_node, assigned_terminating):
        raw[n] += 1 if t else 0
    for n in nominated_node:
        raw[n] -= 1
    return raw


QOS = {"BestEffort": 1, "Burstable": 2, "Guaranteed": 3}  # qosOrder, queue_sort.go:69-73


def qos_less(p1, p2) -> bool:
    """Sort.Less on (priority, class 1..3, timestamp) triples"""
    if p1[0] != p2[0]:
        return p1[0] > p2[0]
    if p1[1] != p2[1]:
        return p1[1] > p2[1]
    return p1[2] < p2[2]


# ------------------------------------------------------------------ constructed columns and feasible sets
RANGES = (1, 99, 100, (1 << 31) - 1, 1 << 32, (1 << 63) // 99, (1 << 63) // 99 + 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 2)
NODES = (1, 3, 63, 64, 65, 255, 256, 257, 1030)
PODS = (1, 2, 65)


class Table:
    """one raw column, its feasible sets (named rows) and the reference bytes"""

    def __init__(self, kind, raw, masks, names, label):
        self.kind, self.raw, self.masks, self.names, self.label = kind, [int(v) for v in raw], np.asarray(masks, dtype=np.uint8), list(names), label
        self.n_nodes, self.n_rows = len(raw), len(names)
        self.values = [NORMALIZE[kind](self.raw, m) for m in self.masks]  # the reference's int64 per cell
        self.want = np.array([[clamp_byte(v) for v in r] for r in self.values], dtype=np.uint8).reshape(self.n_rows, self.n_nodes)
        self.unmasked = np.array([clamp_byte(v) for v in NORMALIZE[kind](self.raw)], dtype=np.uint8)

    def row(self, name):
        return self.names.index(name)

    def mismatches(self, got, rb, re, tag=""):
        """cells of feasible nodes that differ, and (NodeMetadata) invalid nodes' cells that are not 0"""
        out = []
        for r in range(rb, re):
            g, w, m = got[r - rb], self.want[r], self.masks[r] != 0
            bad = (g != w) & m
            if self.kind == META:
                bad |= (np.array(self.raw, dtype=object) == INVALID).astype(bool) & (g != 0)
            for n in np.flatnonzero(bad)[:4]:
                out.append(f"{tag} {self.label} row {r} '{self.names[r]}' node {n} (raw {self.raw[n]}): got {g[n]} want {w[n]}")
        return out


def column(kind, n, span, place, seed):
    """n raw scores spanning exactly `span` (when n >= 2), the minimum at node place[0] and the maximum at place[1]; NodeMetadata
    columns carry invalid nodes in between.  Everything else is drawn below the maximum, with the values next to both ends present."""
    rng = np.random.default_rng(seed)
    if span >= (1 << 64) - 2:
        lo = INT64_MIN + 1
    elif span > INT64_MAX:
        lo = -(1 << 62)
    else:
        lo = -(span // 2) - 7 if kind == META else -(span // 2)
    hi = lo + span
    assert INT64_MIN < lo and hi <= INT64_MAX
    raw = [lo + int(rng.integers(0, 1 << 62)) % (span + 1) for _ in range(n)]
    near = [lo + 1, hi - 1, lo + span // 2, lo + span // 99, lo + span // 100 + 1]
    free = [i for i in range(n) if i not in place]
    for i, v in zip(rng.permutation(free)[:len(near)], near):
        raw[int(i)] = min(max(v, lo), hi)
    if kind == META:
        for i in rng.permutation(free)[len(near):len(near) + max(1, n // 7) if n > 8 else 0]:
            raw[int(i)] = INVALID
    if n >= 2:
        raw[place[0]], raw[place[1]] = lo, hi
    return raw


def placements(n):
    """(minimum's node, maximum's node): first and last, last and first, the last lane of the first 256-node tile and the one live
    lane of the second"""
    out = [(0, n - 1), (n - 1, 0)] if n >= 2 else [(0, 0)]
    if n >= 257:
        out.append((255, 256))
    return out


def masks_for(kind, raw, n_rows, seed):
    """the named feasible sets, then random ones up to n_rows (a batch of 1 or 2 rows takes the first ones of a rotation by seed)"""
    n = len(raw)
    rng = np.random.default_rng(seed + 1)
    valid = [i for i in range(n) if raw[i] != INVALID]
    invalid = [i for i in range(n) if raw[i] == INVALID]
    lo_i, hi_i = (min(valid, key=lambda i: raw[i]), max(valid, key=lambda i: raw[i])) if valid else (0, 0)
    named = []

    def add(name, idx):
        m = np.zeros(n, np.uint8)
        m[list(idx)] = 1
        named.append((name, m))

    add("all nodes feasible", range(n))
    add("one feasible node, valid", [hi_i] if valid else [])
    add("no feasible node", [])
    add("global minimum and maximum infeasible", [i for i in range(n) if not valid or raw[i] not in (raw[lo_i], raw[hi_i])])
    add("first and last node only", {0, n - 1})
    if invalid:
        add("one feasible node, invalid", [invalid[0]])
        add("feasible nodes all invalid", invalid)
    equal = [i for i in valid if raw[i] == raw[hi_i]]
    add("all valid feasible nodes equal, invalid ones mixed in", equal + invalid[:3])
    if n_rows < len(named):
        k = seed % len(named)
        named = [named[0]] + [named[(k + j) % len(named)] for j in range(1, n_rows)] if n_rows > 1 else [named[k]]
        named = named[:n_rows]
    while len(named) < n_rows:
        dens = (0.02, 0.3, 0.9)[len(named) % 3]
        named.append((f"random {dens}", (rng.random(n) < dens).astype(np.uint8)))
    return [m for _, m in named], [s for s, _ in named]


_cache = {}


def table(kind, n, n_rows, span, place, seed=0):
    key = (kind, n, n_rows, span, place, seed)
    if key not in _cache:  # built once (the reference with it) and left unchanged
        raw = column(kind, n, span, place, seed)
        masks, names = masks_for(kind, raw, n_rows, seed)
        _cache[key] = Table(kind, raw, masks, names, f"{kind} N={n} P={n_rows} span={span} place={place}")
    return _cache[key]


def podstate_span(n):
    return 2 * ((1 << 31) - 1) if n >= 2 else 0
