"""The edge generators of tests/nrt_edges.py against the CPU oracle alone: for every example the GPU tests draw
(nrt_edges.EXAMPLES_LONG / EXAMPLES_WIDE), each knob's edge is in the data and decides cells.  These are conditions on the generator,
not measurements of a kernel: where one does not hold the generator is what changes."""
import numpy as np
import pytest

import nrt_edges as E
from helpers import NRT
from scheduler_plugins_amd import objects as O
from test_flatten_nrt_rows import HostOnly

CONTAINER_FAILS = 4
_CACHE = {}


def _built(hdr, oracle, ex):
    if ex not in _CACHE:
        _CACHE.clear()  # (one example at a time: the tables of a 32-slot snapshot are not small)
        snap, edges = E.build(hdr, ex)
        params = O.nrt_params(hdr, O.Resources(), ex.strategy)
        osnap = oracle.Snapshot(snap["nodes"], snap["pods"], rc=snap["rc"], nrt=snap["nrt"], nrt_params=params)
        th = oracle.usable_cpus()
        _CACHE[ex] = (snap, edges, params, osnap.filter_rows(NRT, threads=th), osnap.score_rows(NRT, want_norm=False, threads=th)[0])
    return _CACHE[ex]


ALL = E.EXAMPLES_LONG + E.EXAMPLES_WIDE
IDS = [f"{ex.route}-{i}-{ex.strategy}-{ex.numa_ids}-{ex.slots}" for i, ex in enumerate(ALL)]


def test_example_lists_cover_the_knobs():
    for examples in (E.EXAMPLES_LONG, E.EXAMPLES_WIDE):
        assert {ex.strategy for ex in examples} == set(E.STRATEGIES)
        assert {ex.numa_ids for ex in examples} == {"position", "permuted", "sparse"}
        assert not any(ex.numa_ids == "sparse" and ex.strategy == "LeastNUMANodes" for ex in examples)
        for knob in ("spread", "tight_extra", "many_slots", "max_numa"):
            assert {getattr(ex, knob) for ex in examples} == {False, True}
        for s in E.STRATEGIES:  # every strategy sees ids that are not positions, and every knob
            assert any(ex.strategy == s and ex.numa_ids != "position" for ex in examples)
            assert any(ex.strategy == s and ex.spread for ex in examples) and any(ex.strategy == s and ex.tight_extra for ex in examples)
    assert {ex.slots for ex in E.EXAMPLES_LONG} == {4, 6} and {ex.slots for ex in E.EXAMPLES_WIDE} == {4, 6, 9, 12, 32}
    assert any(ex.strategy == "LeastNUMANodes" and ex.many_slots and ex.slots >= 6 for ex in E.EXAMPLES_WIDE)


@pytest.mark.parametrize("ex", ALL, ids=IDS)
def test_edges_are_in_the_data_and_decide_cells(hdr, oracle, ex):
    snap, edges, params, st, raw = _built(hdr, oracle, ex)
    nrt, pods = snap["nrt"], snap["pods"]
    ids, zptr = nrt.array("zone_numa_id"), nrt.array("zone_ptr")
    pos = np.arange(len(ids)) - np.repeat(zptr[:-1], np.diff(zptr))
    n_ctr = np.diff(pods.array("ctr_ptr"))

    # --- container counts: the limits are there, and nothing exceeds what the route takes
    want = (8, 9, 63, 64) if ex.route == "wide" else (8, 9, 64, 65, 200)
    assert [int(n_ctr[edges["count_rows"][c]]) for c in want] == list(want)
    if ex.route == "wide":
        assert n_ctr.max() == E.WIDE_MAX_CTRS

    # --- NUMA ids
    if ex.numa_ids == "position":
        assert (ids == pos).all()
    else:
        assert (ids != pos).any()
    if ex.numa_ids == "sparse":
        assert (ids >= 8).any() and (ids >= 32).any() and ids.max() <= 63
    if ex.strategy == "LeastNUMANodes":  # the reference indexes the zone list with the id: a permutation of the positions, node by node
        for i in range(len(zptr) - 1):
            assert sorted(ids[zptr[i]:zptr[i + 1]].tolist()) == list(range(zptr[i + 1] - zptr[i]))
    for i in range(len(zptr) - 1):
        assert len(set(ids[zptr[i]:zptr[i + 1]].tolist())) == zptr[i + 1] - zptr[i]

    # --- where a charge goes: ten containers that each fit the untouched zones, the tenth finds them emptied by the nine before
    c = edges["charge"]
    assert st[c["fail"], c["node"]] == CONTAINER_FAILS and st[c["ok"], c["node"]] == 0
    assert n_ctr[c["fail"]] == 10 and n_ctr[c["ok"]] == 9   # the nine are a prefix of the ten: every single container fits
    if ex.numa_ids != "position":
        assert c["low_pos"] != 0 and ids[zptr[c["node"]] + c["low_pos"]] == ids[zptr[c["node"]]:zptr[c["node"] + 1]].min()
    if ex.strategy == "LeastNUMANodes":
        g = edges["greedy"]
        if ex.numa_ids != "position":  # the charge goes to the position an id names: not where it goes with ids == positions
            reset = oracle.Snapshot(snap["nodes"], pods, rc=snap["rc"], nrt=E.ids_reset_to_positions(hdr, nrt), nrt_params=params)
            raw0 = reset.score_rows(NRT, g["row"], g["row"] + 1, want_norm=False)[0]
            assert raw0[0, g["node"]] != raw[g["row"], g["node"]]
            assert (raw0[0] != raw[g["row"]]).any()
        else:
            assert raw[g["row"], g["node"]] == 0

    # --- spread
    if ex.spread:
        s = edges["spread"]
        assert st[s["fail"], s["node"]] == CONTAINER_FAILS and st[s["ok"], s["node"]] == 0
        if ex.slots > 8:
            f = HostOnly().flatten_nrt_wide(snap["nodes"], nrt, snap["rc"], pods, params)["pods"]
            later = 0
            for p in range(len(n_ctr)):
                c0, c1 = f["ctr_ptr"][p], f["ctr_ptr"][p + 1]
                apps = [k for k in range(c0, c1) if f["ctr_kind"][k] == E.APP]
                for k in range(c0, c1):
                    e0, e1 = f["ent_ptr"][k], f["ent_ptr"][k + 1]
                    if (not apps or k != apps[0]) and ((f["ent_slot"][e0:e1] >= 8) & (f["ent_qty"][e0:e1] != 0)).any():
                        later += 1
            assert later >= 3
        kinds, cptr, rptr, res = pods.array("ctr_kind"), pods.array("ctr_ptr"), pods.array("req_ptr"), pods.array("req_res")
        named = {int(k) for k in np.flatnonzero(kinds != E.APP) if (res[rptr[k]:rptr[k + 1]] > E.MEM).any()}
        assert named, "no init or sidecar container names a resource beyond cpu and memory"
        single = [k for k in range(len(kinds)) if rptr[k + 1] - rptr[k] == 1]
        zero = [k for k in range(len(kinds)) if rptr[k + 1] > rptr[k] and (pods.array("req_qty")[rptr[k]:rptr[k + 1]] == 0).all()]
        assert single and zero

    # --- tight_extra: one pod, one node shape, both sides of the boundary
    if ex.tight_extra:
        t = edges["tight"]
        assert st[t["row"], t["lo"]] == CONTAINER_FAILS and st[t["row"], t["eq"]] == 0 and st[t["row"], t["hi"]] == 0

    # --- many_slots: the fifth and later non-zero slots decide the subset
    if "many" in edges:
        m = edges["many"]
        assert m["n_slots"] > 4
        if ex.strategy == "LeastNUMANodes":
            assert raw[m["all"], m["node"]] < raw[m["four"], m["node"]] and raw[m["all"], m["node"]] > 0

    # --- every example: its long / extra-requesting rows pass and fail, and score in more than two ways
    rows = E.edge_rows(snap, ex)
    assert len(rows) > 10 and (n_ctr[rows] > 8).sum() >= 5
    assert (st[rows] == 0).any() and (st[rows] != 0).any()
    assert len(np.unique(raw[rows])) >= 3
