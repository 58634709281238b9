"""The examples of tests/nrt_tall_cases.py hold the edges they are built for: shown with the CPU oracle alone (it walks up to 64 zones),
so that tests/test_gpu_nrt_tall.py compares the GPU against cells that really are at those edges.  No GPU."""
import time

import numpy as np
import pytest

import nrt_tall_cases as TC
import nrt_tall_edge_cases as EC
from helpers import NRT


def _oracle(oracle, hdr, c, strategy="LeastAllocated"):
    s = TC.build(hdr, c, strategy)
    o = oracle.Snapshot(s["nodes"], s["pods"], rc=s["rc"], nrt=s["nrt"], nrt_params=s["params"])
    th = oracle.usable_cpus()
    return o.filter_rows(NRT, threads=th), o.score_rows(NRT, want_norm=False, threads=th)[0]


def test_id_patterns():
    for n in (9, 16, 17, 32, 33, 64):
        for pat in TC.ID_PATTERNS + EC.SHARED_PATTERNS:
            ids = pat(n)
            assert len(ids) == n and 0 <= min(ids) and max(ids) <= 63
            assert (len(set(ids)) == n) == (pat in TC.ID_PATTERNS)    # the duplicate-free patterns are; the shared ones are not
        assert TC.ids_permuted(n)[-1] == 0 and TC.ids_sparse(n)[-1] == min(TC.ids_sparse(n)) and max(TC.ids_sparse(n)) == 63


@pytest.mark.parametrize("nz,pat,n_ctr", [(9, TC.ids_equal, 8), (16, TC.ids_permuted, 8), (17, TC.ids_sparse, 9), (64, TC.ids_permuted, 65), (33, TC.ids_equal, 2)])
def test_charge_case_fails_by_one_unit_at_the_last_zone(hdr, oracle, nz, pat, n_ctr):
    """the deciding zone is the last list position, and a later container fails by one millicore because of the earlier charges"""
    c = TC.charge_case(nz, pat, n_ctr)
    st, _ = _oracle(oracle, hdr, c)
    assert st[0].tolist() == [TC.ST["container"], 0, 0]   # accumulated charge - 1, + 0, + 1
    assert st[1].tolist() == [0, 0, 0]                    # one container fewer fits all three
    # ... and only because of the last position: without its roomy zone nothing fits even one container
    for t in c["nrts"]:
        t["zones"][-1]["resources"]["cpu"] = "500m"
    st, _ = _oracle(oracle, hdr, c)
    assert (st == TC.ST["container"]).all()


@pytest.mark.parametrize("nz,pat", [(9, TC.ids_permuted), (32, TC.ids_sparse)])
def test_partial_resource_case(hdr, oracle, nz, pat):
    st, _ = _oracle(oracle, hdr, TC.partial_resource_case(nz, pat))
    C, P = TC.ST["container"], TC.ST["pod"]
    # node 0: two device zones -> the third device container finds none; node 1 does not list the device; node 2: pod scope sums the pod
    assert st[:3, 0].tolist() == [0, 0, C] and st[:3, 1].tolist() == [C, C, C] and st[:3, 2].tolist() == [0, P, P]
    assert st[3].tolist() == [0, 0, 0] and st[4, 0] == C    # hugepages: two halves fit one zone; 2Gi fits none
    assert st[5].tolist() == [C, C, P]                      # BestEffort with a device request is filtered like any other


def test_flags_case(hdr, oracle):
    c = TC.flags_case([9, 17, 64])
    st, raw = _oracle(oracle, hdr, c)
    for k in range(3):  # per zone count: container scope, pod scope, not single-NUMA, stale
        assert (st[:8, 4 * k + 3] == TC.ST["invalid"]).all() and st[8, 4 * k + 3] == 0   # stale: every pod but the empty BestEffort one
        assert (st[:, 4 * k + 2] == 0).all() and (raw[:6, 4 * k + 2] == 0).all()               # not single-NUMA: passes, scores 0
        assert st[9, 4 * k] == TC.ST["init"] and st[10, 4 * k] == TC.ST["sidecar"]
    assert TC.n_tall(c) == 12


@pytest.mark.parametrize("nz,pat", [(9, TC.ids_equal), (16, TC.ids_permuted)])
def test_least_numa_case(hdr, oracle, nz, pat):
    t0 = time.perf_counter()
    _, raw = _oracle(oracle, hdr, TC.least_numa_case(nz, pat), "LeastNUMANodes")
    assert time.perf_counter() - t0 < 5.0
    assert raw[0].tolist() == [94, 94, 94, 94]            # k = 1, always the minimum
    assert raw[1, 0] == 82 and raw[1, 1] == 76            # k = 2: hit on the closest pair; miss when position 0 is empty
    assert raw[2, 2] == 70 or raw[2, 2] == 64             # k = 3 directly after the last pair
    assert raw[2, 2] < raw[1, 2]
    if nz == 9:
        assert raw[3, 0] == -2 and raw[4, 0] == -2        # 18 cpu = all nine zones: the only subset of its size is the minimum
    else:
        assert raw[3, 3] == -8 and raw[3, 0] == -2        # k = 9 of 16: a miss where the cheap last zone is empty, a hit on the plain node
        assert raw[4, 0] == -86                           # k = 16, the last subset
    assert (raw[5] == 0).all() and (raw[6] == 0).all()    # nothing fits; a name no zone reports
    assert (raw[7] == 100).all()                          # not Guaranteed
    _, raw16 = _oracle(oracle, hdr, TC.least_numa_case(nz, pat, max_numa=16), "LeastNUMANodes")
    assert raw16[0, 0] == 100 - 6 + 3 and raw16[4, 0] == 100 - 6 * nz + 3


@pytest.mark.parametrize("nz", [9, 16])
def test_least_numa_greedy_case(hdr, oracle, nz):
    """the misplaced charges of a permuted-id node change the score: the equal-id node runs out of whole pairs, the permuted one never"""
    _, raw = _oracle(oracle, hdr, TC.least_numa_greedy_case(nz), "LeastNUMANodes")
    assert raw[0, 2] < raw[0, 0] and raw[0, 0] == 82


def test_mix_case_shapes(hdr, oracle):
    for n_nodes, count in ((71, 1), (97, 64), (101, 65)):
        cols = TC.spread_cols(n_nodes, count)
        assert len(cols) == count and n_nodes % 64 != 0
        c = TC.mix_case(n_nodes, cols, [9, 16, 17, 32, 33, 64], seed=count)
        assert TC.n_tall(c) == count
        if count >= 4:
            assert 0 in cols and n_nodes - 1 in cols and any(b - a == 1 for a, b in zip(cols, cols[1:]))
    st, raw = _oracle(oracle, hdr, c)
    tall = np.array(cols)
    assert len(set(st[:, tall].ravel().tolist())) >= 4 and (raw[:6, tall] > 0).any() and (raw[:6, tall] == 0).any()


@pytest.mark.parametrize("name", sorted(TC.least_numa_gpu_cases()))
def test_oracle_cost_of_every_least_numa_gpu_case(hdr, oracle, name):
    """the oracle side of each LeastNUMANodes example the GPU tests run stays within a few seconds on the CPU"""
    c = TC.least_numa_gpu_cases()[name]()
    t0 = time.perf_counter()
    _, raw = _oracle(oracle, hdr, c, "LeastNUMANodes")
    took = time.perf_counter() - t0
    print(f"{name}: {took:.2f} s")
    assert took < 5.0
    assert (raw < 100).any()
