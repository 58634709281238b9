"""QOSSort as one device sort (spx_upload_qos_sort_keys + spx_qos_sort): priority descending, QoS class descending, timestamp
ascending, rows equal in all three keys in ascending row order.  The order is checked pair by pair with the reference's Less
(tests/node_columns_ref.py qos_less) and, whole, against Python's stable sort."""
import numpy as np
import pytest

import node_columns_ref as R
from scheduler_plugins_amd import SpxError, synth
from scheduler_plugins_amd.engine import Engine

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def queue(n, seed, few_keys):
    rng = np.random.default_rng(seed)
    if few_keys:  # many rows equal in all three keys
        prio = rng.integers(-1, 2, n).astype(np.int32)
        ts = rng.integers(0, 3, n).astype(np.int64)
    else:
        prio = rng.choice(np.array([I32_MIN, I32_MIN + 1, -1, 0, 1, 1000, I32_MAX - 1, I32_MAX], dtype=np.int64), n).astype(np.int32)
        ts = rng.choice(np.array([R.INT64_MIN, -(1 << 40), -1, 0, 1, 1 << 40, R.INT64_MAX - 1, R.INT64_MAX], dtype=np.int64), n)
        ts = np.where(rng.random(n) < 0.5, ts, rng.integers(-(1 << 62), 1 << 62, n)).astype(np.int64)
    return prio, rng.integers(1, 4, n).astype(np.uint8), ts


def check(perm, prio, qos, ts):
    n = len(prio)
    assert sorted(perm.tolist()) == list(range(n))
    keys = [(int(prio[i]), int(qos[i]), int(ts[i])) for i in range(n)]
    for x, y in zip(perm[:-1], perm[1:]):
        assert R.qos_less(keys[x], keys[y]) or (keys[x] == keys[y] and x < y), (int(x), keys[x], int(y), keys[y])
    assert perm.tolist() == sorted(range(n), key=lambda i: (-keys[i][0], -keys[i][1], keys[i][2]))  # Python's sort is stable


@pytest.mark.parametrize("n", [1, 2, 64, 65, 1025])
def test_qos_sort(gpu_required, n):
    with Engine(0) as e:
        for seed, few in ((n, False), (n + 1, True)):
            prio, qos, ts = queue(n, seed, few)
            e.upload_qos_sort_keys(prio, qos, ts)
            check(e.qos_sort(), prio, qos, ts)
        # all keys equal: the identity
        e.upload_qos_sort_keys(np.full(n, 7, np.int32), np.full(n, 2, np.uint8), np.full(n, -3, np.int64))
        assert e.qos_sort().tolist() == list(range(n))
        # the extremes of every key against each other
        prio = np.resize(np.array([I32_MIN, I32_MAX, 0], np.int32), n)
        ts = np.resize(np.array([R.INT64_MAX, -5, R.INT64_MIN, 0], np.int64), n)
        qos = np.resize(np.array([1, 3, 2, 3, 1], np.uint8), n)
        e.upload_qos_sort_keys(prio, qos, ts)
        check(e.qos_sort(), prio, qos, ts)


def test_qos_sort_refusals_and_independence(gpu_required, hdr):
    with Engine(0) as e:
        with pytest.raises(SpxError) as ei:
            e.qos_sort()
        assert ei.value.code == -3
        for bad in (0, 4):
            with pytest.raises(SpxError) as ei:
                e.upload_qos_sort_keys([1, 2], [1, bad], [0, 0])
            assert ei.value.code == -1
        # TopologicalSort's result on the same engine is what it was before a QOSSort ran
        snap = synth.network_snapshot(hdr, 64, 300, seed=3, pods_per_group=20)
        e.load_network_objects(snap["nodes"], snap["pods"], snap["appgroups"], snap["nettopo"])
        before = e.sort_queue(snap["pods"]).copy()
        q = synth.node_column_snapshot(1025, seed=3)["qos"]
        e.upload_qos_sort_keys(q["priority"], q["qos"], q["queue_ts"])
        check(e.qos_sort(), q["priority"], q["qos"], q["queue_ts"])
        from scheduler_plugins_amd import lib
        import ctypes as C
        perm = np.zeros(300, np.int32)
        assert lib().spx_sort_keys(e._h, perm.ctypes.data_as(C.POINTER(C.c_int32))) == 0  # the keys uploaded before, untouched
        assert np.array_equal(perm, before)
        assert np.array_equal(e.sort_queue(snap["pods"]), before)
        check(e.qos_sort(), q["priority"], q["qos"], q["queue_ts"])  # and the other way round
