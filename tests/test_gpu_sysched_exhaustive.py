"""SySched at the headline shape, 10 000 nodes x 100 000 pods: every cell of the normalised table against the oracle
(tests/sysched_oracle.py), tolerance 0, and the raw int64 row of every distinct set."""
import numpy as np
import pytest

import sysched_oracle as SO
from scheduler_plugins_amd import synth
from scheduler_plugins_amd.engine import SYSCHED, Engine, mask_of

pytestmark = pytest.mark.gpu


def test_config2_sysched_every_cell(gpu_required, hdr):
    n_nodes, n_pods = 10_000, 100_000
    snap = synth.sysched_snapshot(hdr, n_nodes, n_pods, seed=20260921, n_profiles=32)
    per_set = SO.raw_rows(snap["sets"], snap["host"], snap["residents"])
    norm_set = np.stack([SO.normalize_row(r) for r in per_set]).astype(np.uint8)
    with Engine(0) as e:
        e.load_sysched_objects(snap["objects"])
        e.eval(mask_of(SYSCHED))
        e.sync()
        print(f"config2 sysched: {e.last_eval_ms():.3f} ms, classes {e.sysched_pod_classes()}")
        bad = 0
        for lo in range(0, n_pods, 10_000):
            got = e.all_scores(SYSCHED, lo, lo + 10_000)
            bad += int((got != norm_set[snap["pod_set"][lo:lo + 10_000]]).sum())
        assert bad == 0, f"{bad} of {n_nodes * n_pods} cells differ"
        first = {int(s): p for p, s in reversed(list(enumerate(snap["pod_set"])))}
        for s, p in first.items():
            assert np.array_equal(e.raw(SYSCHED, p), per_set[s]), s
