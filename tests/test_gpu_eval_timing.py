"""spx_last_eval_ms is the device time of the last call's kernels: the engine's own event pair (created without system-scope fences; it
only times) against an outer pair of default events recorded on the engine's stream round the same single call.

The stream is kept busy by a few large fills while the call is enqueued, so that both pairs are taken by packets that the GPU meets back
to back and the host's time inside the call is in neither figure.  Asserted per call: the inner figure is positive, it does not exceed
the outer one by more than the events' resolution, and it falls below the outer one by no more than the call's bound.

The bound on outer - inner: the outer pair adds two packets of its own round the inner pair, so outer - inner is positive by construction.
Measured with this file on the build before the flags changed (default-flag events), outer - inner in ms: see PARENT_GAP_MS.  A timing packet costs 0.0037 ms between two sweeps (tools/micro/evgap.hip: two default-flag hipEventRecords per
step 0.0074 ms; profiles/tlp_pairs/tlp_pairs_ab.md).  A call's bound is the upper end of its spread on that build plus one packet.

Where a call's work sits: spx_eval uploads Allocatable's node tables and broadcasts them BEFORE its first event when they are stale
(prepare_alloc: about 0.05 ms after an upload, and as variable as any copy), and enqueues TargetLoadPacking's first-use work — the
constants, the ambiguity table's memset and its build — AFTER it, in front of the sweep.  The case "first evaluation after an upload"
is about the second: it evaluates Allocatable alone first, so that the first is done, and then brackets the call that runs the
first-use work inside both pairs.

The steady-state step at 1 500 x 512 is shorter than the bound, so a second steady-state case runs at 10 000 x 16 384, where the sweep
writes 166 MB: there an event recorded on the wrong side of the sweep moves the gap by several times the bound, and the inner figure is
also held above the time the table's bytes take at the HBM's peak rate."""
import pytest
import torch

from helpers import ALLOCATABLE, LVRB, TLP
from scheduler_plugins_amd import synth
from scheduler_plugins_amd.engine import Engine, mask_of

pytestmark = pytest.mark.gpu

N_NODES, N_PODS = 1_500, 512
PACKET_MS = 0.0037
# outer - inner in ms on the build before the flags changed: (lowest, highest) of six runs, three each in two sessions on two machines
# ("upload" and "large": one session, three runs).  This build in the same sessions: steady 0.0086 - 0.0091, upload 0.0088 - 0.0089,
# lvrb 0.0086 - 0.0091, empty 0.0080 - 0.0084, decide 0.0085 - 0.0091, large 0.0088 - 0.0090.
PARENT_GAP_MS = {"steady": (0.0098, 0.0102), "upload": (0.0099, 0.0108), "lvrb": (0.0098, 0.0102), "empty": (0.0090, 0.0094),
                 "decide": (0.0096, 0.0103), "large": (0.0099, 0.0101)}
RES_MS = 0.0001  # the timestamps tick at 100 MHz (0.00001 ms); both figures are float32 differences of values below a few ms
HBM_PEAK_BYTES_PER_MS = 8.0e9  # MI355X: 8 TB/s
BOTH = mask_of(ALLOCATABLE, TLP)


class _Rig:
    def __init__(self, hdr, n_engines=1, n_nodes=N_NODES, n_pods=N_PODS):
        self.snap = synth.trimaran_snapshot(hdr, n_nodes, n_pods, seed=5, round_frac=0.1)
        self.stream = torch.cuda.Stream(device=0)
        self.ballast = torch.empty(1 << 30, dtype=torch.uint8, device="cuda:0")
        self.engines = [Engine(0) for _ in range(n_engines)]
        for e in self.engines:
            e.set_stream(self.stream.cuda_stream)
            self.load(e)

    def load(self, e):
        s = self.snap
        e.load_trimaran_objects(s["nodes"], s["rc"], s["pods"], s["metrics"], s["assigned"])

    def close(self):
        for e in self.engines:
            e.close()

    def busy(self):
        with torch.cuda.stream(self.stream):
            for _ in range(8):
                self.ballast.fill_(1)

    def bracket(self, call):
        """records an outer pair round call() on the busy stream; returns the pair"""
        o0, o1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        o0.record(self.stream)
        call()
        o1.record(self.stream)
        return o0, o1

    def check(self, name, e, pair, kind):
        pair[1].synchronize()
        outer = pair[0].elapsed_time(pair[1])
        inner = e.last_eval_ms()
        print(f"{name}: inner {inner:.4f} ms, outer {outer:.4f} ms, outer - inner {outer - inner:.4f} ms")
        assert inner > 0.0, (name, inner)
        assert inner <= outer + RES_MS, (name, inner, outer)
        assert outer - inner <= PARENT_GAP_MS[kind][1] + PACKET_MS, (name, inner, outer, PARENT_GAP_MS[kind][1] + PACKET_MS)
        return inner


@pytest.fixture(scope="module")
def rig(gpu_required, hdr):
    r = _Rig(hdr)
    yield r
    r.close()


def test_steady_state_step(rig):
    """config #2's shape: after the first evaluations the step is one dispatch"""
    e = rig.engines[0]
    for _ in range(3):
        e.eval(BOTH)
    e.sync()
    rig.busy()
    rig.check("steady state", e, rig.bracket(lambda: e.eval(BOTH)), "steady")


def test_first_evaluation_after_an_upload(rig):
    """TargetLoadPacking's constants, the ambiguity table's memset and its build run in front of the sweep, between the engine's two events;
    Allocatable's own upload work, which spx_eval enqueues before its first event, is done by the evaluation of Allocatable alone"""
    e = rig.engines[0]
    rig.load(e)
    e.eval(mask_of(ALLOCATABLE))
    e.sync()
    rig.busy()
    rig.check("after an upload", e, rig.bracket(lambda: e.eval(BOTH)), "upload")


def test_step_that_ends_in_lvrb(rig):
    e = rig.engines[0]
    mask = mask_of(ALLOCATABLE, TLP, LVRB)
    e.eval(mask)
    e.sync()
    rig.busy()
    rig.check("Allocatable + TLP + LVRB", e, rig.bracket(lambda: e.eval(mask)), "lvrb")


def test_empty_row_range(rig):
    e = rig.engines[0]
    e.eval(BOTH)
    e.sync()
    rig.busy()
    rig.check("empty row range", e, rig.bracket(lambda: e.eval(BOTH, 7, 7)), "empty")


def test_decide(rig):
    e = rig.engines[0]
    e.decide(BOTH)
    e.sync()
    rig.busy()
    rig.check("decide", e, rig.bracket(lambda: e.decide(BOTH)), "decide")


def test_steady_state_step_large(gpu_required, hdr):
    """10 000 x 16 384: the sweep is several times the bound, and not shorter than its table's bytes at the HBM's peak rate"""
    r = _Rig(hdr, n_nodes=10_000, n_pods=16_384)
    try:
        e = r.engines[0]
        for _ in range(3):
            e.eval(BOTH)
        e.sync()
        r.busy()
        inner = r.check("steady state, large", e, r.bracket(lambda: e.eval(BOTH)), "large")
        floor = 10_000 * 16_384 / HBM_PEAK_BYTES_PER_MS
        assert inner >= floor, (inner, floor)
    finally:
        r.close()


def test_two_engines_alternating_on_one_stream(gpu_required, hdr):
    r = _Rig(hdr, n_engines=2)
    try:
        a, b = r.engines
        for e in (a, b):
            e.eval(BOTH)
            e.sync()
        r.busy()
        pairs = [(e, r.bracket(lambda e=e: e.eval(BOTH))) for e in (a, b, a, b)]
        # each engine's figure is its own last call's, whatever the other enqueued behind it
        r.check("engine a, second call", a, pairs[2][1], "steady")
        r.check("engine b, second call", b, pairs[3][1], "steady")
    finally:
        r.close()
