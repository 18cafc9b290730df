"""GPU: one stream's broken sensor in the streaming engines (streaming.py, csrc/tip_stream.hip).  Five streams run 60 frames with the
paper model; the raw IMU row of stream 2 is NaN (or +Inf) at frame 20.  The state block holds raw, local, acc-sum and history rings,
the reuse ring a frame's rows for the next 39 calls, a captured graph its own workspace: whatever the bad frame leaves in any of them
must stay in that stream:
  * every other stream's s_rest, c_t and y_last equal the clean run bit for bit at every frame;
  * the poisoned stream's y_last is NaN at every frame whose window holds a bad smoothed frame — the span comes from the front end of
    oracle/streaming_oracle.py (real_time_runner_minimal.py:59-76, :131-147), not from the engine — and the clean run's before;
  * the reuse engine equals the recomputing engine bit for bit (under nan_to_num), the poisoned stream included;
  * after reset(), or detach + attach of that slot, the stream equals a clean one.
Recovery over time is not asserted: the reference averages with the previous pose (:165-166), a NaN root velocity lasts for ever.
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import tip_amd
from tip_amd import synth
from tip_amd import lib as tlib
from oracle.streaming_oracle import StreamOracle
from test_host_cpu import make_model, load_synth
from test_reuse_gpu import _raw_frames

pytestmark = pytest.mark.gpu
N, F, BAD, F0 = 5, 60, 2, 20          # streams, frames, the poisoned stream, the frame its raw row is bad
KEYS = ("s_rest", "c_t", "y_last")
VALUES = {"nan": float("nan"), "inf": float("inf")}


def _model(**kw):
    m = make_model(synth.PAPER, **kw)
    load_synth(m, synth.PAPER, 0)
    return m.cuda().eval()


def _frames(value, F=F):
    raw, s_init = _raw_frames(N, F, 31)
    bad = raw.copy()
    bad[F0, BAD, :] = value
    return raw, bad, s_init


def _bad_span(bad_raw, s_init):
    """Frames at which the poisoned stream's window holds a non-finite x_imu entry: the reference front end on that stream alone."""
    o = StreamOracle(s_init[BAD].astype(np.float64))
    span = []
    for f in range(bad_raw.shape[0]):
        if not o.ingest(bad_raw[f, BAD].astype(np.float64)):
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")           # numpy's "invalid value" on the NaN it is asked to carry
            x_imu, _ = o.build_inputs()
        if not np.isfinite(x_imu).all():
            span.append(f)
    assert span and span[0] == F0                     # the 11-tap acceleration mean sees the row at once (:66-70)
    return set(span)


def _run(eng, raw, before_step=None):
    """[frame] -> None or {key: numpy copy}."""
    out = []
    for f in range(raw.shape[0]):
        if before_step is not None:
            before_step(f)
        o = eng.step(raw[f])
        torch.cuda.synchronize()
        out.append(None if o is None else {k: o[k].cpu().numpy().copy() for k in KEYS})
    return out


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_streams(clean, got, span, tag):
    others = [b for b in range(N) if b != BAD]
    for f, (c, g) in enumerate(zip(clean, got)):
        assert (c is None) == (g is None), (tag, f)
        if c is None:
            continue
        for k in KEYS:
            assert _same_bits(c[k][others], g[k][others]), (tag, f, k, "another stream's output changed")
        if f in span:
            assert np.isnan(g["y_last"][BAD]).all(), (tag, f, "the poisoned stream's row is not NaN in every column")
            assert np.isnan(g["s_rest"][BAD][54:57]).all(), (tag, f, "the host cannot see the bad frame in s_rest[54:57]")
        elif f < F0:
            for k in KEYS:
                assert _same_bits(c[k][BAD], g[k][BAD]), (tag, f, k, "the poisoned stream differs before its bad frame")


def _healthy(m, t0):
    assert tlib.spin_timeouts() == t0
    m.check_handoffs()
    assert not m.is_demoted() and m.demotions == 0 and m.flow_demotions == 0


@pytest.mark.parametrize("value", ["nan", "inf"])
@pytest.mark.parametrize("mode", ["launch", "graph", "live"])
def test_lockstep_engine_keeps_a_bad_sensor_in_its_stream(mode, value):
    raw, bad, s_init = _frames(VALUES[value])
    span = _bad_span(bad, s_init)
    live = mode == "live"
    m = _model(p_state=0.8) if live else _model()
    if live:
        m.train()                                     # the model as the reference deploys it: keep mask and encoder dropout live
    t0 = tlib.spin_timeouts()

    def reseed():
        torch.manual_seed(123)                        # live: reset() draws the engine's device seeds from torch's generator

    reseed()
    eng = tip_amd.streaming.StreamingEngine(m, s_init, use_graph=mode == "graph", live_dropout=live)
    clean = _run(eng, raw)
    assert all(np.isfinite(c[k]).all() for c in clean if c is not None for k in KEYS)
    reseed()
    eng.reset()
    _check_streams(clean, _run(eng, bad), span, (mode, value))
    _healthy(m, t0)
    reseed()
    eng.reset()                                       # state block, graph workspace, module workspace: nothing of the bad run is left
    again = _run(eng, raw)
    for f, (c, g) in enumerate(zip(clean, again)):
        assert (c is None) == (g is None) and (c is None or all(_same_bits(c[k], g[k]) for k in KEYS)), (mode, value, f)
    _healthy(m, t0)


@pytest.mark.parametrize("value", ["nan", "inf"])
def test_reuse_engine_equals_recomputation_with_a_bad_sensor(value):
    """The ring keeps the bad frame's in_linear and layer-0 Q / K / V rows for the 39 windows that follow (full windows from frame 44
    on: the bad frames 20 .. are in every one of them).  The recomputing engine runs the two-window encoder there, as
    tests/test_reuse_gpu.py does: the reuse form is that kernel's."""
    raw, bad, s_init = _frames(VALUES[value])
    span = _bad_span(bad, s_init)
    m = _model()
    lib = tlib.load()
    t0 = tlib.spin_timeouts()
    ref = tip_amd.streaming.StreamingEngine(m, s_init)
    eng = tip_amd.streaming.StreamingEngine(m, s_init, reuse=True)

    def plan(f):
        m.set_plan("fused2" if lib.tip_stream_window_len(f) == 40 else "auto")

    clean = _run(eng, raw, plan)
    eng.reset()
    got_ref, got = _run(ref, bad, plan), _run(eng, bad, plan)
    _check_streams(clean, got, span, ("reuse", value))
    for f, (a, b) in enumerate(zip(got_ref, got)):
        assert (a is None) == (b is None)
        if a is not None:
            for k in KEYS:
                assert _same_bits(np.nan_to_num(a[k]), np.nan_to_num(b[k])), ("reuse vs recomputation", value, f, k)
                assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), ("reuse vs recomputation: NaN positions", value, f, k)
    _healthy(m, t0)
    eng.reset()                                       # forgets the ring
    again = _run(eng, raw, plan)
    for f, (c, g) in enumerate(zip(clean, again)):
        assert (c is None) == (g is None) and (c is None or all(_same_bits(c[k], g[k]) for k in KEYS)), (value, f)
    m.set_plan("auto")
    _healthy(m, t0)


@pytest.mark.parametrize("value", ["nan", "inf"])
@pytest.mark.parametrize("compact", [False, True])
def test_staggered_engine_keeps_a_bad_sensor_in_its_slot(compact, value):
    """Every slot attached from frame 0 (its frames are the engine's).  After the bad run the slot is detached and attached again with
    its s_init: it must then be a clean stream from its frame 0, while the other slots run on.  The plan is pinned to one whose
    per-window bits do not depend on the batch or the window position (a compact pool moves the re-attached slot)."""
    G = 50
    raw, bad, s_init = _frames(VALUES[value], F + G)
    span = _bad_span(bad[:F], s_init)
    m = _model()
    m.set_plan("fused")
    t0 = tlib.spin_timeouts()
    eng = tip_amd.streaming.StaggeredStreamingEngine(m, s_init, compact=compact)

    def run(frames):
        out = []
        for f in range(frames.shape[0]):
            o = eng.step(frames[f])
            torch.cuda.synchronize()
            valid = o["valid"].cpu().numpy()
            out.append(None if not valid.any() else {k: o[k].cpu().numpy().copy() for k in KEYS})
            assert valid.all() or not valid.any()
        return out

    clean = run(raw)
    eng.reset()
    got = run(bad[:F])
    _check_streams(clean[:F], got, span, ("staggered", compact, value))
    _healthy(m, t0)
    # the slot restarts; the others go on with frames F .. F + G - 1 of their own
    eng.detach([BAD])
    eng.attach([BAD], s_init[BAD:BAD + 1])
    others = [b for b in range(N) if b != BAD]
    for g in range(G):
        frame = raw[F + g].copy()
        frame[BAD] = raw[g, BAD]
        o = eng.step(frame)
        torch.cuda.synchronize()
        c, cg = clean[F + g], clean[g]
        for k in KEYS:
            v = o[k].cpu().numpy()
            assert _same_bits(v[others], c[k][others]), (compact, value, g, k, "another slot changed after the re-attach")
            if cg is not None:
                assert _same_bits(v[BAD], cg[k][BAD]), (compact, value, g, k, "the re-attached slot is not a clean stream")
    _healthy(m, t0)


def test_consume_keeps_a_nan_prediction_in_its_stream():
    """The back end alone (tip_stream_consume): a NaN y_last row for stream 1 of 3.  The other streams' outputs and state blocks are
    the clean run's bits; that stream's root velocity s_rest[54:57] is NaN — where the host can see it.  Its 17 joint poses stay
    FINITE: polar_two_axis takes its degenerate branch for a NaN prediction (by design: a frame, not a fault); only the averaged root
    velocity and the history row's prediction columns carry the NaN on."""
    lib = tlib.load()
    n, bad_b = 3, 1
    raw, s_init = _raw_frames(n, 12, 5)
    nb = ctypes.c_size_t()
    assert lib.tip_stream_state_bytes(n, ctypes.byref(nb)) == 0
    st = torch.cuda.current_stream().cuda_stream
    ys = torch.tensor(synth.normal(3, "y", 12 * n * 131).reshape(12, n, 131).astype(np.float32) * 0.3).cuda()

    def run(poison):
        state = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        s0 = torch.tensor(s_init).cuda()
        assert lib.tip_stream_reset(state.data_ptr(), s0.data_ptr(), n, st) == 0
        x_imu, x_s = torch.empty(n, 40, 90, device="cuda"), torch.empty(n, 40, 131, device="cuda")
        s_rest, c_t = torch.zeros(n, 111, device="cuda"), torch.zeros(n, 20, device="cuda")
        out = []
        for f in range(12):
            r = torch.tensor(raw[f]).cuda()
            assert lib.tip_stream_ingest(state.data_ptr(), r.data_ptr(), n, f, x_imu.data_ptr(), x_s.data_ptr(), st) == 0
            if lib.tip_stream_window_len(f) == 0:
                continue
            y = ys[f].clone()
            if poison and f == 8:
                y[bad_b] = float("nan")
            assert lib.tip_stream_consume(state.data_ptr(), y.data_ptr(), n, f - 5, s_rest.data_ptr(), c_t.data_ptr(), st) == 0
            torch.cuda.synchronize()
            out.append((f, s_rest.cpu().numpy().copy(), c_t.cpu().numpy().copy(), state.view(n, -1).cpu().numpy().copy()))
        return out

    others = [b for b in range(n) if b != bad_b]
    for (f, s_c, c_c, st_c), (_, s_b, c_b, st_b) in zip(run(False), run(True)):
        assert _same_bits(s_c[others], s_b[others]) and _same_bits(c_c[others], c_b[others]), f
        assert np.array_equal(st_c[others], st_b[others]), (f, "another stream's state block changed")
        if f < 8:
            assert _same_bits(s_c[bad_b], s_b[bad_b]) and np.array_equal(st_c[bad_b], st_b[bad_b])
        else:
            assert np.isnan(s_b[bad_b][54:57]).all(), (f, "NaN root velocity: the host's signal")
        if f == 8:
            joints = s_b[bad_b][3:54]
            print("consume(NaN row): 17 joint poses finite:", bool(np.isfinite(joints).all()), "| root pose equals clean:",
                  _same_bits(s_b[bad_b][:3], s_c[bad_b][:3]), "| joints:", np.round(joints[:6], 4).tolist())
