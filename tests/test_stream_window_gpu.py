"""GPU: the streaming front / back end at window lengths other than 40 (csrc/tip_stream_w.hip, the tip_stream_*_w family of
include/tip_hip.h, streaming.StreamingEngine / StaggeredStreamingEngine(window=W)) against traces of the REAL
RTRunnerMin(char, model, max_input_l = W, ...) (tests/golden/tip_runner_window_golden.npz: W = 1, 7, 24, 41, 64) and, where no trace
exists, against oracle/streaming_oracle.py:StreamOracle(max_len=W), which tests/test_stream_window_cpu.py pins to the same file.

    W = 1    one-slot rings                                  W = 41   one past the old constant and past ACC_SUM_WIN_LEN
    W = 7    between the 6-tap filter and the 11-tap smoother W = 64   acc-sum over the newest 40 rows of a longer window
    W = 24   acc-sum over fewer than 40 rows                  W = 2, 39, 128 (oracle): the layout's edges, the other side of 40
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import tip_amd
from tip_amd import synth
from tip_amd import lib as tlib
from conftest import ROOT
from oracle.streaming_oracle import StreamOracle, aa_to_rot6d
from test_host_cpu import make_model, load_synth
from test_stream_window_cpu import WINDOWS, block_floats, load_window_traces

pytestmark = pytest.mark.gpu
RUNNER_GOLDEN = os.path.join(ROOT, "tests", "golden", "tip_runner_golden.npz")
TOL_IO = 1e-4      # tests/test_streaming_gpu.py: fp32 device arithmetic vs the reference's float64 numpy, teacher-forced
TOL_LOOP = 5e-4    # tests/test_streaming_gpu.py: closed loop (fp32 feedback through the network)
AUTO = tlib.TIP_STREAM_FRAME_AUTO
StreamingEngine, StaggeredStreamingEngine = tip_amd.streaming.StreamingEngine, tip_amd.streaming.StaggeredStreamingEngine


@pytest.fixture(scope="module")
def traces():
    return load_window_traces()


_paper = {}


def _model(p_state=0.0, train=False):
    key = (p_state, train)
    if key not in _paper:
        m = make_model(synth.PAPER, p_state=p_state) if p_state else make_model(synth.PAPER)
        load_synth(m, synth.PAPER, 0)
        m = m.cuda()
        _paper[key] = m.train() if train else m.eval()
    m = _paper[key]
    m.set_plan("auto")
    return m


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


class Buffers:
    """A state buffer of n streams at window W, reset through tip_stream_reset_w, with windows and outputs of the paper's shape."""

    def __init__(self, n, W, s_init, slots=False):
        self.lib, self.n, self.W = tlib.load(), n, W
        nb = ctypes.c_size_t()
        assert self.lib.tip_stream_state_bytes_w(n, W, ctypes.byref(nb)) == 0 and nb.value == n * block_floats(W) * 4
        self.state = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        self.s_init = _dev(np.asarray(s_init, dtype=np.float32).reshape(n, 114))
        assert self.lib.tip_stream_reset_w(self.state.data_ptr(), self.s_init.data_ptr(), n, 5, 1, W, _st()) == 0
        self.x_imu = torch.full((n, W, 90), 7.0, device="cuda")
        self.x_s = torch.full((n, W, 131), 7.0, device="cuda")
        self.s_rest = torch.zeros(n, 111, device="cuda")
        self.c_t = torch.zeros(n, 20, device="cuda")
        self.rows = torch.full((n,), -7, dtype=torch.int32, device="cuda")

    def ingest(self, raw, f, window=None):
        """Lock-step tip_stream_ingest_w; returns (x_imu [n,T,90], x_s [n,T,131]) or None while priming."""
        W = self.W if window is None else window
        raw = _dev(raw).reshape(self.n, 72)
        assert self.lib.tip_stream_ingest_w(self.state.data_ptr(), raw.data_ptr(), self.n, f, self.x_imu.data_ptr(), self.x_s.data_ptr(),
                                            W, _st()) == 0
        T = self.lib.tip_stream_window_len_w(f, W)
        if T == 0:
            return None
        return (self.x_imu.view(-1)[: self.n * T * 90].view(self.n, T, 90), self.x_s.view(-1)[: self.n * T * 131].view(self.n, T, 131))

    def consume(self, y, k):
        y = _dev(y).reshape(self.n, 131)
        assert self.lib.tip_stream_consume_w(self.state.data_ptr(), y.data_ptr(), self.n, k, self.s_rest.data_ptr(), self.c_t.data_ptr(),
                                             self.W, _st()) == 0


# ---- 1. teacher-forced through the C-ABI against the reference runner --------------------------------------------------------------
@pytest.mark.parametrize("W", WINDOWS)
def test_teacher_forced_matches_reference_runner_at_window(traces, W):
    """The form and bound of tests/test_streaming_gpu.py::test_teacher_forced_matches_reference_runner: every call's newest x_imu /
    x_s row, the stored full windows, every frame's s_rest / c_t; SBP flags exact."""
    tr = traces[W]
    B = Buffers(1, W, tr["s_init"])
    k, worst = 0, {"x_imu": 0.0, "x_s": 0.0, "pose": 0.0}
    for f in range(2 * W + 16):
        win = B.ingest(tr["raw_imu"][f], f)
        if win is None:
            assert f < 5
            continue
        T = int(tr["call_T"][k])
        assert win[0].shape == (1, T, 90) and win[1].shape == (1, T, 131)
        xi, xs = win[0][0].cpu().numpy(), win[1][0].cpu().numpy()
        worst["x_imu"] = max(worst["x_imu"], np.abs(xi[-1] - tr["x_imu_last_rows"][k]).max())
        worst["x_s"] = max(worst["x_s"], np.abs(xs[-1] - tr["x_s_last_rows"][k]).max())
        assert np.abs(xi[-1] - tr["x_imu_last_rows"][k]).max() < TOL_IO, (f, "x_imu")
        assert np.abs(xs[-1] - tr["x_s_last_rows"][k]).max() < TOL_IO, (f, "x_s")
        if f"x_imu_call{k}" in tr:
            assert np.abs(xi - tr[f"x_imu_call{k}"]).max() < TOL_IO, (f, "x_imu window")
            assert np.abs(xs - tr[f"x_s_call{k}"]).max() < TOL_IO, (f, "x_s window")
        B.consume(tr["y_last_rows"][k], k)
        s_rest, c_t = B.s_rest[0].cpu().numpy(), B.c_t[0].cpu().numpy()
        worst["pose"] = max(worst["pose"], np.abs(s_rest - tr["qdq_rest"][f]).max())
        assert np.abs(s_rest - tr["qdq_rest"][f]).max() < TOL_IO, f
        assert np.array_equal(c_t[0::4], tr["ct"][f][0::4])
        assert np.abs(c_t - tr["ct"][f]).max() < TOL_IO
        k += 1
    assert k == 2 * W + 11
    print(f"W={W}: teacher-forced worst errors:", worst)


# ---- 2. the same loop against the oracle where no trace exists ---------------------------------------------------------------------
@pytest.mark.parametrize("W", [2, 39, 128])
def test_teacher_forced_matches_oracle_at_window(traces, W):
    """Synthetic frames (the 64-trace's, cycled past its 144) and one pseudo-random y_last per call, drawn once: no forward.  Every
    window row, not just the newest, every frame."""
    F = 2 * W + 16
    src = traces[64]
    raw = src["raw_imu"][np.arange(F) % src["raw_imu"].shape[0]]
    ys = np.random.RandomState(W).randn(F, 131).astype(np.float32) * 0.5
    o = StreamOracle(src["s_init"], max_len=W)
    B = Buffers(1, W, src["s_init"])
    k = 0
    for f in range(F):
        win = B.ingest(raw[f], f)
        ready = o.ingest(raw[f])
        assert ready == (win is not None)
        if win is None:
            continue
        x_imu, x_s = o.build_inputs()
        assert win[0].shape[1:] == x_imu.shape and win[1].shape[1:] == x_s.shape and x_imu.shape[0] == min(k + 1, W)
        assert np.abs(win[0][0].cpu().numpy() - x_imu).max() < TOL_IO, (f, "x_imu")
        assert np.abs(win[1][0].cpu().numpy() - x_s).max() < TOL_IO, (f, "x_s")
        s_rest, c_t = o.consume(ys[k])
        B.consume(ys[k], k)
        assert np.abs(B.s_rest[0].cpu().numpy() - s_rest).max() < TOL_IO, f
        got = B.c_t[0].cpu().numpy()
        assert np.array_equal(got[0::4], c_t[0::4]) and np.abs(got - c_t).max() < TOL_IO
        k += 1
    assert k == F - 5


# ---- 3. closed loop: StreamingEngine(window=W) with the HIP forward inside ---------------------------------------------------------
@pytest.mark.parametrize("W", [7, 41, 64])
def test_closed_loop_engine_tracks_reference_runner_at_window(traces, W):
    tr = traces[W]
    m = _model()
    eng = StreamingEngine(m, tr["s_init"][None], window=W)
    assert eng.x_imu.shape == (1, W, 90) and eng.x_s.shape == (1, W, 131) and eng.window == W
    n0, worst = m.hip_forward_count(), 0.0
    F = 2 * W + 16
    for f in range(F):
        out = eng.step(tr["raw_imu"][f])
        if f < 5:
            assert out is None
            continue
        assert out["T"] == min(f - 4, W)
        e = np.abs(out["s_rest"][0].cpu().numpy() - tr["qdq_rest"][f]).max()
        worst = max(worst, e)
        assert e < TOL_LOOP, (f, e)
        assert np.abs(out["y_last"][0].cpu().numpy() - tr["y_last_rows"][f - 5]).max() < TOL_LOOP, f
    assert m.hip_forward_count() == n0 + F - 5
    print(f"W={W}: closed-loop worst |pose - reference| = {worst:.3e}")


def _raw_frames(B, F, seed=3):
    """The raw-IMU generator of tests/test_streaming_gpu.py (test_graph_mode_equals_launch_by_launch)."""
    from scipy.spatial.transform import Rotation
    rng = np.random.RandomState(seed)
    raw = np.zeros((F, B, 72), dtype=np.float32)
    for f in range(F):
        raw[f, :, :54] = Rotation.random(B * 6, random_state=100 + f).as_matrix().reshape(B, 54)
        raw[f, :, 54:] = rng.randn(B, 18)
    return raw, rng.randn(B, 114).astype(np.float32) * 0.2


# ---- 4. graph mode -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [24, 64])
def test_graph_mode_equals_launch_by_launch_at_window(W):
    """W + 12 frames: capture at frame W + 4, eight replays."""
    m = _model()
    F = W + 12
    raw, s_init = _raw_frames(2, F)
    ref, eng = StreamingEngine(m, s_init, window=W), StreamingEngine(m, s_init, use_graph=True, window=W)
    for f in range(F):
        a, b = ref.step(raw[f]), eng.step(raw[f])
        assert (a is None) == (b is None) == (f < 5)
        assert (eng._graph is not None) == (f >= W + 4)
        if a is None:
            continue
        torch.cuda.synchronize()
        assert a["T"] == b["T"] == min(f - 4, W)
        for k in ("s_rest", "c_t", "y_last"):
            assert torch.equal(a[k], b[k]), (f, k)
        assert torch.isfinite(b["y_last"]).all()
    assert eng.captures == 1
    assert torch.equal(ref.state, eng.state)
    m.check_handoffs()


# ---- 5. staggered and mapped windows -----------------------------------------------------------------------------------------------
def test_staggered_and_mapped_windows_match_lockstep_at_window_7(traces):
    """n = 3, W = 7; slots attached at frames 0, 3 and 9, slot 1 detached at 14 and re-attached at 17; 26 frames, each slot fed the
    7-trace's frames from its own frame 0 and teacher-forced with its y rows.  Against a one-stream lock-step buffer per slot."""
    lib, W, n, F = tlib.load(), 7, 3, 26
    tr = traces[W]
    starts = {0: [0], 1: [3, 17], 2: [9]}
    stops = {1: [14]}

    def age(i, g):
        """slot i's own frame index at global frame g, None while detached"""
        s = [a for a in starts[i] if a <= g]
        if not s or any(s[-1] < d <= g for d in stops.get(i, [])):
            return None
        return g - s[-1]

    stag, mapd = Buffers(n, W, np.tile(tr["s_init"], (n, 1))), Buffers(n, W, np.tile(tr["s_init"], (n, 1)))
    y_slot = torch.full((n, 131), float("nan"), device="cuda")
    rows_slot = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    solo = {}
    s_one = _dev(tr["s_init"][None])
    for g in range(F):
        att = [i for i in range(n) if g in starts[i]]
        det = [i for i in range(n) if g in stops.get(i, [])]
        for B in (stag, mapd):
            if att:
                sl, rows = _dev(att, torch.int32), _dev(np.tile(tr["s_init"], (len(att), 1)))
                assert lib.tip_stream_attach_w(B.state.data_ptr(), n, sl.data_ptr(), rows.data_ptr(), len(att), W, _st()) == 0
            if det:
                sl = _dev(det, torch.int32)
                assert lib.tip_stream_detach_w(B.state.data_ptr(), n, sl.data_ptr(), len(det), W, _st()) == 0
        for i in att:
            solo[i] = Buffers(1, W, tr["s_init"])
        ages = [age(i, g) for i in range(n)]
        raw = np.stack([tr["raw_imu"][a if a is not None else 0] for a in ages]).astype(np.float32)
        rd = _dev(raw)
        perm = [2, 0, 1]                                         # position -> slot
        sa = _dev(perm, torch.int32)
        assert lib.tip_stream_ingest_staggered_w(stag.state.data_ptr(), rd.data_ptr(), n, stag.x_imu.data_ptr(), stag.x_s.data_ptr(),
                                                 stag.rows.data_ptr(), W, _st()) == 0
        assert lib.tip_stream_ingest_mapped_w(mapd.state.data_ptr(), rd.data_ptr(), n, sa.data_ptr(), n, mapd.x_imu.data_ptr(),
                                              mapd.x_s.data_ptr(), mapd.rows.data_ptr(), W, _st()) == 0
        y = np.zeros((n, 131), dtype=np.float32)
        for i in range(n):
            a = ages[i]
            T = 0 if a is None else lib.tip_stream_window_len_w(a, W)
            assert int(stag.rows[i]) == T - 1 == int(mapd.rows[perm.index(i)]), (g, i)
            if a is not None:
                win = solo[i].ingest(tr["raw_imu"][a], a)
            for name, width in (("x_imu", 90), ("x_s", 131)):
                got, gotm = getattr(stag, name)[i], getattr(mapd, name)[perm.index(i)]
                assert torch.equal(got, gotm), (g, i, name)
                assert not got[T:].any(), (g, i, name)            # rows T_i .. W-1 are zero
                if T:
                    assert torch.equal(got[:T], win[0 if name == "x_imu" else 1][0]), (g, i, name)
            if T:
                y[i] = tr["y_last_rows"][a - 5]
                solo[i].consume(y[i], a - 5)
        yd = _dev(y)
        assert lib.tip_stream_consume_staggered_w(stag.state.data_ptr(), yd.data_ptr(), stag.rows.data_ptr(), n, stag.s_rest.data_ptr(),
                                                  stag.c_t.data_ptr(), W, _st()) == 0
        yp = yd[torch.tensor(perm).cuda()].contiguous()
        assert lib.tip_stream_consume_mapped_w(mapd.state.data_ptr(), yp.data_ptr(), mapd.rows.data_ptr(), sa.data_ptr(), n, n,
                                               mapd.s_rest.data_ptr(), mapd.c_t.data_ptr(), y_slot.data_ptr(), rows_slot.data_ptr(),
                                               W, _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(stag.state, mapd.state) and torch.equal(stag.s_rest, mapd.s_rest) and torch.equal(stag.c_t, mapd.c_t)
        for i in range(n):
            if ages[i] is not None and ages[i] >= 5:
                assert torch.equal(stag.s_rest[i], solo[i].s_rest[0]) and torch.equal(stag.c_t[i], solo[i].c_t[0]), (g, i)
                assert np.abs(stag.s_rest[i].cpu().numpy() - tr["qdq_rest"][ages[i]]).max() < TOL_IO
                assert torch.equal(y_slot[i], yd[i]) and int(rows_slot[i]) == int(stag.rows[i])
    assert age(1, F - 1) == F - 1 - 17 and age(1, 15) is None


def _run_staggered(m, raw, s_init, ev, compact, W):
    eng = StaggeredStreamingEngine(m, s_init, compact=compact, window=W)
    assert eng.x_imu.shape[1] == W
    outs = []
    for f in range(raw.shape[0]):
        det, att = ev.get(f, ([], []))
        eng.detach(det)
        eng.attach(att, s_init[att])
        o = eng.step(raw[f])
        outs.append({k: o[k].clone() for k in ("s_rest", "c_t", "y_last", "T", "valid")})
    torch.cuda.synchronize()
    return outs


EVENTS = {0: ([1, 2, 4], []), 3: ([], [1]), 9: ([0], [2]), 20: ([3], [0, 4]), 30: ([1], []), 33: ([], [1])}


def test_staggered_engines_plain_and_compact_at_window_24_are_bit_identical_on_the_pinned_plan():
    """The existing equality (tests/test_stream_pool_gpu.py, contract 2) at a new length."""
    m = _model()
    n, F, W = 5, 2 * 24 + 8, 24
    raw, s_init = _raw_frames(n, F, seed=5)
    m.set_plan("fused")
    try:
        a, b = _run_staggered(m, raw, s_init, EVENTS, False, W), _run_staggered(m, raw, s_init, EVENTS, True, W)
    finally:
        m.set_plan("auto")
    for f in range(F):
        for k in a[f]:
            assert torch.equal(a[f][k].nan_to_num(7.0), b[f][k].nan_to_num(7.0)), (f, k)
    assert int(a[-1]["T"].max()) == W and bool(a[-1]["valid"].any()) and not bool(a[-1]["valid"].all())


def test_staggered_engines_plain_and_compact_at_window_64_agree_under_auto():
    m = _model()
    n, F, W = 5, 64 + 16, 64
    raw, s_init = _raw_frames(n, F, seed=6)
    a, b = _run_staggered(m, raw, s_init, EVENTS, False, W), _run_staggered(m, raw, s_init, EVENTS, True, W)
    for f in range(F):
        assert torch.equal(a[f]["T"], b[f]["T"]) and torch.equal(a[f]["valid"], b[f]["valid"])
        v = a[f]["valid"]
        for k in ("s_rest", "c_t", "y_last"):
            if bool(v.any()):
                assert float((a[f][k][v] - b[f][k][v]).abs().max()) < TOL_LOOP, (f, k)
    assert int(a[-1]["T"].max()) == W


# ---- 6. override_history after the ring has wrapped --------------------------------------------------------------------------------
def test_override_history_at_window_7_after_the_ring_wrapped():
    """As tests/test_stream_shapes_gpu.py::test_override_history_touches_only_the_pose_columns_of_one_row, at W = 7 and frame 20."""
    m = _model()
    W, n, F = 7, 3, 21
    raw, s_init = _raw_frames(n, F + 1, seed=9)
    eng = StreamingEngine(m, s_init, window=W)
    for f in range(F):
        eng.step(raw[f])
    torch.cuda.synchronize()
    stride, hist = block_floats(W), 3 + 11 * 72 + W * 72 + W * 18        # csrc/tip_stream_w.hip: stream_lay
    before = eng.state.clone().view(torch.float32).view(n, stride).cpu()
    q = np.random.RandomState(1).randn(2, 54).astype(np.float32) * 0.4
    sel = (0, 2)
    eng.override_history(q, sel)
    torch.cuda.synchronize()
    after = eng.state.view(torch.float32).view(n, stride).cpu()
    k = F - 1 - 5
    row = hist + ((k + 1) % W) * 131
    changed = torch.zeros(n, stride, dtype=torch.bool)
    for s in sel:
        changed[s, row: row + 108] = True
    assert torch.equal(after.view(torch.int32)[~changed], before.view(torch.int32)[~changed])
    for j, s in enumerate(sel):
        got = after[s, row: row + 108].numpy()
        assert np.abs(got - aa_to_rot6d(q[j].astype(np.float64))).max() < 2e-6
        assert not np.array_equal(got, before[s, row: row + 108].numpy())
    out = eng.step(raw[F])
    torch.cuda.synchronize()
    assert out["T"] == W
    for s in range(n):
        assert torch.equal(eng.x_s[s, W - 1, :108].cpu(), after[s, row: row + 108])
        assert torch.equal(eng.x_s[s, W - 1, 108:].cpu(), before[s, row + 108: row + 131])


# ---- 7. the layout guard -----------------------------------------------------------------------------------------------------------
def test_layout_guard_answers_with_nan_and_touches_nothing(traces):
    lib, tr = tlib.load(), traces[24]
    B = Buffers(1, 24, tr["s_init"])
    for f in range(9):
        B.ingest(tr["raw_imu"][f], f)
        if f >= 5:
            B.consume(tr["y_last_rows"][f - 5], f - 5)
    twin = Buffers(1, 24, tr["s_init"])                      # the same frames, never misused
    for f in range(9):
        twin.ingest(tr["raw_imu"][f], f)
        if f >= 5:
            twin.consume(tr["y_last_rows"][f - 5], f - 5)
    torch.cuda.synchronize()
    copy = B.state.clone()
    win = B.ingest(tr["raw_imu"][9], 9, window=7)            # T = 5 at either length
    torch.cuda.synchronize()
    assert win[0].shape == (1, 5, 90) and torch.isnan(win[0]).all() and torch.isnan(win[1]).all()
    assert torch.equal(B.state, copy)
    y = _dev(tr["y_last_rows"][4][None])
    s_rest0 = B.s_rest.clone()
    rd, sl = _dev(tr["raw_imu"][9][None]), _dev([0], torch.int32)
    S = B.state.data_ptr()
    assert lib.tip_stream_consume_w(S, y.data_ptr(), 1, 4, B.s_rest.data_ptr(), B.c_t.data_ptr(), 7, _st()) == 0
    assert lib.tip_stream_history_override_w(S, 1, sl.data_ptr(), y.data_ptr(), 1, 7, _st()) == 0
    assert lib.tip_stream_attach_w(S, 1, sl.data_ptr(), B.s_init.data_ptr(), 1, 7, _st()) == 0
    assert lib.tip_stream_detach_w(S, 1, sl.data_ptr(), 1, 7, _st()) == 0
    xi, xs = torch.zeros(1, 7, 90, device="cuda"), torch.zeros(1, 7, 131, device="cuda")
    assert lib.tip_stream_ingest_staggered_w(S, rd.data_ptr(), 1, xi.data_ptr(), xs.data_ptr(), B.rows.data_ptr(), 7, _st()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(xi).all() and torch.isnan(xs).all() and int(B.rows[0]) == -1
    B.rows.fill_(5)
    assert lib.tip_stream_ingest_mapped_w(S, rd.data_ptr(), 1, sl.data_ptr(), 1, xi.data_ptr(), xs.data_ptr(), B.rows.data_ptr(), 7,
                                          _st()) == 0
    torch.cuda.synchronize()
    assert int(B.rows[0]) == -1 and torch.equal(B.state, copy) and torch.equal(B.s_rest, s_rest0)
    # a following correct call is unaffected
    a, b = B.ingest(tr["raw_imu"][9], 9), twin.ingest(tr["raw_imu"][9], 9)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.isfinite(a[0]).all()
    B.consume(tr["y_last_rows"][4], 4), twin.consume(tr["y_last_rows"][4], 4)
    torch.cuda.synchronize()
    assert torch.equal(B.state, twin.state) and torch.equal(B.s_rest, twin.s_rest)
    assert np.abs(B.s_rest[0].cpu().numpy() - tr["qdq_rest"][9]).max() < TOL_IO


# ---- 8. window = 40 through the new names is the old path --------------------------------------------------------------------------
def test_window_40_is_the_old_entry_points_bit_for_bit():
    lib = tlib.load()
    z = np.load(RUNNER_GOLDEN)
    trs = [{k: z[f"stream{i}/{k}"] for k in ("raw_imu", "s_init", "y_last_rows")} for i in range(2)]
    n = 2
    new = Buffers(n, 40, np.stack([t["s_init"] for t in trs]))
    nb = ctypes.c_size_t()
    assert lib.tip_stream_state_bytes(n, ctypes.byref(nb)) == 0 and nb.value == new.state.numel()
    state = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
    assert lib.tip_stream_reset(state.data_ptr(), new.s_init.data_ptr(), n, _st()) == 0
    x_imu, x_s = torch.full((n, 40, 90), 7.0, device="cuda"), torch.full((n, 40, 131), 7.0, device="cuda")
    s_rest, c_t = torch.zeros(n, 111, device="cuda"), torch.zeros(n, 20, device="cuda")
    for f in range(70):
        raw = np.stack([t["raw_imu"][f] for t in trs])
        rd = _dev(raw)
        new.ingest(raw, f)
        assert lib.tip_stream_ingest(state.data_ptr(), rd.data_ptr(), n, f, x_imu.data_ptr(), x_s.data_ptr(), _st()) == 0
        assert lib.tip_stream_window_len(f) == lib.tip_stream_window_len_w(f, 40)
        if f >= 5:
            y = np.stack([t["y_last_rows"][f - 5] for t in trs])
            new.consume(y, f - 5)
            assert lib.tip_stream_consume(state.data_ptr(), _dev(y).data_ptr(), n, f - 5, s_rest.data_ptr(), c_t.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(new.x_imu, x_imu) and torch.equal(new.x_s, x_s), f
        assert torch.equal(new.s_rest, s_rest) and torch.equal(new.c_t, c_t) and torch.equal(new.state, state), f
    # ... and the engine's keyword
    m = _model()
    s_init = np.stack([t["s_init"] for t in trs])
    a, b = StreamingEngine(m, s_init), StreamingEngine(m, s_init, window=40)
    for f in range(70):
        raw = np.stack([t["raw_imu"][f] for t in trs])
        oa, ob = a.step(raw), b.step(raw)
        if oa is not None:
            assert all(torch.equal(oa[k], ob[k]) for k in ("s_rest", "c_t", "y_last")) and oa["T"] == ob["T"]
    torch.cuda.synchronize()
    assert torch.equal(a.state, b.state) and torch.equal(a.x_imu, b.x_imu) and torch.equal(a.x_s, b.x_s)


# ---- 9. live dropout ---------------------------------------------------------------------------------------------------------------
def test_live_dropout_at_window_24_graph_equals_launch_mode():
    from test_live_forward_gpu import P_STATE, P_DROP
    m = _model(p_state=P_STATE, train=True)
    m.ENCODER_DROPOUT = P_DROP
    W, n = 24, 2
    F = W + 12
    raw, s_init = _raw_frames(n, F)
    runs = []
    for use_graph in (False, True):
        torch.manual_seed(7)
        eng = StreamingEngine(m, s_init, use_graph=use_graph, live_dropout=True, window=W)
        outs = []
        for f in range(F):
            o = eng.step(raw[f])
            outs.append(None if o is None else {k: o[k].clone() for k in ("s_rest", "c_t", "y_last")})
        torch.cuda.synchronize()
        runs.append((eng, outs))
    (ea, a), (eb, b) = runs
    assert eb._graph is not None and eb.captures == 1
    for f in range(5, F):
        for k in ("s_rest", "c_t", "y_last"):
            assert torch.equal(a[f][k], b[f][k]), (f, k)
            assert torch.isfinite(a[f][k]).all(), (f, k)
    assert torch.equal(ea.seeds, eb.seeds)
    m.check_handoffs()


def test_live_dropout_refuses_a_window_the_live_forward_does_not_serve():
    m = _model()
    s_init = np.zeros((2, 114), dtype=np.float32)
    for cls in (StreamingEngine, StaggeredStreamingEngine):
        with pytest.raises(ValueError, match="40"):
            cls(m, s_init, live_dropout=True, window=41)
        cls(m, s_init, live_dropout=True, window=40)
