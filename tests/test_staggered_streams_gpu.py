"""GPU tests of per-stream attach / detach with ragged windows: tip_forward_rows (one chosen output row per window) and the
staggered streaming entry points (csrc/tip_stream.hip, streaming.StaggeredStreamingEngine), against the full forward, the trace of
the REAL reference runner (tests/golden/tip_runner_golden.npz) and the fp64 oracle."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tip_amd
from tip_amd import synth
from tip_amd import lib as tlib
from conftest import ROOT
from test_host_cpu import make_model, load_synth
from oracle import oracle

pytestmark = pytest.mark.gpu
RUNNER_GOLDEN = os.path.join(ROOT, "tests", "golden", "tip_runner_golden.npz")
TOL_IO = 1e-4      # as tests/test_streaming_gpu.py: fp32 device arithmetic vs the reference's float64 numpy, teacher-forced
TOL_LOOP = 5e-4    # closed loop (fp32 feedback through the network)
TOL_PARITY = 2e-5  # the project's parity bound against the fp64 oracle


@pytest.fixture(scope="module")
def trace():
    z = np.load(RUNNER_GOLDEN)
    out = {}
    for k in z.files:
        if "/" not in k:
            continue
        tag, name = k.split("/")
        out.setdefault(tag, {})[name] = z[k]
    return [out["stream0"], out["stream1"]]


@pytest.fixture(scope="module")
def paper():
    cfg = synth.PAPER
    m = make_model(cfg)
    w = load_synth(m, cfg, 0)
    return m.cuda().eval(), w


def _rows(B, seed):
    rng = np.random.RandomState(seed)
    r = rng.randint(0, 40, size=B)
    bad = rng.rand(B) < 0.1
    r[bad] = rng.choice([-1, 40], size=int(bad.sum()))
    if B >= 3:
        r[0], r[1] = -1, 40
    return torch.tensor(r, dtype=torch.int32, device="cuda")


def _check_rows(full, got, rows):
    r = rows.long().cpu()
    ok = (r >= 0) & (r < full.shape[1])
    assert got.shape == (full.shape[0], full.shape[2])
    idx = torch.nonzero(ok).flatten()
    if len(idx):
        assert torch.equal(got.cpu()[idx], full.cpu()[idx, r[idx]])
    bad = torch.nonzero(~ok).flatten()
    if len(bad):
        assert torch.isnan(got.cpu()[bad]).all()


PLANS = [("auto", [1, 3, 9, 24, 40, 100, 256, 300, 1024]),
         ("fused", [1, 3, 40, 300, 1024]),
         ("fusedh", [3, 100, 300]),
         ("fused2", [3, 256, 1024]),
         ("fused1s", [1, 9, 24, 100]),
         ("general", [3, 40, 300]),
         ("latency", [1, 3, 9, 24, 40]),
         ("latency_chain", [1, 9, 24])]


@pytest.mark.parametrize("plan,batches", PLANS, ids=[p for p, _ in PLANS])
def test_forward_rows_equals_full_forward(paper, plan, batches):
    """y[b] == forward(...)[b, rows[b]] bit for bit on every plan the inference forward can take, NaN rows for indices outside
    [0, T); with rows = T - 1 everywhere it is forward_last."""
    m, _ = paper
    h = m._ensure_handle()
    m.set_plan("latency" if plan == "latency_chain" else plan)
    if plan == "latency_chain":
        h.set_option(tlib.TIP_OPT_NO_FLOW, 1)
    try:
        for B in batches:
            x_imu, x_s = synth.make_inputs(synth.PAPER, B, 40, seed=B)
            xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
            rows = _rows(B, B)
            with torch.no_grad():
                full = m(xi, xs)
                got = m.forward_rows(xi, xs, rows)
                last = m.forward_last(xi, xs)
                got39 = m.forward_rows(xi, xs, torch.full((B,), 39, dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            _check_rows(full, got, rows)
            assert torch.equal(got39, last), (plan, B)
    finally:
        h.set_option(tlib.TIP_OPT_NO_FLOW, 0)
        m.set_plan("auto")


def test_forward_rows_without_rnn_keep_mask_and_graph():
    """with_rnn=False (the head reads the encoder output), a supplied past-state keep mask, and one captured-graph replay."""
    cfg = dict(synth.PAPER, with_rnn=False)
    m = make_model(cfg)
    load_synth(m, cfg, 1)
    m = m.cuda().eval()
    for B in (3, 40, 300):
        x_imu, x_s = synth.make_inputs(cfg, B, 40, seed=7)
        xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
        rows = _rows(B, 100 + B)
        with torch.no_grad():
            _check_rows(m(xi, xs), m.forward_rows(xi, xs, rows), rows)

    cfg = synth.PAPER
    m = make_model(cfg, p_state=0.8)
    load_synth(m, cfg, 2)
    m = m.cuda().eval()
    for B in (3, 40, 300):
        x_imu, x_s = synth.make_inputs(cfg, B, 40, seed=8)
        xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
        mask = (torch.rand(B, 40, 131, device="cuda") > 0.8).float()
        rows = _rows(B, 200 + B)
        with torch.no_grad():
            full = m._forward_hip(xi, xs, False, keep_mask=mask)
            got = m._forward_hip(xi, xs, True, keep_mask=mask, rows=rows)
        _check_rows(full, got, rows)
        with torch.no_grad():
            y = m.forward_rows(xi, xs, rows)          # the shipped p = 0.8: a mask is drawn per call
        r = rows.long()
        ok = (r >= 0) & (r < 40)
        assert torch.isfinite(y[ok]).all() and torch.isnan(y[~ok]).all()

    m = make_model(cfg)
    load_synth(m, cfg, 0)
    m = m.cuda().eval()
    B = 40
    x_imu, x_s = synth.make_inputs(cfg, B, 40, seed=9)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    rows = _rows(B, 9)
    ws = torch.empty(m.workspace_bytes(B, 40), dtype=torch.uint8, device="cuda")
    out = torch.empty(B, 131, device="cuda")
    with torch.no_grad():
        eager = m.forward_rows(xi, xs, rows)
        m.forward_rows(xi, xs, rows, workspace=ws, out=out)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            m.forward_rows(xi, xs, rows, workspace=ws, out=out)
        out.fill_(0.0)
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(out.cpu().nan_to_num(7.0), eager.cpu().nan_to_num(7.0))


def _cbuf(n):
    lib = tlib.load()
    nb = ctypes.c_size_t()
    assert lib.tip_stream_state_bytes(n, ctypes.byref(nb)) == 0
    return lib, torch.empty(nb.value, dtype=torch.uint8, device="cuda")


def test_teacher_forced_staggered_matches_reference_runner(trace):
    """C-ABI, three slots: golden stream 0 attached at engine frame 0, golden stream 1 at engine frame 17, slot 2 never.  Every slot
    is fed its trace from its own frame 0 and consumes the reference model's own rows: windows, pad rows, row indices and the
    decoded poses must be the reference runner's."""
    n = 3
    lib, state = _cbuf(n)
    st = torch.cuda.current_stream().cuda_stream
    state.fill_(0xFF)                                    # garbage flags until tip_stream_reset
    s0 = torch.zeros(n, 114, device="cuda")
    assert lib.tip_stream_reset(state.data_ptr(), s0.data_ptr(), n, st) == 0
    x_imu = torch.full((n, 40, 90), float("nan"), device="cuda")
    x_s = torch.full((n, 40, 131), float("nan"), device="cuda")
    rows = torch.empty(n, dtype=torch.int32, device="cuda")
    s_rest = torch.zeros(n, 111, device="cuda")
    c_t = torch.zeros(n, 20, device="cuda")
    start = {0: 0, 1: 17}
    played = {0: 0, 1: 0}
    checked = 0
    for F in range(17 + 70):
        for b, f0 in start.items():
            if F == f0:
                sl = torch.tensor([b], dtype=torch.int32, device="cuda")
                si = torch.tensor(trace[b]["s_init"][None], dtype=torch.float32).cuda()
                assert lib.tip_stream_attach(state.data_ptr(), n, sl.data_ptr(), si.data_ptr(), 1, st) == 0
        if F == 70:                                      # stream 0's trace ends
            sl = torch.tensor([0], dtype=torch.int32, device="cuda")
            assert lib.tip_stream_detach(state.data_ptr(), n, sl.data_ptr(), 1, st) == 0
        raw = np.zeros((n, 72), dtype=np.float32)
        fi = {}
        for b, f0 in start.items():
            if f0 <= F < f0 + 70:
                fi[b] = F - f0
                raw[b] = trace[b]["raw_imu"][fi[b]]
        assert lib.tip_stream_ingest_staggered(state.data_ptr(), torch.tensor(raw).cuda().data_ptr(), n, x_imu.data_ptr(),
                                               x_s.data_ptr(), rows.data_ptr(), st) == 0
        torch.cuda.synchronize()
        r = rows.cpu().numpy()
        xi, xs = x_imu.cpu().numpy(), x_s.cpu().numpy()
        y = np.full((n, 131), np.nan, dtype=np.float32)
        assert r[2] == -1 and not xi[2].any() and not xs[2].any()
        for b in range(2):
            if b not in fi:
                assert r[b] == -1 and not xi[b].any() and not xs[b].any()
                continue
            f, tr = fi[b], trace[b]
            k = f - 5
            if k < 0:
                assert r[b] == -1 and not xi[b].any() and not xs[b].any()
                continue
            T = int(tr["call_T"][k])
            assert r[b] == T - 1, (F, b)
            assert not xi[b, T:].any() and not xs[b, T:].any()        # pad rows exactly zero
            assert np.abs(xi[b, T - 1] - tr["x_imu_last_rows"][k]).max() < TOL_IO
            assert np.abs(xs[b, T - 1] - tr["x_s_last_rows"][k]).max() < TOL_IO
            if f"x_imu_call{k}" in tr:
                assert np.abs(xi[b, :T] - tr[f"x_imu_call{k}"]).max() < TOL_IO
                assert np.abs(xs[b, :T] - tr[f"x_s_call{k}"]).max() < TOL_IO
                checked += 1
            y[b] = tr["y_last_rows"][k]
        before = s_rest.cpu().numpy().copy(), c_t.cpu().numpy().copy()
        yd = torch.tensor(y).cuda()
        assert lib.tip_stream_consume_staggered(state.data_ptr(), yd.data_ptr(), rows.data_ptr(), n, s_rest.data_ptr(),
                                                c_t.data_ptr(), st) == 0
        torch.cuda.synchronize()
        sr, ct = s_rest.cpu().numpy(), c_t.cpu().numpy()
        for b in range(n):
            if r[b] < 0:
                assert np.array_equal(sr[b], before[0][b]) and np.array_equal(ct[b], before[1][b])
                continue
            f, tr = fi[b], trace[b]
            assert np.abs(sr[b] - tr["qdq"][f][3:]).max() < TOL_IO, (F, b)
            assert np.array_equal(ct[b][0::4], tr["ct"][f][0::4])
            assert np.abs(ct[b] - tr["ct"][f]).max() < TOL_IO
            played[b] += 1
    assert played == {0: 65, 1: 65} and checked == 12


def _golden_raw(trace, b, f):
    return trace[b]["raw_imu"][f]


def test_closed_loop_staggered_engine_tracks_reference_runner(trace, paper):
    """StaggeredStreamingEngine with the two golden streams at offsets 0 and 23; stream 0 is detached at frame 50 and re-attached at
    60 to replay its trace from the start.  Every valid frame follows the reference runner; T / valid follow each slot's call_T."""
    m, _ = paper
    s_init = np.stack([t["s_init"] for t in trace])
    eng = tip_amd.streaming.StaggeredStreamingEngine(m, s_init)
    eng.detach([1])
    f0 = {0: 0, 1: 23}
    done = {0: 0, 1: 0}
    worst = 0.0
    F = 0
    while F < 130:
        if F == 23:
            eng.attach([1], s_init[1:2])
        if F == 50:
            eng.detach([0])
        if F == 93:
            eng.detach([1])                              # stream 1's trace ends
        if F == 60:
            eng.attach([0], s_init[0:1])
            f0[0] = 60
        live = {b: F - f0[b] for b in (0, 1) if eng.attached[b] and 0 <= F - f0[b] < 70}
        raw = np.zeros((2, 72), dtype=np.float32)
        for b, f in live.items():
            raw[b] = trace[b]["raw_imu"][f]
        out = eng.step(raw)
        torch.cuda.synchronize()
        T, valid = out["T"].cpu().numpy(), out["valid"].cpu().numpy()
        for b in (0, 1):
            f = live.get(b)
            if f is None or f < 5:
                assert not valid[b] and T[b] == 0, (F, b)
                assert torch.isnan(out["y_last"][b]).all()
                continue
            k = f - 5
            assert valid[b] and T[b] == trace[b]["call_T"][k], (F, b)
            e = np.abs(out["s_rest"][b].cpu().numpy() - trace[b]["qdq"][f][3:]).max()
            worst = max(worst, e)
            assert e < TOL_LOOP, (F, b, e)
            assert np.abs(out["y_last"][b].cpu().numpy() - trace[b]["y_last_rows"][k]).max() < TOL_LOOP
            if f == 69:
                done[b] += 1
        F += 1
    assert done == {0: 1, 1: 1}
    print("staggered closed-loop worst |pose - reference| =", worst)


def _raw_frames(F, n, seed):
    from scipy.spatial.transform import Rotation
    rng = np.random.RandomState(seed)
    raw = np.zeros((F, n, 72), dtype=np.float32)
    base = Rotation.random(n * 6, random_state=seed).as_matrix().reshape(n, 54)
    for f in range(F):
        raw[f, :, :54] = base
        raw[f, :, 54:] = rng.randn(n, 18) * 0.5
    return raw


def test_padded_windows_match_fp64_oracle(paper):
    """At T_i in {1, 7, 31, 39, 40} the slot's y_last is the oracle's last row of its T_i-row window (zero padding behind it)."""
    m, w = paper
    n = 5
    raw = _raw_frames(60, n, 5)
    s_init = np.random.RandomState(6).randn(n, 114).astype(np.float32) * 0.2
    eng = tip_amd.streaming.StaggeredStreamingEngine(m, s_init)
    eng.detach([1, 2, 3, 4])
    starts = {0: 0, 1: 3, 2: 11, 3: 14, 4: 17}
    want = {1, 7, 31, 39, 40}
    seen = set()
    for F in range(60):
        att = [b for b, f0 in starts.items() if F == f0 and b]
        if att:
            eng.attach(att, s_init[att])
        out = eng.step(raw[F])
        torch.cuda.synchronize()
        T = out["T"].cpu().numpy()
        for b in range(n):
            t = int(T[b])
            if t not in want:
                continue
            xi = eng.x_imu[b, :t].double().cpu().numpy()[None]
            xs = eng.x_s[b, :t].double().cpu().numpy()[None]
            yo = oracle.forward(synth.PAPER, w, xi, xs, dtype=np.float64)[0, -1]
            err = np.abs(out["y_last"][b].cpu().numpy() - yo).max()
            assert err < TOL_PARITY, (F, b, t, err)
            seen.add(t)
    assert seen == want


def _schedule(n, F, seed, keep):
    rng = np.random.RandomState(seed)
    ev = []
    for f in range(F):
        det = [int(i) for i in rng.choice(n, 4, replace=False) if i != keep]
        att = [int(i) for i in rng.choice(n, 4, replace=False) if i != keep and i not in det]
        ev.append((det, att))
    return ev


def _run(m, raw, s_init, ev, use_graph=False, poison=False):
    eng = tip_amd.streaming.StaggeredStreamingEngine(m, s_init, use_graph=use_graph)
    if poison:
        eng.x_imu.fill_(float("nan"))
        eng.x_s.fill_(float("nan"))
    outs = []
    for f in range(raw.shape[0]):
        if ev is not None:
            det, att = ev[f]
            eng.detach(det)
            eng.attach(att, s_init[att])
        o = eng.step(raw[f])
        outs.append({k: v.clone() for k, v in o.items()})
    torch.cuda.synchronize()
    return outs


def test_slot_outputs_do_not_depend_on_other_slots(paper):
    """Plan pinned: slot 7's outputs are bit-identical whatever the other 299 slots' attach / detach schedule is."""
    m, _ = paper
    n, F, keep = 300, 50, 7
    raw = _raw_frames(F, n, 8)
    s_init = np.random.RandomState(9).randn(n, 114).astype(np.float32) * 0.2
    m.set_plan("fused")
    try:
        a = _run(m, raw, s_init, _schedule(n, F, 1, keep))
        b = _run(m, raw, s_init, _schedule(n, F, 2, keep))
    finally:
        m.set_plan("auto")
    for f in range(F):
        for k in ("s_rest", "c_t", "y_last", "T", "valid"):
            assert torch.equal(a[f][k][keep].nan_to_num(7.0), b[f][k][keep].nan_to_num(7.0)), (f, k)
    assert bool(a[-1]["valid"][keep])


def test_poisoned_buffers_do_not_leak(paper):
    """NaN-filled window buffers before the first frame, attach and detach events: finite outputs, bit-identical to clean buffers."""
    m, _ = paper
    n, F = 40, 50
    raw = _raw_frames(F, n, 10)
    s_init = np.random.RandomState(11).randn(n, 114).astype(np.float32) * 0.2
    ev = _schedule(n, F, 3, -1)
    a = _run(m, raw, s_init, ev, poison=False)
    b = _run(m, raw, s_init, ev, poison=True)
    for f in range(F):
        v = a[f]["valid"]
        assert torch.equal(v, b[f]["valid"])
        for k in ("s_rest", "c_t", "y_last"):
            assert torch.equal(a[f][k].nan_to_num(7.0), b[f][k].nan_to_num(7.0)), (f, k)
        assert torch.isfinite(b[f]["y_last"][v]).all() and torch.isnan(b[f]["y_last"][~v]).all()
        assert torch.isfinite(b[f]["s_rest"]).all()


@pytest.mark.parametrize("n", [1, 3, 40, 300])
def test_graph_mode_equals_launch_by_launch(paper, n):
    """use_graph=True: one capture at the first step, a replay per frame, attach / detach between replays — bit-identical to the
    launch-by-launch engine over 120 frames."""
    m, _ = paper
    F = 120
    raw = _raw_frames(F, n, 12 + n)
    s_init = np.random.RandomState(13).randn(n, 114).astype(np.float32) * 0.2
    rng = np.random.RandomState(n)
    ev = []
    for f in range(F):
        det = [int(i) for i in range(n) if rng.rand() < 0.03]
        att = [int(i) for i in range(n) if rng.rand() < 0.03 and i not in det]
        ev.append((det, att))
    a = _run(m, raw, s_init, ev, use_graph=False)
    b = _run(m, raw, s_init, ev, use_graph=True)
    for f in range(F):
        for k in ("s_rest", "c_t", "y_last", "T", "valid"):
            assert torch.equal(a[f][k].nan_to_num(7.0), b[f][k].nan_to_num(7.0)), (f, k)
    m.check_handoffs()


def test_refusals_and_handoff_contract(paper, monkeypatch):
    m, _ = paper
    s_init = np.zeros((4, 114), dtype=np.float32)
    m.train()
    with pytest.raises(RuntimeError):
        tip_amd.streaming.StaggeredStreamingEngine(m, s_init)
    m.eval()
    with pytest.raises(RuntimeError):
        tip_amd.streaming.StaggeredStreamingEngine(m, s_init, reuse=True)
    eng = tip_amd.streaming.StaggeredStreamingEngine(m, s_init)
    for bad in ([4], [-1], [1, 1]):
        with pytest.raises(ValueError):
            eng.attach(bad, np.zeros((len(bad), 114), dtype=np.float32))
        with pytest.raises(ValueError):
            eng.detach(bad)
    with pytest.raises(RuntimeError):
        m.forward_rows(torch.zeros(1, 40, 90, device="cuda"), torch.zeros(1, 40, 131, device="cuda"),
                       torch.zeros(1, dtype=torch.int64, device="cuda"))
    raw = _raw_frames(12, 4, 14)
    eng.detach([2])
    for f in range(8):
        out = eng.step(raw[f])
    assert out["valid"].cpu().tolist() == [True, True, False, True]
    # a hand-off loss reported by the model's forward (simulated on the host): every attached slot restarts, then the error
    real = m.forward_rows

    def lossy(*a, **k):
        y = real(*a, **k)
        m.demotions += 1
        return y

    monkeypatch.setattr(m, "forward_rows", lossy)
    d0 = m.demotions
    with pytest.raises(tlib.TipHandoffError):
        eng.step(raw[8])
    monkeypatch.setattr(m, "forward_rows", real)
    m.demotions = d0
    assert eng.attached == [True, True, False, True]
    for f in range(6):
        out = eng.step(raw[9 + f % 3])
        torch.cuda.synchronize()
        assert out["T"].cpu().tolist() == ([0, 0, 0, 0] if f < 5 else [1, 1, 0, 1])
