"""GPU tests of the streaming front / back end at the four model shapes (x_imu 72 | 90 columns, state 119 | 131 columns) and of the
host override of the fed-back pose: csrc/tip_stream.hip, include/tip_hip.h (tip_stream_reset_shaped, tip_stream_history_override),
streaming.py — against traces of the REAL reference runners (tests/golden/tip_runner_shapes_golden.npz), the numpy restatement
pinned to them (tests/test_stream_shapes_cpu.py: ShapedOracle) and the fp64 forward oracle.  Tolerances are the project's own."""
import ctypes

import numpy as np
import pytest
import torch

import tip_amd
from tip_amd import synth
from tip_amd import lib as tlib
from oracle import oracle
from oracle.streaming_oracle import aa_to_rot6d
from test_host_cpu import make_model, load_synth
from test_stream_shapes_cpu import TAGS, ShapedOracle, load_traces

pytestmark = pytest.mark.gpu
TOL_IO = 1e-4      # tests/test_streaming_gpu.py: fp32 device arithmetic vs the reference's float64 numpy, teacher-forced
TOL_LOOP = 5e-4    # tests/test_streaming_gpu.py: closed loop (fp32 feedback through the network)
TOL_TIGHT = 2e-5   # tests/test_hip_parity.py: a forward against the fp64 oracle

CFGS = {"min_noacc_5": dict(synth.TRAIN_DEFAULT), "full_noacc_2": dict(synth.PAPER, size_s=119, with_acc_sum=False),
        "full_acc_2": dict(synth.PAPER, size_s=119), "full_acc_5_ik": dict(synth.PAPER)}
NARROW = dict(synth.PAPER, size_s=119, with_acc_sum=False)        # (72, 119)
# state block layout (csrc/tip_stream.hip, namespace sz), in floats
STRIDE, HIST, OUTS, LAST, CTR, ATT, SHP = 10496, 4392, 9632, 10418, 10472, 10473, 10474


@pytest.fixture(scope="module")
def traces():
    return load_traces()


_models = {}


def _model(cfg):
    key = tuple(sorted(cfg.items()))
    if key not in _models:
        m = make_model(cfg)
        w = load_synth(m, cfg, 0)
        _models[key] = (m.cuda().eval(), w)
    m = _models[key][0]
    m.set_plan("auto")
    m._ensure_handle().set_option(tlib.TIP_OPT_NO_FLOW, 0)
    return m


def _raw_frames(B, F, seed):
    from scipy.spatial.transform import Rotation
    rng = np.random.RandomState(seed)
    raw = np.zeros((F, B, 72), dtype=np.float32)
    for f in range(F):
        raw[f, :, :54] = Rotation.random(B * 6, random_state=1000 * seed + f).as_matrix().reshape(B, 54)
        raw[f, :, 54:] = rng.randn(B, 18)
    return raw, rng.randn(B, 114).astype(np.float32) * 0.2


def _widths(cfg):
    return 72 + (18 if cfg["with_acc_sum"] else 0), cfg["size_s"], cfg["size_s"] - 111


# ---- 1. the plain forward at size_s = 119 ------------------------------------------------------------------------------------------
_oracle_cache = {}


def _oracle_case(acc, T):
    """One batch of windows per (acc-sum, T) and its fp64 oracle output; windows are independent, so a plan tested on B windows
    uses the first B."""
    if (acc, T) not in _oracle_cache:
        cfg = dict(synth.PAPER, size_s=119, with_acc_sum=acc)
        B = 66 if T == 40 else 9
        x_imu, x_s = synth.make_inputs(cfg, B, T, seed=119 + T)
        w = synth.make_weights(cfg, seed=0)
        _oracle_cache[(acc, T)] = (cfg, x_imu, x_s, oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64))
    return _oracle_cache[(acc, T)]


# plan, windows at T = 40, windows at T = 12 (0: the plan serves full windows only)
PLANS_119 = [("general", 5, 5), ("fused", 7, 7), ("fusedh", 7, 7), ("fused2", 5, 0), ("fused1s2", 66, 0), ("fused1s4", 9, 0),
             ("latency", 3, 3), ("latency_chain", 3, 3), ("auto", 66, 9)]


@pytest.mark.parametrize("acc", [True, False], ids=["acc", "noacc"])
@pytest.mark.parametrize("plan,B40,B12", PLANS_119, ids=[p[0] for p in PLANS_119])
def test_forward_parity_at_two_sbps(acc, plan, B40, B12):
    """size_s = 119 (two-SBP models, the 119-column tail of the head kernels) with and without acc-sum on every inference plan AUTO
    can choose: full output, last row and forward_rows against the fp64 oracle."""
    for T, B in ((40, B40), (12, B12)):
        if B == 0:
            continue
        cfg, x_imu, x_s, yo = _oracle_case(acc, T)
        m = _model(cfg)
        h = m._ensure_handle()
        m.set_plan("latency" if plan == "latency_chain" else plan)      # (a pinned plan that does not serve the shape raises)
        h.set_option(tlib.TIP_OPT_NO_FLOW, 1 if plan == "latency_chain" else 0)
        try:
            xi, xs = torch.tensor(x_imu[:B]).cuda(), torch.tensor(x_s[:B]).cuda()
            rows_np = np.random.RandomState(B + T).randint(0, T, size=B)
            rows = torch.tensor(rows_np, dtype=torch.int32, device="cuda")
            n0 = m.hip_forward_count()
            with torch.no_grad():
                full, last, got = m(xi, xs), m.forward_last(xi, xs), m.forward_rows(xi, xs, rows)
            torch.cuda.synchronize()
            assert m.hip_forward_count() == n0 + 3, "the HIP path did not run"
            m.check_handoffs()
            e_full = np.abs(full.cpu().numpy() - yo[:B]).max()
            e_last = np.abs(last.cpu().numpy() - yo[:B, -1]).max()
            e_rows = np.abs(got.cpu().numpy() - yo[np.arange(B), rows_np]).max()
            print(f"size_s 119 acc={acc} plan={plan} B={B} T={T}: full {e_full:.2e} last {e_last:.2e} rows {e_rows:.2e}")
            assert full.shape == (B, T, 119) and np.isfinite(full.cpu().numpy()).all()
            assert e_full < TOL_TIGHT and e_last < TOL_TIGHT and e_rows < TOL_TIGHT, (plan, B, T, e_full, e_last, e_rows)
        finally:
            h.set_option(tlib.TIP_OPT_NO_FLOW, 0)
            m.set_plan("auto")


# ---- 2. teacher-forced through the C-ABI -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(TAGS))
def test_teacher_forced_matches_reference_runners(traces, tag):
    """tip_stream_reset_shaped -> ingest -> consume with the reference model's own outputs: every model input, every decoded pose,
    SBP flags bit-exact.  The buffers are allocated at the widest shape and pre-filled with NaN: what a narrow shape does not write
    stays NaN, what it writes is finite (no column that does not exist is read or written)."""
    tr = traces[tag]
    n_sbps, acc = TAGS[tag]
    nx, ns, nc = 90 if acc else 72, 111 + 4 * n_sbps, 4 * n_sbps
    lib = tlib.load()
    nb = ctypes.c_size_t()
    assert lib.tip_stream_state_bytes(1, ctypes.byref(nb)) == 0
    state = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    s_init = torch.tensor(tr["s_init"][None], dtype=torch.float32).cuda()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.tip_stream_reset_shaped(state.data_ptr(), s_init.data_ptr(), 1, 3, 1, st) == -1
    assert lib.tip_stream_reset_shaped(state.data_ptr(), s_init.data_ptr(), 1, n_sbps, 1 if acc else 0, st) == 0
    nan = float("nan")
    x_imu = torch.full((40 * 90,), nan, device="cuda")
    x_s = torch.full((40 * 131,), nan, device="cuda")
    s_rest = torch.full((111 + 8,), nan, device="cuda")
    c_t = torch.full((20 + 8,), nan, device="cuda")
    k = 0
    worst = {"x_imu": 0.0, "x_s": 0.0, "pose": 0.0}
    for f in range(70):
        raw = torch.tensor(tr["raw_imu"][f][None], dtype=torch.float32).cuda()
        T = lib.tip_stream_window_len(f)
        x_imu.fill_(nan), x_s.fill_(nan)
        assert lib.tip_stream_ingest(state.data_ptr(), raw.data_ptr(), 1, f, x_imu.data_ptr(), x_s.data_ptr(), st) == 0
        if T == 0:
            continue
        assert T == tr["call_T"][k]
        torch.cuda.synchronize()
        assert torch.isnan(x_imu[T * nx:]).all() and torch.isnan(x_s[T * ns:]).all()
        xi = x_imu[: T * nx].view(T, nx).cpu().numpy()
        xs = x_s[: T * ns].view(T, ns).cpu().numpy()
        assert np.isfinite(xi).all() and np.isfinite(xs).all()
        worst["x_imu"] = max(worst["x_imu"], np.abs(xi[-1] - tr["x_imu_last_rows"][k]).max())
        worst["x_s"] = max(worst["x_s"], np.abs(xs[-1] - tr["x_s_last_rows"][k]).max())
        assert np.abs(xi[-1] - tr["x_imu_last_rows"][k]).max() < TOL_IO, (f, worst)
        assert np.abs(xs[-1] - tr["x_s_last_rows"][k]).max() < TOL_IO, (f, worst)
        if f"x_imu_call{k}" in tr:
            assert np.abs(xi - tr[f"x_imu_call{k}"]).max() < TOL_IO
            assert np.abs(xs - tr[f"x_s_call{k}"]).max() < TOL_IO
        y = torch.tensor(tr["y_last_rows"][k][None], dtype=torch.float32).cuda()
        assert lib.tip_stream_consume(state.data_ptr(), y.data_ptr(), 1, k, s_rest.data_ptr(), c_t.data_ptr(), st) == 0
        if "hist_q" in tr:       # RTRunner's corrected feedback, through the C-ABI
            q = torch.tensor(tr["hist_q"][f][None], dtype=torch.float32).cuda()
            slot = torch.zeros(1, dtype=torch.int32, device="cuda")
            assert lib.tip_stream_history_override(state.data_ptr(), 1, slot.data_ptr(), q.data_ptr(), 1, st) == 0
        torch.cuda.synchronize()
        assert torch.isnan(s_rest[111:]).all() and torch.isnan(c_t[nc:]).all()
        pose, ct = s_rest[:111].cpu().numpy(), c_t[:nc].cpu().numpy()
        worst["pose"] = max(worst["pose"], np.abs(pose - tr["qdq"][f][3:]).max())
        assert np.abs(pose - tr["qdq"][f][3:]).max() < TOL_IO, (f, worst)
        assert np.array_equal(ct[0::4], tr["ct"][f][0::4])
        assert np.abs(ct - tr["ct"][f]).max() < TOL_IO
        k += 1
    assert k == 65
    print(tag, "teacher-forced worst errors:", worst)


# ---- 3. closed loop, engine vs trace -----------------------------------------------------------------------------------------------
def _closed_loop(tr, cfg, override):
    m = _model(cfg)
    nx, ns, nc = _widths(cfg)
    eng = tip_amd.streaming.StreamingEngine(m, tr["s_init"][None])
    assert eng.x_imu.shape == (1, 40, nx) and eng.x_s.shape == (1, 40, ns) and eng.c_t.shape == (1, nc)
    n0 = m.hip_forward_count()
    worst_pose, worst_xs = 0.0, 0.0
    for f in range(70):
        out = eng.step(tr["raw_imu"][f][None])
        if f < 5:
            assert out is None
            continue
        k, T = f - 5, out["T"]
        torch.cuda.synchronize()
        assert out["y_last"].shape == (1, ns) and out["c_t"].shape == (1, nc) and out["s_rest"].shape == (1, 111)
        xs_new = eng.x_s.view(-1)[: T * ns].view(T, ns)[-1].cpu().numpy()
        worst_xs = max(worst_xs, np.abs(xs_new - tr["x_s_last_rows"][k]).max())
        worst_pose = max(worst_pose, np.abs(out["s_rest"][0].cpu().numpy() - tr["qdq"][f][3:]).max())
        if override:
            eng.override_history(tr["hist_q"][f][None])
    assert m.hip_forward_count() == n0 + 65
    m.check_handoffs()
    return worst_pose, worst_xs


@pytest.mark.parametrize("tag", list(TAGS))
def test_closed_loop_engine_tracks_reference_runners(traces, tag):
    tr, cfg = traces[tag], CFGS[tag]
    if tag == "min_noacc_5":
        sched = _model(cfg)._ensure_handle().schedule(1, 40)
        assert [p[2] for p in sched["parts"]] == [tlib.TIP_PLAN_GENERAL], sched      # 8 heads: AUTO's general plan
    worst_pose, worst_xs = _closed_loop(tr, cfg, override="hist_q" in tr)
    print(tag, f"closed loop worst |pose - reference| = {worst_pose:.2e}, worst |newest x_s row - reference| = {worst_xs:.2e}")
    assert worst_pose < TOL_LOOP and worst_xs < TOL_LOOP, (tag, worst_pose, worst_xs)
    if "hist_q" in tr:
        # the same loop WITHOUT the override feeds back the uncorrected pose: the model inputs leave the reference's
        _, xs_plain = _closed_loop(tr, cfg, override=False)
        print(tag, f"without override_history: worst |newest x_s row - reference| = {xs_plain:.2e}")
        assert xs_plain > TOL_LOOP


# ---- 4. override_history touches nothing else --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [dict(synth.PAPER), NARROW], ids=["90x131", "72x119"])
@pytest.mark.parametrize("kind", ["lockstep", "staggered", "compact"])
def test_override_history_touches_only_the_pose_columns_of_one_row(cfg, kind):
    m = _model(cfg)
    nx, ns, nc = _widths(cfg)
    n, F = 4, 9
    raw, s_init = _raw_frames(n, F, 5)
    S = tip_amd.streaming
    eng = {"lockstep": lambda: S.StreamingEngine(m, s_init), "staggered": lambda: S.StaggeredStreamingEngine(m, s_init),
           "compact": lambda: S.StaggeredStreamingEngine(m, s_init, compact=True)}[kind]()
    q = np.random.RandomState(1).randn(2, 54).astype(np.float32) * 0.4
    sel = (2, 3)
    with pytest.raises(RuntimeError):
        eng.override_history(q, sel)                             # nothing consumed yet
    if kind == "compact":
        eng.detach([0])                                          # positions [3, 1, 2]: slot 3 does not sit at its index
    for f in range(F):
        eng.step(raw[f])
    with pytest.raises(ValueError):
        eng.override_history(q, [2, 2])
    with pytest.raises(ValueError):
        eng.override_history(q[:, :50], sel)
    with pytest.raises(ValueError):
        eng.override_history(q, [2, n])
    if kind != "lockstep":
        eng.detach([1])
        with pytest.raises(RuntimeError):
            eng.override_history(q, [2, 1])                      # a detached slot
    torch.cuda.synchronize()
    before = eng.state.clone().view(torch.float32).view(n, STRIDE).cpu()
    outs = {k: getattr(eng, k).clone() for k in ("s_rest", "c_t", "x_imu", "x_s")}
    qdq = np.zeros((2, 114), dtype=np.float32)
    qdq[:, 3:57] = q
    eng.override_history(torch.tensor(qdq).cuda(), sel)          # a full qdq on the device: [3:57] is taken
    torch.cuda.synchronize()
    after = eng.state.view(torch.float32).view(n, STRIDE).cpu()
    k = F - 1 - 5                                                # the call the last frame belonged to
    row = HIST + ((k + 1) % 40) * ns
    changed = torch.zeros(n, STRIDE, dtype=torch.bool)
    changed[sel[0], row: row + 108] = changed[sel[1], row: row + 108] = True
    a, b = after.view(torch.int32), before.view(torch.int32)
    assert torch.equal(a[~changed], b[~changed]), "override_history wrote outside columns 0-107 of the newest history row"
    for j, slot in enumerate(sel):
        got = after[slot, row: row + 108].numpy()
        assert np.abs(got - aa_to_rot6d(q[j].astype(np.float64))).max() < 2e-6
        assert not np.array_equal(got, before[slot, row: row + 108].numpy())
    for kname, v in outs.items():
        assert torch.equal(torch.nan_to_num(getattr(eng, kname)), torch.nan_to_num(v)), kname
    assert int(b[1, SHP]) == (0 if ns == 131 else 1) | (0 if nx == 90 else 2)          # the shape word of every block
    # ... and the next frame reads the overridden row as the newest history row of the model input
    out = eng.step(raw[0])
    torch.cuda.synchronize()
    T = F - 4
    for j, slot in enumerate(sel):
        if kind == "lockstep":
            xs_new = eng.x_s.view(-1)[: n * T * ns].view(n, T, ns)[slot, -1]
        else:
            pos = eng.positions.index(slot) if kind == "compact" else slot
            xs_new = eng.x_s[pos, T - 1]
        assert torch.equal(xs_new[:108].cpu(), after[slot, row: row + 108])
    assert out is not None


# ---- 5. the engine forms at (72, 119) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
def test_narrow_graph_mode_equals_launch_by_launch(B):
    m = _model(NARROW)
    raw, s_init = _raw_frames(B, 64, 11 + B)
    ref = tip_amd.streaming.StreamingEngine(m, s_init)
    eng = tip_amd.streaming.StreamingEngine(m, s_init, use_graph=True)
    q = np.random.RandomState(B).randn(B, 54).astype(np.float32) * 0.3
    for f in range(64):
        a, b = ref.step(raw[f]), eng.step(raw[f])
        assert (a is None) == (b is None)
        if a is None:
            continue
        torch.cuda.synchronize()
        for k in ("s_rest", "c_t", "y_last"):
            assert torch.equal(a[k], b[k]), (f, k)
        assert torch.isfinite(b["y_last"]).all() and b["y_last"].shape == (B, 119) and b["c_t"].shape == (B, 8)
        if f in (30, 50, 51):                # an override between two launches / two replays: one small launch, no re-capture
            g = eng._graph
            ref.override_history(q), eng.override_history(q)
            assert eng._graph is g
    assert eng._graph is not None
    m.check_handoffs()


@pytest.mark.parametrize("B", [1, 5])
def test_narrow_reuse_equals_recomputation(B):
    """reuse=True at 72 + 119 input columns: bit-identical to recomputing every window on the two-window encoder (the pattern of
    tests/test_reuse_gpu.py)."""
    m = _model(NARROW)
    lib = tlib.load()
    raw, s_init = _raw_frames(B, 90, 21 + B)
    ref = tip_amd.streaming.StreamingEngine(m, s_init)
    eng = tip_amd.streaming.StreamingEngine(m, s_init, reuse=True)
    full = 0
    try:
        for f in range(raw.shape[0]):
            m.set_plan("fused2" if lib.tip_stream_window_len(f) == 40 else "auto")
            a, b = ref.step(raw[f]), eng.step(raw[f])
            assert (a is None) == (b is None)
            if a is None:
                continue
            for k in ("s_rest", "c_t", "y_last"):
                assert torch.equal(a[k], b[k]), (f, k, float((a[k] - b[k]).abs().max()))
            assert torch.isfinite(b["y_last"]).all()
            full += a["T"] == 40
    finally:
        m.set_plan("auto")
    assert full == 46
    m.check_handoffs()


STARTS = (0, 7, 19)          # the global frame at which each slot starts the trace


def _slot_frame(g, i):
    f = g - STARTS[i]
    return f if 0 <= f < 70 else None


def test_narrow_staggered_tracks_reference_runner_teacher_forced(traces):
    """tip_stream_attach / ingest_staggered / consume_staggered at (72, 119): three slots replay the full_noacc_2 trace from
    different frames; every slot's model inputs and poses are the trace's."""
    tr = traces["full_noacc_2"]
    nx, ns, nc = 72, 119, 8
    lib = tlib.load()
    n = 3
    nb = ctypes.c_size_t()
    assert lib.tip_stream_state_bytes(n, ctypes.byref(nb)) == 0
    state = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    s_init = torch.tensor(np.tile(tr["s_init"][None], (n, 1)), dtype=torch.float32).cuda()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.tip_stream_reset_shaped(state.data_ptr(), s_init.data_ptr(), n, 2, 0, st) == 0
    x_imu = torch.full((n, 40, nx), float("nan"), device="cuda")
    x_s = torch.full((n, 40, ns), float("nan"), device="cuda")
    rows = torch.empty(n, dtype=torch.int32, device="cuda")
    s_rest = torch.zeros(n, 111, device="cuda")
    c_t = torch.zeros(n, nc, device="cuda")
    checked = 0
    for g in range(70 + STARTS[-1]):
        for i in range(n):
            sl = torch.tensor([i], dtype=torch.int32, device="cuda")
            if g == STARTS[i]:
                assert lib.tip_stream_attach(state.data_ptr(), n, sl.data_ptr(), s_init[i:i + 1].data_ptr(), 1, st) == 0
            if g == STARTS[i] + 70:
                assert lib.tip_stream_detach(state.data_ptr(), n, sl.data_ptr(), 1, st) == 0
        fr = [_slot_frame(g, i) for i in range(n)]
        raw = torch.tensor(np.stack([tr["raw_imu"][f] if f is not None else np.zeros(72) for f in fr]), dtype=torch.float32).cuda()
        assert lib.tip_stream_ingest_staggered(state.data_ptr(), raw.data_ptr(), n, x_imu.data_ptr(), x_s.data_ptr(), rows.data_ptr(),
                                               st) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(x_imu).all() and torch.isfinite(x_s).all()
        y = torch.full((n, ns), float("nan"), device="cuda")
        for i, f in enumerate(fr):
            T = lib.tip_stream_window_len(f) if f is not None else 0
            assert int(rows[i]) == T - 1
            assert not x_imu[i, T:].any() and not x_s[i, T:].any()              # rows past the window: zero
            if T:
                k = f - 5
                assert np.abs(x_imu[i, T - 1].cpu().numpy() - tr["x_imu_last_rows"][k]).max() < TOL_IO, (g, i)
                assert np.abs(x_s[i, T - 1].cpu().numpy() - tr["x_s_last_rows"][k]).max() < TOL_IO, (g, i)
                if f"x_imu_call{k}" in tr:
                    assert np.abs(x_imu[i, :T].cpu().numpy() - tr[f"x_imu_call{k}"]).max() < TOL_IO
                    assert np.abs(x_s[i, :T].cpu().numpy() - tr[f"x_s_call{k}"]).max() < TOL_IO
                y[i] = torch.tensor(tr["y_last_rows"][k], dtype=torch.float32)
        assert lib.tip_stream_consume_staggered(state.data_ptr(), y.data_ptr(), rows.data_ptr(), n, s_rest.data_ptr(), c_t.data_ptr(),
                                                st) == 0
        torch.cuda.synchronize()
        for i, f in enumerate(fr):
            if f is not None and f >= 5:
                assert np.abs(s_rest[i].cpu().numpy() - tr["qdq"][f][3:]).max() < TOL_IO, (g, i)
                assert np.array_equal(c_t[i].cpu().numpy()[0::4], tr["ct"][f][0::4])
                assert np.abs(c_t[i].cpu().numpy() - tr["ct"][f]).max() < TOL_IO
                checked += 1
    assert checked == 3 * 65


@pytest.mark.parametrize("compact", [False, True], ids=["slots", "compact"])
@pytest.mark.parametrize("graph", [False, True], ids=["launch", "graph"])
def test_narrow_staggered_engine_tracks_reference_runner_closed_loop(traces, compact, graph):
    tr = traces["full_noacc_2"]
    m = _model(NARROW)
    n = 3
    s_init = np.tile(tr["s_init"][None], (n, 1)).astype(np.float32)
    eng = tip_amd.streaming.StaggeredStreamingEngine(m, s_init, use_graph=graph, compact=compact)
    if compact and graph:
        eng.prewarm()
    eng.detach([1, 2])
    worst, checked = 0.0, 0
    for g in range(70 + STARTS[-1]):
        for i in range(n):
            if g == STARTS[i] and i:
                eng.attach([i], s_init[i:i + 1])
            if g == STARTS[i] + 70:
                eng.detach([i])
        fr = [_slot_frame(g, i) for i in range(n)]
        out = eng.step(np.stack([tr["raw_imu"][f] if f is not None else np.zeros(72) for f in fr]).astype(np.float32))
        torch.cuda.synchronize()
        assert out["y_last"].shape == (n, 119) and out["c_t"].shape == (n, 8)
        for i, f in enumerate(fr):
            T = tlib.load().tip_stream_window_len(f) if f is not None else 0
            assert int(out["T"][i]) == T and bool(out["valid"][i]) == (T > 0)
            if T:
                e = np.abs(out["s_rest"][i].cpu().numpy() - tr["qdq"][f][3:]).max()
                worst = max(worst, e)
                assert e < TOL_LOOP, (g, i, e)
                assert np.abs(out["y_last"][i].cpu().numpy() - tr["y_last_rows"][f - 5]).max() < TOL_LOOP
                checked += 1
    assert checked == 3 * 65
    m.check_handoffs()
    print(f"(72, 119) staggered closed loop compact={compact} graph={graph}: worst |pose - reference| = {worst:.2e}")


def test_narrow_compact_pool_equals_fixed_slots_bit_for_bit():
    """compact=True == compact=False per slot on the pinned `fused` plan under an attach / detach schedule, at (72, 119)."""
    m = _model(NARROW)
    m.set_plan("fused")
    try:
        n, F = 6, 75
        raw, s_init = _raw_frames(n, F, 31)
        a = tip_amd.streaming.StaggeredStreamingEngine(m, s_init)
        b = tip_amd.streaming.StaggeredStreamingEngine(m, s_init, compact=True)
        rng = np.random.RandomState(4)
        for f in range(F):
            if f and f % 6 == 0:
                att = a.attached
                off = [i for i in range(n) if att[i] and rng.rand() < 0.35]
                on = [i for i in range(n) if not att[i] and rng.rand() < 0.6]
                for e in (a, b):
                    e.detach(off)
                    e.attach(on, s_init[on])
            oa, ob = a.step(raw[f]), b.step(raw[f])
            torch.cuda.synchronize()
            assert torch.equal(oa["T"], ob["T"]) and torch.equal(oa["valid"], ob["valid"])
            v = oa["valid"]
            for k in ("s_rest", "c_t"):
                assert torch.equal(oa[k], ob[k]), (f, k)
            assert torch.equal(oa["y_last"][v], ob["y_last"][v]), f
            assert torch.isfinite(ob["y_last"][v]).all()
        assert int(oa["valid"].sum()) >= 1
    finally:
        m.set_plan("auto")


# ---- 6. poisoned buffers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["min_noacc_5", "full_noacc_2", "full_acc_2"])
@pytest.mark.parametrize("kind", ["lockstep", "staggered", "compact"])
def test_poisoned_buffers_at_the_narrow_shapes(tag, kind):
    """x_imu, x_s, c_t, s_rest pre-filled with NaN: every window the forward reads was written in full, nothing NaN comes out; the
    device restatement (ShapedOracle, random closed loop) agrees with the poses."""
    cfg = CFGS[tag]
    m = _model(cfg)
    n_sbps, acc = TAGS[tag]
    n, F = 3, 50
    raw, s_init = _raw_frames(n, F, 41)
    S = tip_amd.streaming
    eng = {"lockstep": lambda: S.StreamingEngine(m, s_init), "staggered": lambda: S.StaggeredStreamingEngine(m, s_init),
           "compact": lambda: S.StaggeredStreamingEngine(m, s_init, compact=True)}[kind]()
    for name in ("x_imu", "x_s", "c_t", "s_rest"):
        getattr(eng, name).fill_(float("nan"))
    oracles = [ShapedOracle(s_init[b].astype(np.float64), n_sbps, acc) for b in range(n)]
    worst = 0.0
    for f in range(F):
        out = eng.step(raw[f])
        ready = [o.ingest(raw[f][b].astype(np.float64)) for b, o in enumerate(oracles)]
        if f < 5:
            assert not any(ready)
            continue
        torch.cuda.synchronize()
        for k in ("s_rest", "c_t", "y_last"):
            assert torch.isfinite(out[k]).all(), (f, k)
        y = out["y_last"].cpu().numpy()
        for b, o in enumerate(oracles):                          # teacher-forced on the device's own y: the glue alone
            o.build_inputs()
            sr, ct = o.consume(y[b])
            d = np.abs(out["s_rest"][b].cpu().numpy() - sr)
            # (a joint within 0.05 rad of pi: either sign of its rotation vector is the same rotation — not compared as a vector)
            d[:54][np.repeat(np.linalg.norm(sr[:54].reshape(18, 3), axis=1) > np.pi - 0.05, 3)] = 0.0
            worst = max(worst, d.max())
            assert np.array_equal(out["c_t"][b].cpu().numpy()[0::4], ct[0::4]), (f, b)
    m.check_handoffs()
    print(tag, kind, f"poisoned run: worst |pose - restatement| = {worst:.2e}")
    assert worst < TOL_IO


# ---- 7. unsupported shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [dict(synth.PAPER, size_s=123), dict(synth.PAPER, input_size_imu=60)], ids=["size_s123", "imu60"])
def test_unsupported_shapes_raise_value_error(cfg):
    m = make_model(cfg).cuda().eval()
    s_init = np.zeros((2, 114), dtype=np.float32)
    for make in (lambda: tip_amd.streaming.StreamingEngine(m, s_init), lambda: tip_amd.streaming.StaggeredStreamingEngine(m, s_init),
                 lambda: tip_amd.streaming.StaggeredStreamingEngine(m, s_init, compact=True)):
        with pytest.raises(ValueError, match="72 / 119"):
            make()
