"""GPU tests of offline replay (tip_amd.replay.ReplayPool; csrc/tip_replay.hip): the two kernels through the C-ABI, the pool against
the same recordings run alone through a one-slot StaggeredStreamingEngine (bit for bit on a plan whose bits do not depend on batch or
position), graph mode against launch by launch, the trace of the real reference runner, and the lost-hand-off restart."""
import numpy as np
import pytest
import torch

import tip_amd
from tip_amd import replay, synth
from tip_amd import lib as tlib
from test_host_cpu import make_model, load_synth
from test_staggered_streams_gpu import paper, trace, TOL_LOOP  # noqa: F401

pytestmark = pytest.mark.gpu
Engine = tip_amd.streaming.StaggeredStreamingEngine
LENGTHS = [6, 7, 44, 45, 46, 12, 90]      # priming only, the first valid row, the window filling at frame 44
NARROW = dict(synth.PAPER, size_s=119, with_acc_sum=False)


def _recordings(lengths, seed0=200):
    recs, s0 = zip(*(synth.make_recording(L, seed=seed0 + i) for i, L in enumerate(lengths)))
    return list(recs), np.stack(s0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same(a: replay.ReplayResult, b: replay.ReplayResult, who):
    assert np.array_equal(a.valid, b.valid), who
    for k in ("s_rest", "c_t", "y_last"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (who, k)


def _alone(m, rec, s0, **kw):
    """One recording through a fresh one-slot engine, frame by frame through step(), laid out by the script's row conventions."""
    eng = Engine(m, s0[None], **kw)
    L = rec.shape[0]
    s = torch.zeros(L, 111, device="cuda")
    c = torch.zeros(L, eng.nc, device="cuda")
    y = torch.full((L, eng.ns), float("nan"), device="cuda")
    v = torch.zeros(L, dtype=torch.bool, device="cuda")
    s[:] = torch.tensor(s0[3:]).cuda()
    frames = torch.tensor(rec).cuda()
    for t in range(L - 1):
        out = eng.step(frames[t][None])
        ok = out["valid"][0]
        v[t + 1] = ok
        s[t + 1] = torch.where(ok, out["s_rest"][0], s[0])
        c[t + 1] = torch.where(ok, out["c_t"][0], c[0])
        y[t + 1] = out["y_last"][0]
    torch.cuda.synchronize()
    return replay.ReplayResult(s.cpu().numpy(), c.cpu().numpy(), v.cpu().numpy(), y.cpu().numpy())


@pytest.fixture(scope="module")
def case(paper):
    """The recordings of LENGTHS and, under set_plan("fused"), each of them run alone."""
    m, _ = paper
    recs, s0 = _recordings(LENGTHS)
    m.set_plan("fused")
    try:
        alone = [_alone(m, r, s0[i]) for i, r in enumerate(recs)]
    finally:
        m.set_plan("auto")
    return recs, s0, alone


def _check_conventions(out, recs, s0):
    for i, r in enumerate(out):
        L, prim = recs[i].shape[0], min(recs[i].shape[0], 6)
        assert r.s_rest.shape == (L, 111) and r.valid.shape == (L,) and r.valid.dtype == bool
        assert not r.valid[:prim].any() and r.valid[prim:].all(), i
        assert np.array_equal(r.s_rest[:prim], np.repeat(s0[i][None, 3:], prim, 0)) and not r.c_t[:prim].any(), i
        if r.y_last is not None:
            assert np.isnan(r.y_last[:prim]).all()


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------------------
def _kernels_model(cur, end, n_rows, corpus, rows_slot, s_rest, c_t, y_slot, s_out, c_out, y_out, valid):
    """tip_replay_feed and tip_replay_collect as include/tip_hip.h states them, in numpy (in place; returns raw)."""
    n = len(cur)
    raw = np.zeros((n, 72), np.float32)
    for s in range(n):
        if 0 <= cur[s] < n_rows:
            raw[s] = corpus[cur[s]]
    for s in range(n):
        c = cur[s]
        if c < 0:
            continue
        if c + 1 >= n_rows:
            cur[s] = -1
            continue
        if rows_slot[s] >= 0:
            s_out[c + 1], c_out[c + 1], valid[c + 1] = s_rest[s], c_t[s], 1
            if y_out is not None:
                y_out[c + 1] = y_slot[s]
        else:
            s_out[c + 1], c_out[c + 1], valid[c + 1] = s_out[c], 0.0, 0
            if y_out is not None:
                y_out[c + 1] = np.nan
        cur[s] = -1 if c + 1 >= end[s] else c + 1
    return raw


@pytest.mark.parametrize("ns,keep_y", [(131, True), (119, True), (131, False)])
def test_kernels_through_the_c_abi(ns, keep_y):
    """Hand-made cursor tables, three frames: idle slots; a slot on its first frame (priming), one priming further in, one on its last fed
    frame; two slots of different recordings on adjacent corpus rows (the last row of one, the first rows of the next); a cursor that
    points past the corpus.  Everything around raw and around every output is NaN before and after; cursors end where they must."""
    lib, st = tlib.load(), torch.cuda.current_stream().cuda_stream
    rng = np.random.RandomState(5)
    n, n_rows, nc = 9, 41, ns - 111
    # recordings (corpus rows): A 0-9, B 10-19, C 20-29, D 30-34, E 35-40
    cur = np.array([-1, 0, 12, 28, 33, 35, -1, 40, 5], dtype=np.int64)
    end = np.array([-1, 9, 19, 29, 34, 40, 7, 45, 9], dtype=np.int64)
    rows_by_frame = [np.array([-1, -1, -1, 39, 3, -1, 5, 2, 0], dtype=np.int32),
                     np.array([-1, -1, 0, 39, 4, -1, 5, 2, 1], dtype=np.int32),
                     np.array([7, -1, 1, -1, 5, -1, 5, 2, 2], dtype=np.int32)]
    corpus = rng.randn(n_rows, 72).astype(np.float32)

    def guarded(rows, width, fill=None):
        t = torch.full((rows + 2, width), float("nan"), device="cuda")
        if fill is not None:
            t[1:-1] = torch.tensor(fill).cuda()
        return t

    g_corpus, g_raw = guarded(n_rows, 72, corpus), guarded(n, 72)
    h_s, h_c = rng.randn(n_rows, 111).astype(np.float32), rng.randn(n_rows, nc).astype(np.float32)
    h_y, h_v = rng.randn(n_rows, ns).astype(np.float32), np.full(n_rows, 7, np.uint8)
    g_s, g_c, g_y = guarded(n_rows, 111, h_s), guarded(n_rows, nc, h_c), guarded(n_rows, ns, h_y)
    g_v = torch.full((n_rows + 32,), 9, dtype=torch.uint8, device="cuda")
    g_v[16:16 + n_rows] = 7
    d_tbl = torch.full((4, n), -99, dtype=torch.int64, device="cuda")         # rows 1 and 2: cur, end; 0 and 3: guards
    d_tbl[1], d_tbl[2] = torch.tensor(cur).cuda(), torch.tensor(end).cuda()
    h_y_arg = h_y if keep_y else None
    for f, rows_slot in enumerate(rows_by_frame):
        s_rest, c_t = rng.randn(n, 111).astype(np.float32), rng.randn(n, nc).astype(np.float32)
        y_slot = rng.randn(n, ns).astype(np.float32)
        y_slot[rows_slot < 0] = np.nan
        d_s, d_c, d_ys = guarded(n, 111, s_rest), guarded(n, nc, c_t), guarded(n, ns, y_slot)
        d_rows = torch.tensor(rows_slot).cuda()
        g_raw[1:-1] = float("nan")
        assert lib.tip_replay_feed(g_corpus[1:].data_ptr(), n_rows, d_tbl[1].data_ptr(), n, g_raw[1:].data_ptr(), st) == 0
        assert lib.tip_replay_collect(d_tbl[1].data_ptr(), d_tbl[2].data_ptr(), n, n_rows, d_s[1:].data_ptr(), d_c[1:].data_ptr(),
                                      d_ys[1:].data_ptr(), d_rows.data_ptr(), ns, g_s[1:].data_ptr(), g_c[1:].data_ptr(),
                                      g_y[1:].data_ptr() if keep_y else None, g_v[16:].data_ptr(), st) == 0
        torch.cuda.synchronize()
        raw = _kernels_model(cur, end, n_rows, corpus, rows_slot, s_rest, c_t, y_slot, h_s, h_c, h_y_arg, h_v)
        assert np.array_equal(g_raw[1:-1].cpu().numpy(), raw), f
        assert d_tbl[1].cpu().tolist() == cur.tolist() and d_tbl[2].cpu().tolist() == end.tolist(), f
        assert bool((d_tbl[0] == -99).all()) and bool((d_tbl[3] == -99).all())
        for g, h in ((g_s, h_s), (g_c, h_c), (g_y, h_y)):
            assert np.array_equal(_bits(g[1:-1].cpu().numpy()), _bits(h)), f          # (h_y is left alone when keep_y is False)
            assert bool(torch.isnan(g[0]).all()) and bool(torch.isnan(g[-1]).all()), f
        assert np.array_equal(g_v[16:16 + n_rows].cpu().numpy(), h_v) and bool((g_v[:16] == 9).all()) and bool((g_v[16 + n_rows:] == 9).all())
        assert bool(torch.isnan(g_raw[0]).all()) and bool(torch.isnan(g_raw[-1]).all()) and bool(torch.isnan(g_corpus[0]).all())
        # inputs are read only
        assert np.array_equal(_bits(d_s[1:-1].cpu().numpy()), _bits(s_rest)) and np.array_equal(g_corpus[1:-1].cpu().numpy(), corpus)
    #   slot: 0 idle, 1 A (3 priming frames), 2 B, 3 C ended after frame 0, 4 D ended after frame 0, 5 E, 6 idle, 7 past the corpus, 8 A's tail
    assert cur.tolist() == [-1, 3, 15, -1, -1, 38, -1, -1, 8]
    assert h_v[[1, 2, 3]].tolist() == [0, 0, 0] and h_v[[13, 14, 15]].tolist() == [0, 1, 1] and h_v[29] == 1 and h_v[34] == 1
    assert h_v[35] == 7 and h_v[[36, 37, 38]].tolist() == [0, 0, 0]               # E's row 0 is the host's: never written
    assert np.array_equal(h_s[36], h_s[35]) and np.array_equal(h_s[38], h_s[35]) and not h_c[36].any()


# ---- 2. bit identity with each recording run alone --------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [3, 1])
def test_pool_equals_each_recording_alone(paper, case, slots):
    m, _ = paper
    recs, s0, alone = case
    plan = replay.plan_replay(LENGTHS, slots)
    if slots == 3:
        # with these lengths: a frame on which one slot turns over while another, re-attached the frame before, is still on its first
        # priming frames (several slots turning over on ONE frame: test_slots_turning_over_on_the_same_frame)
        att_frames = [f for f, (att, _) in enumerate(plan.frames) if att and f > 0]
        assert any(b - a == 1 for a, b in zip(att_frames, att_frames[1:])), att_frames
    m.set_plan("fused")
    try:
        pool = replay.ReplayPool(m, slots=slots, use_graph=False, keep_y=True)
        out = pool.run(recs, s0)
    finally:
        m.set_plan("auto")
    assert pool.frames == plan.n_frames and pool.restarts == 0
    assert not any(pool.engine.attached)
    _check_conventions(out, recs, s0)
    for i in range(len(recs)):
        _same(out[i], alone[i], (slots, i))
    assert out[1].valid.sum() == 1 and not out[0].valid.any()


_alone_cache = {}
SAME_FRAME = [([6, 6, 44, 45, 46, 12, 90], 2, 1),       # frame 5: slots 0 and 1 turn over while slot 2 is mid-recording
              ([30] * 7, 3, 0)]                          # equal lengths (a test set cropped to one test_len): all three at once, twice


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("lengths,together,beside", SAME_FRAME, ids=["two_of_three", "all_three"])
def test_slots_turning_over_on_the_same_frame(paper, lengths, together, beside, use_graph):
    """Slots whose recordings end on the same frame take their next recordings on ONE engine frame: one attach of several attached
    slots and one upload of the cursor table that rewrites several live cursors, while the other slots go on.  A fresh attach to a
    free slot cannot coincide with a turn-over (no slot is free while a recording waits), but turn-overs coincide whenever lengths
    do.  Every recording's rows are, bit for bit, the recording run alone on set_plan("fused")."""
    m, _ = paper
    recs, s0 = _recordings(lengths, seed0=600)
    plan = replay.plan_replay(lengths, 3)
    hits = []
    for f, (att, _) in enumerate(plan.frames):
        if f == 0 or len(att) != together:
            continue
        turned = {s for s, _ in att}
        going = [i for i, L in enumerate(lengths) if plan.start[i] < f <= plan.start[i] + L - 2 and plan.slot[i] not in turned]
        if len(going) == beside:
            hits.append(f)
    assert hits, "no frame on which the slots turn over together"
    m.set_plan("fused")
    try:
        key = tuple(lengths)
        if key not in _alone_cache:                     # (computed once, shared by the two modes)
            _alone_cache[key] = [_alone(m, r, s0[i]) for i, r in enumerate(recs)]
        alone = _alone_cache[key]
        pool = replay.ReplayPool(m, slots=3, use_graph=use_graph, keep_y=True)
        out = pool.run(recs, s0)
    finally:
        m.set_plan("auto")
    assert pool.frames == plan.n_frames and pool.restarts == 0 and not any(pool.engine.attached)
    _check_conventions(out, recs, s0)
    for i in range(len(recs)):
        _same(out[i], alone[i], (lengths, i))


# ---- 3. graph mode -----------------------------------------------------------------------------------------------------------------
def test_graph_mode_equals_launch_by_launch(paper):
    """The same case under AUTO, 3 slots: captured frames (feed -> the engine's mapped frame -> collect, one capture per bucket) give
    the launch-by-launch bits; a second run of the same pool re-captures and gives them again."""
    m, _ = paper
    recs, s0 = _recordings(LENGTHS)
    ref = replay.ReplayPool(m, slots=3, use_graph=False, keep_y=True).run(recs, s0)
    pool = replay.ReplayPool(m, slots=3, use_graph=True, keep_y=True)
    out = pool.run(recs, s0)
    assert pool.frames == replay.plan_replay(LENGTHS, 3).n_frames
    assert 1 <= pool.engine.captures <= len(pool.engine.ladder)
    for i in range(len(recs)):
        _same(out[i], ref[i], i)
    again = pool.run(recs, s0)
    for i in range(len(recs)):
        _same(again[i], ref[i], ("second run", i))


# ---- 4. the real runner --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
def test_replay_tracks_reference_runner(trace, paper, use_graph):
    """The raw IMU of the golden trace as one recording between two synthetic ones, two slots: the step on frame f fills row f + 1 with
    what the reference's RTRunnerMin returned for frame f."""
    m, _ = paper
    tr = trace[0]
    syn, s_syn = _recordings([31, 80], seed0=300)
    recs = [syn[0], tr["raw_imu"].astype(np.float32), syn[1]]
    s0 = np.stack([s_syn[0], tr["s_init"].astype(np.float32), s_syn[1]])
    out = replay.ReplayPool(m, slots=2, use_graph=use_graph, keep_y=True).run(recs, s0)
    _check_conventions(out, recs, s0)
    r, worst = out[1], 0.0
    F = tr["raw_imu"].shape[0]
    assert r.s_rest.shape[0] == F
    for f in range(F - 1):                        # (the last frame is never fed)
        if f < 5:
            assert not r.valid[f + 1] and np.array_equal(r.s_rest[f + 1], s0[1][3:])
            assert np.abs(s0[1].astype(np.float64) - tr["qdq"][f])[3:].max() < 1e-6        # the runner returns s_init while it primes
            continue
        e = np.abs(r.s_rest[f + 1] - tr["qdq"][f][3:]).max()
        worst = max(worst, e)
        assert r.valid[f + 1] and e < TOL_LOOP, (f, e)
        assert np.abs(r.y_last[f + 1] - tr["y_last_rows"][f - 5]).max() < TOL_LOOP, f
        assert np.array_equal(r.c_t[f + 1][0::4], tr["ct"][f][0::4]), f
        assert np.abs(r.c_t[f + 1] - tr["ct"][f]).max() < TOL_LOOP, f
    print("replay closed-loop worst |pose - reference| =", worst)


# ---- 5. AUTO against the pinned plan ---------------------------------------------------------------------------------------------------
def test_auto_stays_within_the_loop_bound_of_the_pinned_plan(paper, case):
    """AUTO changes plan with the bucket, so bits may differ from the pinned plan's; the closed loop stays within TOL_LOOP over the
    first 60 frames of every recording, and valid is the same."""
    m, _ = paper
    recs, s0, alone = case
    out = replay.ReplayPool(m, slots=3, use_graph=False, keep_y=True).run(recs, s0)
    worst = 0.0
    for i, r in enumerate(out):
        assert np.array_equal(r.valid, alone[i].valid)
        for k in ("s_rest", "c_t", "y_last"):
            a, b = getattr(r, k)[:61], getattr(alone[i], k)[:61]
            assert np.array_equal(np.isnan(a), np.isnan(b))
            if a[r.valid[:61]].size:
                worst = max(worst, float(np.abs(a[r.valid[:61]] - b[r.valid[:61]]).max()))
    print("AUTO against fused, worst over 60 frames:", worst)
    assert worst < TOL_LOOP


# ---- 6. shapes and window --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,window", [(synth.PAPER, 24), (NARROW, 40)], ids=["window24", "two_sbp_no_acc_sum"])
def test_shapes_and_window(paper, cfg, window):
    if cfg is synth.PAPER:
        m = paper[0]
    else:
        m = make_model(cfg)
        load_synth(m, cfg, 0)
        m = m.cuda().eval()
    lengths = [7, 33, 12, 40]                    # window 24 fills at frame 28
    recs, s0 = _recordings(lengths, seed0=400)
    m.set_plan("fused")
    try:
        alone = [_alone(m, r, s0[i], window=window) for i, r in enumerate(recs)]
        pool = replay.ReplayPool(m, slots=2, window=window, use_graph=False, keep_y=True)
        out = pool.run(recs, s0)
    finally:
        m.set_plan("auto")
    assert pool.engine.window == window
    assert out[1].c_t.shape == (33, cfg["size_s"] - 111) and out[1].y_last.shape == (33, cfg["size_s"])
    _check_conventions(out, recs, s0)
    for i in range(len(recs)):
        _same(out[i], alone[i], i)


# ---- 7. the deployed model: dropout live ----------------------------------------------------------------------------------------------
def test_live_dropout_pool():
    cfg = synth.PAPER
    m = make_model(cfg, p_state=0.8, dropout=0.1)
    load_synth(m, cfg, 0)
    m = m.cuda().train()
    lengths = [20, 7, 50]
    recs, s0 = _recordings(lengths, seed0=500)
    with pytest.raises(RuntimeError):
        replay.ReplayPool(m, slots=2)                                # the engine's own refusal of a .train() model without live_dropout
    pool = replay.ReplayPool(m, slots=2, live_dropout=True, use_graph=True, keep_y=True)
    torch.manual_seed(7)
    out = pool.run(recs, s0)
    _check_conventions(out, recs, s0)
    for r in out:
        assert np.isfinite(r.s_rest).all() and np.isfinite(r.c_t).all() and np.isfinite(r.y_last[r.valid]).all()
    m.eval()
    quiet = replay.ReplayPool(m, slots=2, live_dropout=False, use_graph=False, keep_y=True).run(recs, s0)
    m.train()
    assert not np.array_equal(out[2].s_rest[6:], quiet[2].s_rest[6:])
    # one slot, one recording: a one-slot live engine under the same seed (the engine draws its device seeds from torch's generator at
    # every reset; ReplayPool.run resets once)
    one = replay.ReplayPool(m, slots=1, live_dropout=True, use_graph=False, keep_y=True)
    torch.manual_seed(11)
    got = one.run(recs[2:], s0[2:])[0]
    eng = Engine(m, s0[2:], compact=True, live_dropout=True)
    torch.manual_seed(11)
    eng.reset()
    L = lengths[2]
    frames = torch.tensor(recs[2]).cuda()
    for t in range(L - 1):
        o = eng.step(frames[t][None])
        torch.cuda.synchronize()
        if t < 5:
            assert not bool(o["valid"][0])
            continue
        assert bool(o["valid"][0])
        assert np.array_equal(_bits(o["s_rest"][0].cpu().numpy()), _bits(got.s_rest[t + 1])), t
        assert np.array_equal(_bits(o["y_last"][0].cpu().numpy()), _bits(got.y_last[t + 1])), t
        assert np.array_equal(_bits(o["c_t"][0].cpu().numpy()), _bits(got.c_t[t + 1])), t


# ---- 8. no host traffic ----------------------------------------------------------------------------------------------------------------
def test_no_per_frame_host_traffic(paper, monkeypatch):
    """Launch by launch (a replayed graph does not pass through tip_forward's host entry), 3 slots: one forward per engine frame, every
    frame through the device-fed method, the host-fed step paths never entered, attach / detach on exactly the frames of the plan."""
    m, _ = paper
    recs, s0 = _recordings(LENGTHS)
    pool = replay.ReplayPool(m, slots=3, use_graph=False)
    eng = pool.engine

    def never(*a, **k):
        raise AssertionError("a host-fed step path was taken")

    monkeypatch.setattr(eng, "step", never)
    monkeypatch.setattr(eng, "_step_compact", never)
    calls = []
    real_attach, real_detach = eng.attach, eng.detach
    monkeypatch.setattr(eng, "attach", lambda sl, rows: (calls.append(("a", eng.fed_frames - base, list(sl))), real_attach(sl, rows))[1])
    monkeypatch.setattr(eng, "detach", lambda sl: (calls.append(("d", eng.fed_frames - base, list(sl))), real_detach(sl))[1])
    base = eng.fed_frames
    n0, fed0 = m.hip_forward_count(), eng.fed_frames
    out = pool.run(recs, s0)
    plan = replay.plan_replay(LENGTHS, 3)
    assert pool.frames == plan.n_frames == eng.fed_frames - fed0
    assert m.hip_forward_count() - n0 == pool.frames            # (no frame of this schedule is empty)
    want = []
    for f, (att, det) in enumerate(plan.frames):
        want += [("d", f, list(det))] if det else []
        want += [("a", f, [s for s, _ in att])] if att else []
    want += [("d", plan.n_frames, list(plan.final_detach))]
    assert [c for c in calls if c[2]] == want
    assert out[0].y_last is None and out[6].valid.sum() == LENGTHS[6] - 6
    with pytest.raises(ValueError):
        pool.run(recs, s0[:3])
    with pytest.raises(ValueError):
        pool.run([], s0[:0])
    with pytest.raises(ValueError):
        pool.run([recs[0][:, :60]], s0[:1])


# ---- 9. lost hand-off --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
def test_lost_handoff_restarts_the_recordings_in_flight(paper, case, monkeypatch, use_graph):
    """A loss simulated on the host as tests/test_stream_pool_gpu.py does (launch mode: the model's demotion counter moves during a
    forward; graph mode: the poll before a replay raises): run() restarts the recordings in flight, counts them, and finishes with
    the undisturbed run's rows; a second loss in the same run is raised."""
    m, _ = paper
    recs, s0, alone = case
    plan = replay.plan_replay(LENGTHS, 3)
    LOSS = 20                                                       # engine frame on which the loss is noticed
    in_flight = [i for i, L in enumerate(LENGTHS) if L > 1 and plan.start[i] <= LOSS <= plan.start[i] + L - 2]
    assert len(in_flight) == 3
    m.set_plan("fused")
    try:
        pool = replay.ReplayPool(m, slots=3, use_graph=use_graph, keep_y=True)
        eng = pool.engine
        d0 = m.demotions

        def run_with_losses(at):
            """Lose the hand-off on the calls `at` of the engine's device-fed step (counted over the whole run, the failing ones
            included): the loss is armed in front of the call and disarms itself when it fires."""
            state = {"f": -1}
            real_step = eng._step_fed

            def step_fed():
                state["f"] += 1
                if state["f"] in at:
                    if use_graph:
                        def lost(synchronize=True, clear=False):
                            monkeypatch.setattr(m, "check_handoffs", real_check)
                            raise tlib.TipHandoffError(tlib.TIP_ERR_HANDOFF, "simulated")
                        real_check = m.check_handoffs
                        monkeypatch.setattr(m, "check_handoffs", lost)
                        monkeypatch.setattr(m, "_answer_handoff", lambda h: "demoted")
                    else:
                        real_fwd = m.forward_rows

                        def lossy(*a, **k):
                            y = real_fwd(*a, **k)
                            m.demotions += 1
                            monkeypatch.setattr(m, "forward_rows", real_fwd)
                            return y
                        monkeypatch.setattr(m, "forward_rows", lossy)
                return real_step()

            monkeypatch.setattr(eng, "_step_fed", step_fed)
            try:
                return pool.run(recs, s0)
            finally:
                monkeypatch.undo()
                m.demotions = d0

        out = run_with_losses({LOSS})
        assert pool.restarts == len(in_flight)
        # the frames before the loss, then the restarted schedule: the three recordings again from their frame 0, the rest behind them
        rest = replay._plan(LENGTHS, 3, [i for i in range(len(LENGTHS)) if plan.start[i] > LOSS],
                            {plan.slot[i]: i for i in in_flight})
        assert pool.frames == LOSS + rest.n_frames
        for i in range(len(recs)):
            _same(out[i], alone[i], i)
        with pytest.raises(tlib.TipHandoffError):
            run_with_losses({LOSS, LOSS + 9})
        out = pool.run(recs, s0)                                    # the pool is usable afterwards
        assert pool.restarts == 0
        for i in range(len(recs)):
            _same(out[i], alone[i], ("after", i))
    finally:
        m.set_plan("auto")
        m.demotions = d0
