"""GPU tests of ReplayPool(terrain=...) (tip_amd.replay; csrc/tip_replay.hip: tip_replay_mask, tip_replay_collect_tracked): the full
runner's tail inside the pool's frame, IK feedback in the loop.  The new entries through the C-ABI on fabricated buffers; the tracked
pool against the plain pool plus the post-pass (multi_sbp off) and against each recording run alone through a one-slot engine stepped
from the host with TerrainTracker.step + feed_back (multi_sbp on), bit for bit under set_plan("fused"); graph mode; host traffic and
the launch budget; the lost hand-off; and the reference's true closed loop (tests/golden/tip_terrain_loop_golden.npz).

The model is the synthetic one with the contact logits of lankle, rankle and root shifted by +0.5 (replay_terrain_oracle.BIAS_INDEX /
BIAS_SHIFT, the fixture's departure from load_synth), on upright recordings (replay_terrain_oracle.standing_recording): the CPU oracle
composition (tests/replay_terrain_oracle.py with the fp64 forward oracle) fires on rows 7 .. of every recording of 8 frames or more
with these — lengths (70, 48, 8, 7, 1, 30), seeds 700 ..: 62, 41, 1, 0, 0 and 20 fired rows — which is what the conditions below need;
they are asserted from the device's own `fire`."""
import os

import numpy as np
import pytest
import torch

import replay_terrain_oracle as rto
import terrain_oracle as to
import tip_amd
from tip_amd import kinematics as kin
from tip_amd import replay, synth, terrain
from tip_amd import lib as tlib
from test_host_cpu import make_model
from test_staggered_streams_gpu import TOL_LOOP

pytestmark = pytest.mark.gpu
f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "tip_terrain_golden.npz"))
TABLE = {k[len("table/"):]: GOLDEN[k] for k in GOLDEN.files if k.startswith("table/")}
LOOP_PATH = os.path.join(HERE, "golden", "tip_terrain_loop_golden.npz")
Engine = tip_amd.streaming.StaggeredStreamingEngine
LENGTHS = (70, 48, 8, 7, 1, 30)
NARROW = dict(synth.PAPER, size_s=119, with_acc_sum=False)
ARRAYS = ("s_rest", "c_t", "valid", "y_last", "root", "viz_locs", "q_hist", "fire")


@pytest.fixture(scope="module")
def skel():
    return kin.Skeleton.from_table(GOLDEN)


def _shifted_model(cfg=synth.PAPER, **kw):
    m = make_model(cfg, **kw)
    w = synth.make_weights(cfg, seed=0)
    w["linear.bias"] = w["linear.bias"].copy()
    idx = [i for i in rto.BIAS_INDEX if i < cfg["size_s"]]
    w["linear.bias"][idx] += f32(rto.BIAS_SHIFT)
    m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    return m.cuda()


@pytest.fixture(scope="module")
def model():
    return _shifted_model().eval()


def _recordings(lengths, seed0=700):
    recs, s0 = zip(*(rto.standing_recording(L, seed0 + i) for i, L in enumerate(lengths)))
    return list(recs), np.stack(s0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b, who, fields=ARRAYS + ("off_map", "regions_full")):
    for k in fields:
        x, y = getattr(a, k), getattr(b, k)
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(_bits(x), _bits(y)), (who, k)
        else:
            assert x == y, (who, k, x, y)


def _check_conventions(out, recs, s0):
    for i, r in enumerate(out):
        L, prim = recs[i].shape[0], min(recs[i].shape[0], 6)
        assert type(r) is replay.TrackedReplayResult
        assert r.s_rest.shape == (L, 111) and r.root.shape == (L, 3) and r.viz_locs.shape == (L, 5, 3) and r.q_hist.shape == (L, 54)
        assert r.fire.shape == (L,) and r.fire.dtype == bool and r.valid.dtype == bool
        assert not r.valid[:prim].any() and r.valid[prim:].all(), i
        assert np.array_equal(r.s_rest[:prim], np.repeat(s0[i][None, 3:], prim, 0)) and not r.c_t[:prim].any(), i
        assert np.array_equal(r.root[:prim], np.repeat(s0[i][None, :3], prim, 0)) and (r.viz_locs[:prim] == 100).all(), i
        assert np.array_equal(r.q_hist[:prim], np.repeat(s0[i][None, 3:57], prim, 0)) and not r.fire[:prim].any(), i
        assert np.array_equal(r.q_hist[~r.fire], r.s_rest[~r.fire, :54]), i
        assert np.array_equal(r.qdq, np.concatenate([r.root, r.s_rest], axis=1))


def _alone(m, skel, rec, s0, multi, window=40, map_bound=5.0, max_regions=64):
    """One recording through a fresh one-slot engine stepped from the host, launch mode, with TerrainTracker.step + feed_back behind
    every frame — the only way to get IK feedback before ReplayPool(terrain=...) — laid out by the script's row conventions."""
    eng = Engine(m, s0[None], window=window)
    tt = terrain.TerrainTracker(skel, 1, "cuda", map_bound, 0.1, multi_sbp=multi, max_regions=max_regions)
    tt.reset(None, s0[None])
    L = rec.shape[0]
    dev = dict(s_rest=torch.zeros(L, 111), c_t=torch.zeros(L, eng.nc), y_last=torch.full((L, eng.ns), float("nan")),
               valid=torch.zeros(L, dtype=torch.bool), root=torch.zeros(L, 3), viz_locs=torch.full((L, 5, 3), 100.0),
               q_hist=torch.zeros(L, 54), fire=torch.zeros(L, dtype=torch.bool))
    dev = {k: v.cuda() for k, v in dev.items()}
    dev["s_rest"][:], dev["root"][:], dev["q_hist"][:] = (torch.tensor(s0[a:b]).cuda() for a, b in ((3, 114), (0, 3), (3, 57)))
    frames = torch.tensor(rec).cuda()
    for t in range(L - 1):
        out = eng.step(frames[t][None])
        tt.step(out)
        tt.feed_back(eng)
        ok = out["valid"][0]
        dev["valid"][t + 1] = ok
        dev["y_last"][t + 1] = out["y_last"][0]
        for k, src in (("s_rest", out["s_rest"]), ("c_t", out["c_t"]), ("root", tt.root), ("viz_locs", tt.viz_locs), ("q_hist", tt.q_hist)):
            dev[k][t + 1] = torch.where(ok, src[0], dev[k][0])
        dev["fire"][t + 1] = ok & (tt.fire[0] >= 0)
    torch.cuda.synchronize()
    st = tt.state(0)
    return replay.TrackedReplayResult(*(dev[k].cpu().numpy() for k in ARRAYS), int(st.off_map), int(st.regions_full))


def _pool(m, skel, slots, multi, use_graph=False, **kw):
    tkw = {k: kw.pop(k) for k in ("map_bound", "max_regions") if k in kw}
    return replay.ReplayPool(m, slots=slots, use_graph=use_graph, keep_y=True,
                             terrain=dict(skel=skel, map_bound=tkw.get("map_bound", 5.0), grid_size=0.1, multi_sbp=multi,
                                          max_regions=tkw.get("max_regions", 64)), **kw)


@pytest.fixture(scope="module")
def case(model, skel):
    """The recordings of LENGTHS and, under set_plan("fused") with multi_sbp on, each of them run alone; the plain pool's rows."""
    recs, s0 = _recordings(LENGTHS)
    model.set_plan("fused")
    try:
        alone = [_alone(model, skel, r, s0[i], True) for i, r in enumerate(recs)]
        plain = replay.ReplayPool(model, slots=2, use_graph=False, keep_y=True).run(recs, s0)
    finally:
        model.set_plan("auto")
    return recs, s0, alone, plain


# ---- 1. the new entries through the C-ABI -----------------------------------------------------------------------------------------
def _guarded(rows, width, fill, dtype=torch.float32, guard=float("nan")):
    t = torch.full((rows + 2, width), guard, dtype=dtype, device="cuda")
    t[1:-1] = torch.as_tensor(fill, dtype=dtype).reshape(rows, width).cuda()
    return t


@pytest.mark.parametrize("ns,keep_y", [(131, True), (119, False)])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_entries_through_the_c_abi(n, ns, keep_y):
    """Slot s owns corpus rows 4s .. 4s + 3 and feeds three of them; four frames.  Frame f: slot s primes when (s + f) % 3 == 0, else
    it produced a row, fired when (s + f) % 2 == 1; with n > 3 every fourth slot is idle from the start; on frame 2 every cursor reaches
    its end, on frame 3 all are idle.  Outputs against the header's statement in numpy; the shared outputs and the cursors bit-equal to
    tip_replay_collect on the same inputs; guard rows around every output untouched; the mask as stated."""
    lib, st = tlib.load(), torch.cuda.current_stream().cuda_stream
    rng = np.random.RandomState(n)
    nc, n_rows, stride = ns - 111, 4 * n, 1280 + 64
    cur = np.array([-1 if (n > 3 and s % 4 == 3) else 4 * s for s in range(n)], dtype=np.int64)
    end = np.array([4 * s + 3 for s in range(n)], dtype=np.int64)
    width = {"s": 111, "c": nc, "y": ns, "root": 3, "viz": 15, "q": 54, "cnt": 2}
    host = {k: rng.randn(n_rows, w).astype(f32) for k, w in width.items() if k != "cnt"}
    host["cnt"] = rng.randint(0, 50, (n_rows, 2)).astype(np.int32)
    host["v"], host["fire"] = np.full(n_rows, 7, np.uint8), np.full(n_rows, 7, np.uint8)
    dev = {k: _guarded(n_rows, w, host[k], torch.int32 if k == "cnt" else torch.float32, guard=-77 if k == "cnt" else float("nan"))
           for k, w in width.items()}
    dev["v"] = _guarded(n_rows, 1, host["v"], torch.uint8, guard=9)
    dev["fire"] = _guarded(n_rows, 1, host["fire"], torch.uint8, guard=9)
    twin = {k: dev[k].clone() for k in ("s", "c", "y", "v")}                     # tip_replay_collect's outputs, on the same inputs
    tbl = torch.tensor(np.stack([cur, end, cur, end])).cuda()                     # rows 0, 1: the tracked call's; 2, 3: the plain one's
    mask = torch.full((n + 2,), 9, dtype=torch.uint8, device="cuda")
    for f in range(4):
        rows_slot = np.array([-1 if (s + f) % 3 == 0 else 5 + s for s in range(n)], dtype=np.int32)
        t_fire = np.array([s if (s + f) % 2 == 1 else -1 for s in range(n)], dtype=np.int32)
        s_rest, c_t, y_slot = (rng.randn(n, w).astype(f32) for w in (111, nc, ns))
        t_root, t_viz, t_q = (rng.randn(n, w).astype(f32) for w in (3, 15, 54))
        blocks = rng.randint(0, 255, (n, stride)).astype(np.uint8)
        counters = blocks[:, 1208:1216].copy().view(np.int32)
        d = [torch.tensor(x).cuda() for x in (s_rest, c_t, y_slot, rows_slot, t_root, t_viz, t_q, t_fire, blocks)]
        before = cur.copy()
        assert lib.tip_replay_mask(tbl[0].data_ptr(), d[3].data_ptr(), n, mask[1:].data_ptr(), st) == 0
        assert lib.tip_replay_collect_tracked(
            tbl[0].data_ptr(), tbl[1].data_ptr(), n, n_rows, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), ns,
            dev["s"][1:].data_ptr(), dev["c"][1:].data_ptr(), dev["y"][1:].data_ptr() if keep_y else None, dev["v"][1:].data_ptr(),
            d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), d[8].data_ptr(), stride,
            dev["root"][1:].data_ptr(), dev["viz"][1:].data_ptr(), dev["q"][1:].data_ptr(), dev["fire"][1:].data_ptr(),
            dev["cnt"][1:].data_ptr(), st) == 0
        assert lib.tip_replay_collect(tbl[2].data_ptr(), tbl[3].data_ptr(), n, n_rows, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                      d[3].data_ptr(), ns, twin["s"][1:].data_ptr(), twin["c"][1:].data_ptr(),
                                      twin["y"][1:].data_ptr() if keep_y else None, twin["v"][1:].data_ptr(), st) == 0
        torch.cuda.synchronize()
        for s in range(n):                                                         # the header's statement
            c = cur[s]
            if c < 0:
                continue
            o = c + 1
            if rows_slot[s] >= 0:
                host["s"][o], host["c"][o], host["v"][o] = s_rest[s], c_t[s], 1
                host["root"][o], host["viz"][o], host["q"][o], host["fire"][o] = t_root[s], t_viz[s], t_q[s], t_fire[s] >= 0
                host["cnt"][o] = counters[s]
                if keep_y:
                    host["y"][o] = y_slot[s]
            else:
                host["s"][o], host["c"][o], host["v"][o] = host["s"][c], 0.0, 0
                host["root"][o], host["viz"][o], host["q"][o], host["fire"][o], host["cnt"][o] = host["root"][c], 100.0, host["q"][c], 0, host["cnt"][c]
                if keep_y:
                    host["y"][o] = np.nan
            cur[s] = -1 if o >= end[s] else o
        assert mask[1:-1].cpu().tolist() == [int(rows_slot[s] >= 0 and before[s] >= 0) for s in range(n)], f
        assert mask[0].item() == 9 and mask[-1].item() == 9
        assert tbl[0].cpu().tolist() == cur.tolist() and torch.equal(tbl[0], tbl[2]) and tbl[1].cpu().tolist() == end.tolist(), f
        for k in dev:
            got = dev[k][1:-1].cpu().numpy().reshape(host[k].shape)
            assert np.array_equal(_bits(got), _bits(host[k])), (f, k)
            g0, g1 = dev[k][0], dev[k][-1]
            assert bool((torch.isnan(g0) & torch.isnan(g1)).all()) if dev[k].dtype == torch.float32 else bool(((g0 == g1) & (g0 == (9 if k in ("v", "fire") else -77))).all()), (f, k)
        for k in twin:
            assert torch.equal(dev[k].view(torch.uint8), twin[k].view(torch.uint8)), (f, k)      # bit for bit, NaNs included
    assert (cur == -1).all()
    bad = torch.zeros(64, dtype=torch.uint8, device="cuda").data_ptr()
    assert lib.tip_replay_mask(None, bad, 1, bad, st) == -1 and lib.tip_replay_mask(bad, bad, 0, bad, st) == 0
    args = [bad, bad, 1, 4, bad, bad, bad, bad, 131, bad, bad, bad, bad, bad, bad, bad, bad, bad, 1280, bad, bad, bad, bad, bad]
    for k, v in ((0, None), (1, None), (2, -1), (3, -1), (4, None), (5, None), (7, None), (8, 120), (9, None), (10, None), (12, None), (13, None),
                 (14, None), (15, None), (16, None), (17, None), (18, 100), (19, None), (20, None), (21, None), (22, None), (23, None)):
        a = list(args)
        a[k] = v
        assert lib.tip_replay_collect_tracked(*a, st) == -1, k
    a = list(args)
    a[2] = 0
    assert lib.tip_replay_collect_tracked(*a, st) == 0


# ---- 2. multi_sbp off: the plain pool plus the post-pass ------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [2, 3])
def test_without_feedback_the_tracked_pool_is_the_plain_pool_plus_the_post_pass(model, skel, slots):
    recs, s0 = _recordings(LENGTHS)
    model.set_plan("fused")
    try:
        plain = replay.ReplayPool(model, slots=slots, use_graph=False, keep_y=True).run(recs, s0)
        pool = _pool(model, skel, slots, False)
        out = pool.run(recs, s0)
    finally:
        model.set_plan("auto")
    assert pool.frames == replay.plan_replay(LENGTHS, slots).n_frames and pool.restarts == 0 and pool.tracker.n == slots
    _check_conventions(out, recs, s0)
    offs = np.concatenate([[0], np.cumsum(LENGTHS)])
    root, viz, q_hist, fire, states = terrain.track_terrain(skel, s0, np.concatenate([r.s_rest for r in plain]),
                                                            np.concatenate([r.c_t for r in plain]), np.concatenate([r.valid for r in plain]),
                                                            offs, multi_sbp=False)
    torch.cuda.synchronize()
    root, viz, q_hist, fire = (t.cpu().numpy() for t in (root, viz, q_hist, fire))
    for i, r in enumerate(out):
        _same(r, plain[i], (slots, i), ("s_rest", "c_t", "valid", "y_last"))
        a, b = offs[i], offs[i + 1]
        assert np.array_equal(_bits(r.root), _bits(root[a:b])) and np.array_equal(_bits(r.viz_locs), _bits(viz[a:b])), i
        assert np.array_equal(_bits(r.q_hist), _bits(q_hist[a:b])) and np.array_equal(r.fire, fire[a:b] >= 0) and not r.fire.any(), i
        assert (r.off_map, r.regions_full) == (states[i].off_map, states[i].regions_full)
    assert not np.array_equal(out[0].root[6:], np.repeat(s0[0][None, :3], LENGTHS[0] - 6, 0))          # the root moved


# ---- 3. multi_sbp on: each recording equals itself run alone --------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [2, 3])
def test_with_feedback_every_recording_equals_itself_alone(model, skel, case, slots):
    recs, s0, alone, plain = case
    model.set_plan("fused")
    try:
        pool = _pool(model, skel, slots, True)
        out = pool.run(recs, s0)
    finally:
        model.set_plan("auto")
    plan = replay.plan_replay(LENGTHS, slots)
    assert pool.frames == plan.n_frames and pool.restarts == 0 and not any(pool.engine.attached)
    _check_conventions(out, recs, s0)
    for i in range(len(recs)):
        _same(out[i], alone[i], (slots, i))
    # from the device's own fire: the IK fired; a slot that had fired took another recording afterwards (the reset); the feedback
    # reached the model — up to a recording's first fired row the plain pool's rows, behind it not
    assert sum(int(r.fire.sum()) for r in out) >= 5
    took_over = [i for i in range(len(recs)) if LENGTHS[i] > 1 and any(
        plan.slot[j] == plan.slot[i] and 0 <= plan.start[j] < plan.start[i] and out[j].fire.any() for j in range(len(recs)))]
    assert took_over, "no slot that fired took another recording"
    reached = 0
    for i, r in enumerate(out):
        if not r.fire.any():
            assert np.array_equal(_bits(r.s_rest), _bits(plain[i].s_rest)), i
            continue
        t = int(np.nonzero(r.fire)[0][0])
        assert np.array_equal(_bits(r.s_rest[:t + 1]), _bits(plain[i].s_rest[:t + 1])), i
        if t + 1 < LENGTHS[i]:
            assert (r.s_rest[t + 1:] != plain[i].s_rest[t + 1:]).any(), i
            reached += 1
    assert reached >= 2


# ---- 4. graph mode ---------------------------------------------------------------------------------------------------------------------
def test_graph_mode_equals_launch_by_launch(model, skel):
    """Captured tracked frames (feed -> the engine's frame -> mask -> terrain step -> override -> tracked collect, one capture per bucket
    met) give the launch-by-launch bits under AUTO, every array; a second run re-captures and gives them again."""
    recs, s0 = _recordings(LENGTHS)
    ref_pool = _pool(model, skel, 3, True)
    ref = ref_pool.run(recs, s0)
    pool = _pool(model, skel, 3, True, use_graph=True)
    out = pool.run(recs, s0)
    plan = replay.plan_replay(LENGTHS, 3)
    assert pool.frames == ref_pool.frames == plan.n_frames
    k_at = [sum(1 for i, L in enumerate(LENGTHS) if L > 1 and plan.start[i] <= f <= plan.start[i] + L - 2) for f in range(plan.n_frames)]
    assert pool.engine.captures == len({pool.engine.bucket(k) for k in k_at})
    assert sum(int(r.fire.sum()) for r in out) >= 5
    for i in range(len(recs)):
        _same(out[i], ref[i], i)
    again = pool.run(recs, s0)
    for i in range(len(recs)):
        _same(again[i], ref[i], ("second run", i))


# ---- 5. no host traffic, the launch budget ---------------------------------------------------------------------------------------------
def _count_calls(monkeypatch, lib, calls):
    for name in tlib.EXPORTS:
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _f=fn, _n=name: (calls.append(_n), _f(*a))[1])


def test_no_per_frame_host_traffic_and_the_launch_budget(model, skel, monkeypatch):
    """Launch by launch, 3 slots: every frame through the device-fed method, the host-fed step paths and the tracker's host-side step
    arguments never entered, attach / detach and the tracker's resets on exactly the frames of the plan — and the C-ABI calls of one
    steady frame: the plain fed frame's, with tip_replay_collect replaced by tip_replay_collect_tracked and three more in front of it."""
    recs, s0 = _recordings(LENGTHS)
    plan = replay.plan_replay(LENGTHS, 3)
    per_frame = {}
    for tracked in (False, True):
        pool = _pool(model, skel, 3, True) if tracked else replay.ReplayPool(model, slots=3, use_graph=False, keep_y=True)
        eng = pool.engine

        def never(*a, **k):
            raise AssertionError("a host-fed step path was taken")

        monkeypatch.setattr(eng, "step", never)
        monkeypatch.setattr(eng, "_step_compact", never)
        monkeypatch.setattr(eng, "override_history", never)
        events, calls, marks = [], [], []
        base = eng.fed_frames
        real_attach, real_detach, real_step = eng.attach, eng.detach, eng._step_fed
        monkeypatch.setattr(eng, "attach", lambda sl, rows: (events.append(("a", eng.fed_frames - base, list(sl))), real_attach(sl, rows))[1])
        monkeypatch.setattr(eng, "detach", lambda sl: (events.append(("d", eng.fed_frames - base, list(sl))), real_detach(sl))[1])
        if tracked:
            real_reset = pool.tracker.reset
            monkeypatch.setattr(pool.tracker, "reset", lambda sl, rows: (events.append(("r", eng.fed_frames - base, list(sl), np.array(rows))),
                                                                          real_reset(sl, rows))[1])

        def step_fed():
            a = len(calls)
            r = real_step()
            marks.append((a, len(calls)))
            return r

        monkeypatch.setattr(eng, "_step_fed", step_fed)
        _count_calls(monkeypatch, pool.lib, calls)
        n0 = model.hip_forward_count()
        out = pool.run(recs, s0)
        monkeypatch.undo()
        assert pool.frames == plan.n_frames == len(marks) and model.hip_forward_count() - n0 == pool.frames
        want = []
        for f, (att, det) in enumerate(plan.frames):
            want += [("d", f, list(det))] if det else []
            want += [("a", f, [s for s, _ in att])] if att else []
        want += [("d", plan.n_frames, list(plan.final_detach))]
        assert [e[:3] for e in events if e[0] != "r" and e[2]] == want
        if tracked:
            resets = [e for e in events if e[0] == "r"]
            att_frames = [(f, sorted(att)) for f, (att, _) in enumerate(plan.frames) if att]
            assert [(e[1], e[2]) for e in resets] == [(f, [s for s, _ in att]) for f, att in att_frames]
            for e, (f, att) in zip(resets, att_frames):
                assert np.array_equal(e[3], s0[[i for _, i in att]])
            assert sum(int(r.fire.sum()) for r in out) >= 5
        steady = next(f for f, (att, det) in enumerate(plan.frames) if f > 8 and not att and not det)
        a, b = marks[steady]
        per_frame[tracked] = calls[a:b]
    plain, tracked = per_frame[False], per_frame[True]
    print("one steady frame, plain:", plain, "\n tracked:", tracked)
    assert plain[0] == "tip_replay_feed" and plain[-1] == "tip_replay_collect"
    assert tracked[:len(plain) - 1] == plain[:-1]
    assert tracked[len(plain) - 1:] == ["tip_replay_mask", "tip_terrain_track", "tip_stream_history_override", "tip_replay_collect_tracked"]
    assert len(tracked) - len(plain) == 3


# ---- 6. the lost hand-off --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
def test_lost_handoff_restarts_recordings_and_tracker_blocks(model, skel, case, monkeypatch, use_graph):
    """A loss simulated on the host exactly as tests/test_replay_gpu.py does (launch mode: the model's demotion counter moves during a
    forward; graph mode: the poll before a replay raises; no launch is disturbed): the recordings in flight start over, their tracker
    blocks with them, and the run ends on the undisturbed run's rows, the new arrays included."""
    m = model
    recs, s0, alone, _ = case
    plan = replay.plan_replay(LENGTHS, 3)
    LOSS = 20
    in_flight = [i for i, L in enumerate(LENGTHS) if L > 1 and plan.start[i] <= LOSS <= plan.start[i] + L - 2]
    assert len(in_flight) == 3 and any(alone[i].fire[:LOSS - plan.start[i]].any() for i in in_flight)      # the IK had fired before the loss
    m.set_plan("fused")
    d0 = m.demotions
    try:
        pool = _pool(m, skel, 3, True, use_graph=use_graph)
        eng = pool.engine
        state = {"f": -1}
        real_step = eng._step_fed
        resets = []
        real_reset = pool.tracker.reset
        monkeypatch.setattr(pool.tracker, "reset", lambda sl, rows: (resets.append(list(sl)), real_reset(sl, rows))[1])

        def step_fed():
            state["f"] += 1
            if state["f"] == LOSS:
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
            out = pool.run(recs, s0)
        finally:
            monkeypatch.undo()
            m.demotions = d0
        assert pool.restarts == len(in_flight)
        assert sorted(plan.slot[i] for i in in_flight) in resets                  # the blocks of the restarted recordings, in one reset
        for i in range(len(recs)):
            _same(out[i], alone[i], i)
        out = pool.run(recs, s0)                                                  # the pool is usable afterwards
        assert pool.restarts == 0
        for i in range(len(recs)):
            _same(out[i], alone[i], ("after", i))
    finally:
        m.set_plan("auto")
        m.demotions = d0


# ---- 7. more slots than a wave ---------------------------------------------------------------------------------------------------------
def test_sixty_five_slots(model, skel):
    lengths = [8 + (i % 5) for i in range(66)]
    recs, s0 = _recordings(lengths, seed0=900)
    model.set_plan("fused")
    try:
        pool = _pool(model, skel, 65, True)
        out = pool.run(recs, s0)
        alone = [_alone(model, skel, r, s0[i], True) for i, r in enumerate(recs)]
    finally:
        model.set_plan("auto")
    _check_conventions(out, recs, s0)
    assert pool.plan.slot[65] == pool.plan.slot[0] and pool.plan.start[65] == lengths[0] - 1          # the 66th takes the first free slot
    for i in range(66):
        _same(out[i], alone[i], i)
    assert sum(int(r.fire.sum()) for r in out) >= 20


# ---- 8. a small map, a short region list -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("map_bound,max_regions", [(1.0, 64), (1.0, 4), (5.0, 4), (5.0, 2)])
def test_small_map_and_short_region_list(model, skel, map_bound, max_regions):
    """Recordings of 64 .. 70 frames (a held contact writes the map when its tick runs out, 51 frames on) whose characters stand at
    different places, two of them where a patch does not fit a map 20 cells a side: off_map and regions_full per recording are what
    tests/terrain_oracle.py counts on the recording's own rows, and what the recording run alone gives."""
    lengths = (70, 64, 66, 68)
    recs, s0 = _recordings(lengths, seed0=800)
    s0 = s0.copy()
    s0[:, 0], s0[:, 1] = [0.1, 0.75, -0.2, -0.8], [0.0, 0.1, 0.72, -0.1]
    model.set_plan("fused")
    try:
        pool = _pool(model, skel, 2, True, map_bound=map_bound, max_regions=max_regions)
        out = pool.run(recs, s0)
        alone = [_alone(model, skel, r, s0[i], True, map_bound=map_bound, max_regions=max_regions) for i, r in enumerate(recs)]
    finally:
        model.set_plan("auto")
    assert pool.tracker.state(0).region_map.shape == ((20, 20) if map_bound == 1.0 else (100, 100))
    total = full = 0
    for i, r in enumerate(out):
        _same(r, alone[i], i)
        o = to.track(TABLE, s0[i], r.s_rest, r.c_t, r.valid, map_bound, 0.1, True, max_regions)
        print(f"map_bound {map_bound} max_regions {max_regions} recording {i}: off_map {r.off_map} regions_full {r.regions_full}; oracle "
              f"{o[4].off_map} {o[4].regions_full}; updates {sum(o[5]['counts'][k] for k in ('merge', 'new', 'region0'))}; "
              f"smallest margin {min(o[5]['margins'].values()):.2e}")
        assert (r.off_map, r.regions_full) == (o[4].off_map, o[4].regions_full), i
        total += r.off_map
        full += r.regions_full
    # (the CPU oracle composition counts 0, 3, 2 and 3 updates off the small map, and three new regions in recordings 1 and 3)
    if map_bound == 1.0:
        assert total >= 2 and out[0].off_map == 0
    else:
        assert total == 0 and (full >= 2) == (max_regions == 2)


# ---- 9, 10. another window, a two-SBP model -----------------------------------------------------------------------------------------------
def test_window_24(model, skel):
    lengths = [7, 33, 12, 40]                    # window 24 fills at frame 28
    recs, s0 = _recordings(lengths, seed0=400)
    model.set_plan("fused")
    try:
        alone = [_alone(model, skel, r, s0[i], True, window=24) for i, r in enumerate(recs)]
        pool = _pool(model, skel, 2, True, window=24)
        out = pool.run(recs, s0)
    finally:
        model.set_plan("auto")
    assert pool.engine.window == 24
    _check_conventions(out, recs, s0)
    for i in range(len(recs)):
        _same(out[i], alone[i], i)
    assert sum(int(r.fire.sum()) for r in out) >= 5


def test_two_sbp_model(skel):
    m = _shifted_model(NARROW).eval()
    lengths = [7, 33, 12, 40]
    recs, s0 = _recordings(lengths, seed0=400)
    with pytest.raises(ValueError, match="two-SBP"):
        _pool(m, skel, 2, True)
    m.set_plan("fused")
    try:
        plain = replay.ReplayPool(m, slots=2, use_graph=False, keep_y=True).run(recs, s0)
        out = _pool(m, skel, 2, False).run(recs, s0)
    finally:
        m.set_plan("auto")
    _check_conventions(out, recs, s0)
    offs = np.concatenate([[0], np.cumsum(lengths)])
    root, viz, q_hist, fire, _ = terrain.track_terrain(skel, s0, np.concatenate([r.s_rest for r in plain]), np.concatenate([r.c_t for r in plain]),
                                                       np.concatenate([r.valid for r in plain]), offs, multi_sbp=False)
    torch.cuda.synchronize()
    for i, r in enumerate(out):
        assert r.c_t.shape == (lengths[i], 8) and r.y_last.shape == (lengths[i], 119)
        _same(r, plain[i], i, ("s_rest", "c_t", "valid", "y_last"))
        a, b = offs[i], offs[i + 1]
        assert np.array_equal(_bits(r.root), _bits(root[a:b].cpu().numpy())) and np.array_equal(_bits(r.viz_locs), _bits(viz[a:b].cpu().numpy()))
        assert np.array_equal(_bits(r.q_hist), _bits(q_hist[a:b].cpu().numpy())) and not r.fire.any()


def test_refusals(model, skel):
    with pytest.raises(ValueError, match="terrain is dict"):
        replay.ReplayPool(model, slots=2, terrain=dict(skel=skel, map_bound=5.0, grid_size=0.1, cells=3))
    with pytest.raises(ValueError, match="terrain is dict"):
        replay.ReplayPool(model, slots=2, terrain=dict(map_bound=5.0, grid_size=0.1))
    table = {k: np.array(v) for k, v in TABLE.items()}
    knee = int(table["parent"][int(table["sbp"][0]) - 1])
    table["state_col"] = table["state_col"].copy()
    table["state_col"][knee - 1] = -1                                              # a welded knee: not three spherical links
    broken = kin.Skeleton.from_table({"table/" + k: v for k, v in table.items()})
    with pytest.raises(ValueError, match="three spherical links"):
        replay.ReplayPool(model, slots=2, terrain=dict(skel=broken, map_bound=5.0, grid_size=0.1, multi_sbp=True))
    plain = replay.ReplayPool(model, slots=2)
    assert plain.tracker is None


# ---- 11. the deployed model: dropout live --------------------------------------------------------------------------------------------------
def test_live_dropout_pool(skel):
    m = _shifted_model(p_state=0.8, dropout=0.1).train()
    lengths = [20, 7, 50]
    recs, s0 = _recordings(lengths, seed0=500)
    runs = []
    for use_graph in (True, False):
        pool = _pool(m, skel, 2, True, use_graph=use_graph, live_dropout=True)
        torch.manual_seed(7)
        runs.append(pool.run(recs, s0))
    for out in runs:
        _check_conventions(out, recs, s0)
        for r in out:
            assert np.isfinite(r.s_rest).all() and np.isfinite(r.c_t).all() and np.isfinite(r.y_last[r.valid]).all()
            assert np.isfinite(r.root).all() and np.isfinite(r.viz_locs).all() and np.isfinite(r.q_hist).all()
    for i in range(len(recs)):
        _same(runs[0][i], runs[1][i], i)


# ---- 12. the reference's closed loop -----------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(LOOP_PATH), reason="tests/golden/make_terrain_loop_golden.py found no qualifying seed")
@pytest.mark.parametrize("use_graph", [False, True])
def test_pool_tracks_the_reference_closed_loop(model, skel, use_graph):
    """The fixture's recording between two synthetic ones, two slots: over F_cmp rows the pool follows the real RTRunner.step around
    the reference's own model with the IK feedback in the loop.  s_rest, y_last and the fed-back pose on fired rows within TOL_LOOP;
    fire flags and contact flags equal; root and viz_locs within 3 x the error, against the fixture, of the SAME LOOP restated in numpy
    float32 on the same weights and frames (the fixture's f32/*: the forward oracle and terrain_oracle in float32 — the device's
    tracker reads the rows of a float32 network, so the floor is the loop's, not that of a tracker teacher-forced on fp64 rows, which
    is 6.6e-07 for the root and which the device's 2.2e-06 does not meet).
    Measured on an MI355X, both modes alike, 127 fired rows of 160, every fire flag equal: s_rest 2.01e-05, y_last 2.44e-06,
    c_t 2.09e-07, q_hist on fired rows 2.07e-05 (TOL_LOOP 5e-04); root fp32 noise 2.61e-06 / device error 2.19e-06, viz_locs
    6.21e-06 / 7.12e-06."""
    g = np.load(LOOP_PATH)
    assert np.array_equal(g["bias_index"], rto.BIAS_INDEX) and np.allclose(g["bias_shift"], rto.BIAS_SHIFT)
    F = int(g["F_cmp"][0])
    syn, s_syn = _recordings([31, 80], seed0=300)
    recs = [syn[0], g["raw_imu"][:F].astype(f32), syn[1]]
    s0 = np.stack([s_syn[0], g["s_init"].astype(f32), s_syn[1]])
    out = _pool(model, skel, 2, True, use_graph=use_graph).run(recs, s0)
    _check_conventions(out, recs, s0)
    r, v = out[1], g["valid"][:F]
    assert np.array_equal(r.valid, v)
    err = {"s_rest": np.abs(r.s_rest - g["qdq"][:F, 3:]).max(), "y_last": np.abs(r.y_last[v] - g["y_last"][:F][v]).max(),
           "c_t": np.abs(r.c_t - g["ct"][:F]).max()}
    fired = g["fire"][:F]
    err["q_hist"] = np.abs(r.q_hist[fired] - g["q_hist"][:F][fired]).max()
    noise = {"root": float(np.abs(g["f32/root"].astype(np.float64) - g["qdq"][:F, :3]).max()),
             "viz_locs": float(np.abs(g["f32/viz_locs"].astype(np.float64) - g["viz_locs"][:F]).max())}
    dev = {"root": float(np.abs(r.root.astype(np.float64) - g["qdq"][:F, :3]).max()),
           "viz_locs": float(np.abs(r.viz_locs.astype(np.float64) - g["viz_locs"][:F]).max())}
    print(f"closed loop against the reference, use_graph={use_graph}, F_cmp {F}, fired rows {int(fired.sum())} (device {int(r.fire.sum())}): "
          + "  ".join(f"{k} {x:.3e}" for k, x in err.items())
          + "  " + "  ".join(f"{k} fp32 noise {noise[k]:.3e} device error {dev[k]:.3e}" for k in noise))
    flips = np.nonzero(r.fire != fired)[0]
    assert flips.size == 0, ("fire flags differ on rows", flips.tolist())
    assert np.array_equal(r.c_t[:, 0::4], g["ct"][:F, 0::4])
    for k in ("s_rest", "y_last", "c_t", "q_hist"):
        assert err[k] < TOL_LOOP, (k, err[k])
    for k in noise:
        assert dev[k] <= 3.0 * noise[k], (k, dev[k], noise[k])


# ---- 13. end to end ------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_metrics(model, skel):
    """ReplayPool(terrain=...) -> trim_like_reference(r.qdq) -> kinematics.evaluate; with multi_sbp off it is the same call on
    kinematics.track_replay's rows."""
    lengths = (70, 48)
    recs, s0 = _recordings(lengths)
    rng = np.random.RandomState(1)
    offs = np.array([0, 70, 118])
    model.set_plan("fused")
    try:
        plain = replay.ReplayPool(model, slots=2, use_graph=False).run(recs, s0)
        off = _pool(model, skel, 2, False).run(recs, s0)
        on = _pool(model, skel, 2, True).run(recs, s0)
    finally:
        model.set_plan("auto")
    post = kin.track_replay(skel, plain, s0, terrain=dict(map_bound=5.0, grid_size=0.1))
    gt = np.concatenate([np.repeat(s0[i][None], L, 0) for i, L in enumerate(lengths)]) + 0.01 * rng.randn(118, 114).astype(f32)
    m_post = kin.evaluate(skel, np.concatenate([replay.trim_like_reference(q) for q, _ in post]), gt, offs)
    m_off = kin.evaluate(skel, np.concatenate([replay.trim_like_reference(r.qdq) for r in off]), gt, offs)
    m_on = kin.evaluate(skel, np.concatenate([replay.trim_like_reference(r.qdq) for r in on]), gt, offs)
    assert m_off.shape == (2, 7) and np.array_equal(m_off, m_post)
    for i, (q, viz) in enumerate(post):
        assert np.array_equal(_bits(q), _bits(off[i].qdq)) and np.array_equal(_bits(viz), _bits(off[i].viz_locs))
    assert np.isfinite(m_on).all() and not np.array_equal(m_on, m_off)
