"""tip_amd.terrain on the device (csrc/tip_terrain.hip) against tests/terrain_oracle.py and the reference-generated golden
(tests/golden/tip_terrain_golden.npz: the real RTRunner.step, teacher-forced).  The skeleton comes from the golden's table only.
Discrete state — region map, ticks, region count, fire, the two counters — must be EQUAL; continuous values may differ from the fp64
reference by at most 3 x the error of the same restatement in numpy float32 on the same inputs, per kind of output
(tests/test_kin_gpu.py's rule).

Measured on an MI355X (test 1, the worst of the three tracks and both modes, one call and live alike; fp32 noise / device error):
    root 1.05e-06 / 1.07e-06   viz_locs 4.11e-06 / 4.03e-06 (the markers at 100: one float32 rounding of the output)
    q_hist 5.36e-06 / 5.24e-06   region_height 4.10e-07 / 1.39e-07   ik_deltas 1.87e-07 / 1.84e-07"""
import numpy as np
import pytest
import torch

import terrain_oracle as to
import tip_amd
from tip_amd import kinematics as kin
from tip_amd import synth, terrain
from test_host_cpu import make_model, load_synth
from test_terrain_cpu import golden_track

pytestmark = pytest.mark.gpu
f32 = np.float32
GOLDEN = np.load(__file__.replace("test_terrain_gpu.py", "golden/tip_terrain_golden.npz"))
TABLE = {k[len("table/"):]: GOLDEN[k] for k in GOLDEN.files if k.startswith("table/")}
TRACKS = ("track0", "track1", "track2")
LENGTHS = (70, 48, 8, 7)          # 70 crosses the 64-row FK batch; 7: five priming rows and two valid ones
KINDS = ("root", "viz_locs", "q_hist", "region_height", "ik_deltas")


@pytest.fixture(scope="module")
def skel():
    return kin.Skeleton.from_table(GOLDEN)


def _np(*tensors):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def _case(tag, multi):
    """A golden track as the float32 the device gets, and what the reference made of it."""
    s_init, s_rest, ct, valid, exp = golden_track(GOLDEN, tag, multi)
    return s_init.astype(f32), s_rest.astype(f32), ct.astype(f32), valid, exp


def _errors(root, viz, q_hist, st, exp):
    """Per kind of output, the largest distance from the reference; q_hist on the rows the reference fired on."""
    rows = exp["fire_rows"]
    return {"root": float(np.abs(root - exp["root"]).max()), "viz_locs": float(np.abs(viz - exp["viz_locs"]).max()),
            "q_hist": float(np.abs(q_hist[rows] - exp["q_hist"][rows]).max()) if len(rows) else 0.0,
            "region_height": float(np.abs(np.asarray(st.region_height, dtype=np.float64) - exp["region_height"]).max()),
            "ik_deltas": float(np.abs(np.asarray(st.ik_deltas, dtype=np.float64) - exp["ik_deltas"]).max())}


def _live(skel, cases, multi, map_bound=5.0, max_regions=64):
    """TerrainTracker.step frame by frame over sequences of different lengths, one per slot: the rows each slot produced, stacked back
    to back as track_terrain returns them, and the tracker."""
    n = len(cases)
    tt = terrain.TerrainTracker(skel, n, "cuda", map_bound, 0.1, multi_sbp=multi, max_regions=max_regions)
    tt.reset(None, np.stack([c[0] for c in cases]))
    lens = [c[1].shape[0] for c in cases]
    nc = cases[0][2].shape[1]
    s_rest, c_t, valid = np.zeros((max(lens), n, 111), f32), np.zeros((max(lens), n, nc), f32), np.zeros((max(lens), n), bool)
    for i, c in enumerate(cases):
        s_rest[:lens[i], i], c_t[:lens[i], i], valid[:lens[i], i] = c[1], c[2], c[3]
    sd, cd, vd = torch.from_numpy(s_rest).cuda(), torch.from_numpy(c_t).cuda(), torch.from_numpy(valid).cuda()
    outs = [[] for _ in range(n)]
    for t in range(max(lens)):
        alive = [i for i in range(n) if t < lens[i]]
        tt.step({"s_rest": sd[t], "c_t": cd[t], "valid": vd[t]}, None if len(alive) == n else alive)
        row = [x.clone() for x in (tt.root, tt.viz_locs, tt.q_hist, tt.fire)]
        for i in alive:
            outs[i].append([x[i] for x in row])
    cat = [torch.stack([r[k] for o in outs for r in o]) for k in range(4)]
    return _np(*cat), tt


# ---- 1. the golden tracks, teacher-forced, both modes --------------------------------------------------------------------------------
@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("tag", TRACKS)
def test_golden_tracks_in_one_call_and_frame_by_frame(skel, tag, multi):
    s_init, s_rest, ct, valid, exp = _case(tag, multi)
    n = s_rest.shape[0]
    lo = to.track(TABLE, s_init, s_rest, ct, valid, 5.0, 0.1, multi, 64, dtype=f32)
    noise = _errors(lo[0].astype(np.float64), lo[1].astype(np.float64), lo[2].astype(np.float64), lo[4], exp)
    out = terrain.track_terrain(skel, s_init[None], s_rest, ct, valid, [0, n], multi_sbp=multi)
    (live, tt) = _live(skel, [(s_init, s_rest, ct, valid)], multi)
    for name, (root, viz, q_hist, fire), st in (("one call", _np(*out[:4]), out[4][0]), ("live", live, tt.state(0))):
        err = _errors(root.astype(np.float64), viz.astype(np.float64), q_hist.astype(np.float64), st, exp)
        print(f"{tag} multi={int(multi)} {name}: " + "   ".join(f"{k} fp32 noise {noise[k]:.3e} device error {err[k]:.3e}" for k in KINDS))
        assert np.array_equal(fire >= 0, exp["fire"]) and (fire[exp["fire"]] == 0).all()
        assert np.array_equal(st.region_map, exp["region_map"]) and st.n_regions == len(exp["region_height"])
        assert np.array_equal(st.ticks, exp["ticks"][-1]) and st.off_map == 0 and st.regions_full == 0
        assert np.array_equal(st.region_weight, exp["region_weight"])
        assert np.array_equal(st.height_map, st.region_height[st.region_map])
        for k in KINDS:
            assert err[k] <= 3.0 * noise[k], (name, k, err[k], noise[k])
        assert (viz[~valid] == 100).all() and (root[~valid] == s_init[:3]).all()
        assert np.array_equal(q_hist[~exp["fire"]], s_rest[~exp["fire"], :54])


# ---- 2, 3. chunking, the carry, ragged sequences, isolation --------------------------------------------------------------------------
def _ragged(R, nc=20):
    """R sequences of LENGTHS in turn: rows of the golden tracks from their start (so that the priming rows lead), with the foot
    offsets of each sequence scaled a little differently so that no two are alike."""
    seqs = []
    for i in range(R):
        s_init, s_rest, ct, valid, _ = _case(TRACKS[(i + 2) % 3], True)      # (the standing track, whose IK fires early, gets the 70 rows)
        n = LENGTHS[i % len(LENGTHS)]
        ct = ct[:n].copy()
        ct[:, 1::4] *= f32(1.0 + 0.01 * i)
        seqs.append((s_init, s_rest[:n], ct[:, :nc], valid[:n]))
    offs = np.concatenate([[0], np.cumsum([s[1].shape[0] for s in seqs])]).astype(np.int64)
    return seqs, offs


def _run(skel, seqs, offs, multi, **kw):
    out = terrain.track_terrain(skel, np.stack([s[0] for s in seqs]), np.concatenate([s[1] for s in seqs]), np.concatenate([s[2] for s in seqs]),
                                np.concatenate([s[3] for s in seqs]), offs, multi_sbp=multi, **kw)
    return _np(*out[:4]), out[4].bytes


@pytest.fixture(scope="module")
def three(skel):
    seqs, offs = _ragged(3)
    return seqs, offs, _run(skel, seqs, offs, True)


@pytest.mark.parametrize("chunk", [1, 7, 64, 65])
def test_chunks_give_the_bits_of_the_single_call(skel, three, chunk):
    seqs, offs, (ref, ref_bytes) = three
    got, got_bytes = _run(skel, seqs, offs, True, chunk=chunk)
    for a, b, name in zip(got, ref, ("root", "viz_locs", "q_hist", "fire")):
        assert np.array_equal(a, b), name
    assert np.array_equal(got_bytes, ref_bytes)
    assert (ref[3] >= 0).sum() >= 3                                   # the IK fired inside these rows


def test_live_tracker_gives_the_bits_of_the_single_call(skel, three):
    seqs, offs, (ref, ref_bytes) = three
    got, tt = _live(skel, seqs, True)
    for a, b, name in zip(got, ref, ("root", "viz_locs", "q_hist", "fire")):
        assert np.array_equal(a, b), name
    assert np.array_equal(tt.state_bytes(), ref_bytes)


@pytest.mark.parametrize("R", [3, 66])
def test_ragged_sequences_equal_themselves_run_alone(skel, R):
    seqs, offs = _ragged(R)
    (root, viz, q_hist, fire), blocks = _run(skel, seqs, offs, True)
    for i in sorted(set(range(min(R, 12))) | {R - 1}):                   # all twelve (track, length) pairs, and the last sequence
        (r1, v1, q1, f1), b1 = _run(skel, [seqs[i]], np.array([0, seqs[i][1].shape[0]]), True)
        a, b = offs[i], offs[i + 1]
        assert np.array_equal(root[a:b], r1) and np.array_equal(viz[a:b], v1) and np.array_equal(q_hist[a:b], q1), i
        assert np.array_equal(fire[a:b] >= 0, f1 >= 0) and (fire[a:b][f1 >= 0] == i).all(), i
        assert np.array_equal(blocks[i], b1[0]), i


def test_stepping_a_subset_leaves_the_other_slots_alone(skel, three):
    seqs, _, _ = three
    tt = terrain.TerrainTracker(skel, 3, "cuda", multi_sbp=True)
    tt.reset(None, np.stack([s[0] for s in seqs]))
    rows = {k: torch.from_numpy(np.stack([s[i][:8] for s in seqs], axis=1)).cuda() for k, i in (("s_rest", 1), ("c_t", 2), ("valid", 3))}
    for t in range(7):
        tt.step({k: v[t] for k, v in rows.items()})
    before = tt.state_bytes()
    tt.fire[:] = 1                                                     # a stale entry must not survive a subset step
    tt.step({k: v[7] for k, v in rows.items()}, [1])
    after = tt.state_bytes()
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2]) and not np.array_equal(after[1], before[1])
    assert tt.fire[0].item() == -1 and tt.fire[2].item() == -1


# ---- 4, 5. a small map and a short region list --------------------------------------------------------------------------------------
def walking_case():
    """The standing track with the right foot's contact walked out along x, 1 m over the track: on a 20-cell map (map_bound 1.0, half
    of it a patch) its updates leave the map one after the other."""
    s_init, s_rest, ct, valid, _ = _case("track2", True)
    ct = ct.copy()
    ct[:, 5] += np.linspace(0, 1.0, ct.shape[0]).astype(f32)
    return s_init, s_rest, ct, valid


def stairs_case():
    """The standing track with the right foot's contact raised by 0.25 m every 24 frames: a new region each time."""
    s_init, s_rest, ct, valid, _ = _case("track2", True)
    ct = ct.copy()
    ct[:, 7] += (0.25 * (np.arange(ct.shape[0]) // 24)).astype(f32)
    return s_init, s_rest, ct, valid


def _against_oracle(skel, case, multi, map_bound, max_regions, slot_of=1):
    """`case` on slot 1 of a three-slot tracker (the others reset and left alone), against the fp64 oracle on the same float32 rows:
    discrete state equal, continuous within 3 x float32 noise; the neighbours' bytes unchanged.  Returns the oracle's state and trace."""
    s_init, s_rest, ct, valid = case
    ref = to.track(TABLE, s_init, s_rest, ct, valid, map_bound, 0.1, multi, max_regions)
    low = to.track(TABLE, s_init, s_rest, ct, valid, map_bound, 0.1, multi, max_regions, dtype=f32)
    assert min(ref[5]["margins"].values()) >= 1e-4, ref[5]["margins"]       # the case is sound: no decision at the mercy of rounding
    tt = terrain.TerrainTracker(skel, 3, "cuda", map_bound, 0.1, multi_sbp=multi, max_regions=max_regions)
    tt.reset(None, np.stack([s_init] * 3))
    before = tt.state_bytes()
    sd, cd, vd = (torch.from_numpy(np.repeat(x[:, None], 3, axis=1)).cuda() for x in (s_rest, ct, valid))
    got = []
    for t in range(s_rest.shape[0]):
        tt.step({"s_rest": sd[t], "c_t": cd[t], "valid": vd[t]}, [slot_of])
        got.append([x[slot_of].clone() for x in (tt.root, tt.viz_locs, tt.q_hist, tt.fire)])
    root, viz, q_hist, fire = _np(*[torch.stack([g[k] for g in got]) for k in range(4)])
    after = tt.state_bytes()
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])
    st, ost = tt.state(slot_of), ref[4]
    assert np.array_equal(st.region_map, ost.region_map) and np.array_equal(st.d2_map, ost.d2_map)
    assert np.array_equal(st.ticks, ost.ticks) and st.n_regions == len(ost.region_height)
    assert (st.off_map, st.regions_full) == (ost.off_map, ost.regions_full)
    assert np.array_equal(fire >= 0, ref[3])
    finite = np.isfinite(ref[0]).all(axis=1)
    for name, a, k in (("root", root, 0), ("viz_locs", viz, 1), ("q_hist", q_hist, 2)):
        noise = float(np.abs(low[k][finite].astype(np.float64) - ref[k][finite]).max())
        err = float(np.abs(a[finite].astype(np.float64) - ref[k][finite]).max())
        print(f"{name}: fp32 noise {noise:.3e} device error {err:.3e}")
        assert err <= 3.0 * noise, (name, err, noise)
    hn = float(np.abs(np.array(low[4].region_height, dtype=np.float64) - np.array(ost.region_height)).max())
    assert float(np.abs(st.region_height - np.array(ost.region_height)).max()) <= 3.0 * hn
    return st, ost, ref[5]


def test_small_map_updates_that_leave_the_map(skel):
    st, ost, tr = _against_oracle(skel, walking_case(), True, 1.0, 64)
    print("off_map", st.off_map, "updates inside", tr["counts"]["region0"] + tr["counts"]["merge"] + tr["counts"]["new"])
    assert st.region_map.shape == (20, 20) and st.off_map >= 3 and tr["counts"]["region0"] + tr["counts"]["new"] >= 3


def test_region_list_of_four(skel):
    st, ost, tr = _against_oracle(skel, stairs_case(), False, 5.0, 4)
    print("regions_full", st.regions_full, "regions", st.n_regions)
    assert st.n_regions == 4 and st.regions_full >= 3 and st.region_map.max() == 3
    # nothing was written past the fourth region: the map starts right behind region_weight[3], and it equals the oracle's
    assert len(st.region_height) == len(st.region_weight) == 4 and np.array_equal(st.region_weight, np.array(ost.region_weight))


# ---- 6. a non-finite row -------------------------------------------------------------------------------------------------------------
def test_non_finite_row_stays_in_its_slot(skel, three):
    seqs, offs, (ref, ref_bytes) = three
    bad = [tuple(x.copy() for x in s) for s in seqs]
    bad[1][1][20, 54] = np.nan                                          # the root velocity of row 20 of sequence 1
    bad[1][2][30, 1] = np.inf                                           # and, later, a contact offset
    (root, viz, q_hist, fire), blocks = _run(skel, bad, offs, True)
    for i in (0, 2):
        a, b = offs[i], offs[i + 1]
        assert np.array_equal(root[a:b], ref[0][a:b]) and np.array_equal(viz[a:b], ref[1][a:b]) and np.array_equal(q_hist[a:b], ref[2][a:b])
        assert np.array_equal(fire[a:b], ref[3][a:b]) and np.array_equal(blocks[i], ref_bytes[i])
    a = offs[1]
    assert np.isfinite(root[a:a + 20]).all() and np.isnan(root[a + 20:offs[2], 0]).all()      # (x: the column the NaN velocity feeds)
    s_init, s_rest, ct, valid = bad[1]
    o = to.track(TABLE, s_init, s_rest, ct, valid, 5.0, 0.1, True, 64)
    st = terrain.TerrainState(blocks[1], 100, 64)
    assert np.array_equal(st.region_map, o[4].region_map) and np.array_equal(st.d2_map, o[4].d2_map) and st.n_regions == len(o[4].region_height)
    assert np.array_equal(st.ticks, o[4].ticks) and st.off_map == o[4].off_map == 0


# ---- 7. plumbing: the tracker beside an engine ---------------------------------------------------------------------------------------
_model_cache = []


def _model():
    if not _model_cache:
        m = make_model(dict(synth.PAPER))
        load_synth(m, dict(synth.PAPER), 0)
        _model_cache.append(m.cuda().eval())
    return _model_cache[0]


def _frames(n, F, seed):
    rng = np.random.RandomState(seed)
    raw = rng.randn(F, n, 72).astype(f32)
    eye = np.eye(3, dtype=f32).reshape(9)
    raw[:, :, :54] = np.tile(eye, 6) + 0.05 * raw[:, :, :54]
    return torch.from_numpy(raw).cuda(), (rng.randn(n, 114) * 0.2).astype(f32)


@pytest.mark.parametrize("kind", ["lockstep", "staggered"])
def test_feed_back_equals_the_host_override(skel, kind):
    """Three engines on the same frames: A is corrected on the device (feed_back), B through the existing host override_history with
    the downloaded q_hist / fire, C as A under use_graph=True.  The trackers are fed fabricated frames — the golden tracks' rows, one
    track per slot — so that the IK fires on known frames whatever the synthetic model says."""
    S = tip_amd.streaming
    m, n, F = _model(), 3, 60
    raw, s_init = _frames(n, F, 3)
    make = (lambda **kw: S.StreamingEngine(m, s_init, **kw)) if kind == "lockstep" else (lambda **kw: S.StaggeredStreamingEngine(m, s_init, **kw))
    engines = [make(), make(), make(use_graph=True)]
    cases = [_case(t, True) for t in TRACKS]
    trackers = []
    for _ in engines:
        tt = terrain.TerrainTracker(skel, n, "cuda", multi_sbp=True)
        tt.reset(None, np.stack([c[0] for c in cases]))
        trackers.append(tt)
    rows = {k: torch.from_numpy(np.stack([c[i][5:5 + F] for c in cases], axis=1)).cuda() for k, i in (("s_rest", 1), ("c_t", 2))}
    ones = torch.ones(n, dtype=torch.bool, device="cuda")
    fired, k = 0, 0
    for f in range(F):
        outs = [e.step(raw[f]) for e in engines]
        if outs[0] is None or not bool(torch.as_tensor(outs[0].get("valid", True)).all()):
            continue
        torch.cuda.synchronize()
        for key in ("s_rest", "c_t", "y_last"):
            assert torch.equal(outs[0][key], outs[1][key]) and torch.equal(outs[0][key], outs[2][key]), (f, key)
        fab = {"s_rest": rows["s_rest"][k], "c_t": rows["c_t"][k], "valid": ones}
        k += 1
        for e, tt in zip(engines, trackers):
            tt.step(fab)
        trackers[0].feed_back(engines[0])
        trackers[2].feed_back(engines[2])
        q, fire = _np(trackers[1].q_hist, trackers[1].fire)
        sel = [int(s) for s in np.nonzero(fire >= 0)[0]]
        assert [int(fire[s]) for s in sel] == sel
        if sel:
            engines[1].override_history(q[sel], sel)
        fired += len(sel)
    print(kind, "frames corrected:", k, "rows the IK fired on:", fired)
    assert fired >= 5 and k >= 50
    m.check_handoffs()


def test_a_tracker_that_never_fires_leaves_the_engine_alone(skel):
    """The root's SBP flag 0 throughout: no root residue, no IK, fire -1 on every frame — feed_back is a launch that writes nothing."""
    S = tip_amd.streaming
    m, n, F = _model(), 3, 30
    raw, s_init = _frames(n, F, 4)
    bare, eng = S.StreamingEngine(m, s_init), S.StreamingEngine(m, s_init)
    cases = [_case(t, True) for t in TRACKS]
    tt = terrain.TerrainTracker(skel, n, "cuda", multi_sbp=True)
    tt.reset(None, np.stack([c[0] for c in cases]))
    rows = {k: torch.from_numpy(np.stack([c[i][5:5 + F] for c in cases], axis=1)).cuda() for k, i in (("s_rest", 1), ("c_t", 2))}
    rows["c_t"][:, :, 16] = 0
    assert tt.step(None)[0] is tt.root                                  # out=None: nothing launched
    k = 0
    for f in range(F):
        a, b = bare.step(raw[f]), eng.step(raw[f])
        if a is None:
            continue
        tt.step({"s_rest": rows["s_rest"][k], "c_t": rows["c_t"][k]})
        tt.feed_back(eng)
        k += 1
        torch.cuda.synchronize()
        assert (tt.fire == -1).all()
        for key in ("s_rest", "c_t", "y_last"):
            assert torch.equal(a[key], b[key]), (f, key)
    assert torch.equal(bare.state, eng.state) and k >= 20
    with pytest.raises(ValueError):
        eng.override_history_device(tt.q_hist.cpu(), tt.fire)
    with pytest.raises(ValueError):
        eng.override_history_device(tt.q_hist, tt.fire.long())


# ---- 8. two-SBP models ---------------------------------------------------------------------------------------------------------------
def test_two_sbp_models(skel):
    seqs, offs = _ragged(3, nc=8)
    (root, viz, q_hist, fire), blocks = _run(skel, seqs, offs, False)
    # the SBPs a two-SBP model lacks stay far away: 100 less the frame's xy correction, which :463 takes off every location
    assert (fire == -1).all() and (viz[:, 2:, 2] == 100).all() and (np.abs(viz[:, 2:, :2] - 100) <= 0.5 / 60 + 1e-5).all()
    for i, (s_init, s_rest, ct, valid) in enumerate(seqs):
        ref = to.track(TABLE, s_init, s_rest, ct, valid, 5.0, 0.1, False, 64)
        low = to.track(TABLE, s_init, s_rest, ct, valid, 5.0, 0.1, False, 64, dtype=f32)
        a, b = offs[i], offs[i + 1]
        for name, got, k in (("root", root, 0), ("viz_locs", viz, 1)):
            noise = float(np.abs(low[k].astype(np.float64) - ref[k]).max())
            err = float(np.abs(got[a:b].astype(np.float64) - ref[k]).max())
            assert err <= 3.0 * noise, (i, name, err, noise)
        st = terrain.TerrainState(blocks[i], 100, 64)
        assert np.array_equal(st.region_map, ref[4].region_map) and np.array_equal(st.ticks, ref[4].ticks)
        assert np.array_equal(q_hist[a:b], s_rest[:, :54])
    with pytest.raises(ValueError, match="two-SBP"):
        _run(skel, seqs, offs, True)
    tt = terrain.TerrainTracker(skel, 3, "cuda", multi_sbp=True)
    with pytest.raises(ValueError, match="two-SBP"):
        tt.step({"s_rest": torch.zeros(3, 111, device="cuda"), "c_t": torch.zeros(3, 8, device="cuda")})


# ---- 9. one SBP step for both runners --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_rows():
    """Three sequences of 1, 64 and 65 rows — the edges of the 64-row FK tile — cut from the golden tracks, with the numpy oracle's word
    that they test something: on each, some row has an active foot, and nothing the flat-ground runner makes of them is non-finite."""
    import kin_oracle as ko
    cuts = (("track2", 5, 6), ("track0", 0, 64), ("track1", 0, 65))      # the standing track's feet are down on its first valid row
    seqs = []
    for tag, a, b in cuts:
        s_init, s_rest, ct, valid, _ = _case(tag, False)
        seqs.append((s_init, s_rest[a:b], ct[a:b], valid[a:b]))
    for s_init, s_rest, ct, valid in seqs:
        for nc in (20, 8):
            root, viz, tr = ko.track(TABLE, s_init, s_rest, ct[:, :nc], valid)
            assert (tr["flags"] == 1).any() and np.isfinite(root).all() and np.isfinite(viz).all()
    offs = np.concatenate([[0], np.cumsum([s[1].shape[0] for s in seqs])]).astype(np.int64)
    return seqs, offs


@pytest.mark.parametrize("nc", [20, 8])
@pytest.mark.parametrize("chunk", [None, 7])
def test_flat_ground_and_terrain_runners_agree_on_x_and_y_bit_for_bit(skel, edge_rows, chunk, nc):
    """kinematics.track and terrain.track_terrain(multi_sbp=False) run the same SBP step (csrc/tip_kin_track.h) and disagree about the
    height only — the flat-ground rule against the map — which neither x nor y reads: the x and y columns of root and of viz_locs are
    the same bits."""
    seqs, offs = edge_rows
    s0, s_rest, ct, valid = (np.stack([s[0] for s in seqs]), np.concatenate([s[1] for s in seqs]),
                             np.concatenate([s[2][:, :nc] for s in seqs]), np.concatenate([s[3] for s in seqs]))
    root_k, viz_k = _np(*kin.track(skel, s0, s_rest, ct, valid, offs, chunk=chunk))
    root_t, viz_t = _np(*terrain.track_terrain(skel, s0, s_rest, ct, valid, offs, multi_sbp=False, chunk=chunk)[:2])
    assert root_k.shape == (130, 3) and viz_k.shape == (130, 5, 3)
    assert np.array_equal(root_k[:, :2].view(np.uint32), root_t[:, :2].view(np.uint32))
    assert np.array_equal(viz_k[:, :, :2].view(np.uint32), viz_t[:, :, :2].view(np.uint32))
    assert not np.array_equal(root_k[:, 2], root_t[:, 2])              # (the two did run their own z rules)


def test_track_replay_routes_through_the_terrain(skel):
    """kinematics.track_replay(terrain=...) is track_terrain with multi_sbp off on the same rows; terrain=None is the flat-ground tracker."""
    from tip_amd.replay import ReplayResult
    seqs, offs = _ragged(2)
    res = [ReplayResult(s[1], s[2], s[3], None) for s in seqs]
    s0 = np.stack([s[0] for s in seqs])
    got = kin.track_replay(skel, res, s0, terrain=dict(map_bound=5.0, grid_size=0.1))
    (root, viz, _, _), _ = _run(skel, seqs, offs, False)
    for i, (qdq, v) in enumerate(got):
        a, b = offs[i], offs[i + 1]
        assert np.array_equal(qdq[:, :3], root[a:b]) and np.array_equal(v, viz[a:b]) and np.array_equal(qdq[:, 3:], seqs[i][1])
    flat = kin.track_replay(skel, res, s0)
    assert not np.array_equal(flat[0][0][:, 2], got[0][0][:, 2])          # the flat-ground rule and the map disagree about the height
    with pytest.raises(ValueError, match="terrain is dict"):
        kin.track_replay(skel, res, s0, terrain=dict(map_bound=5.0))
