"""Per-wearer body scale on the device (the SCALED = true kernels of csrc/tip_kin.hip and csrc/tip_terrain.hip behind the *_scaled
entries) against tests/scale_oracle.py and the reference-generated golden (tests/golden/tip_scale_golden.npz: the real RTRunner.step
on characters scaled by 0.875 and 1.0625).  The skeleton comes from the golden's (unscaled) table only.  Discrete state must be EQUAL;
continuous values may differ from the fp64 oracle by at most 3 x the error of the same oracle run in numpy float32 on the same inputs
(tests/test_kin_gpu.py's rule), per kind of output; both figures are printed.  The scales the oracles get are the float32 values the
device gets."""
import ctypes

import numpy as np
import pytest
import torch

import kin_oracle as ko
import scale_oracle as so
import tip_amd
from tip_amd import kinematics as kin
from tip_amd import lib as tlib
from tip_amd import replay, synth, terrain
from test_host_cpu import make_model, load_synth
from test_kin_gpu import _metric_case, _pose_err
from test_replay_terrain_gpu import _recordings, _shifted_model
from test_terrain_cpu import golden_track

pytestmark = pytest.mark.gpu
f32 = np.float32
GOLDEN = np.load(__file__.replace("test_scale_gpu.py", "golden/tip_scale_golden.npz"))
TABLE = {k[len("table/"):]: GOLDEN[k] for k in GOLDEN.files if k.startswith("table/")}
FIXTURE = (("sA", 0.875, "track1"), ("sA", 0.875, "track2"), ("sB", 1.0625, "track0"), ("sB", 1.0625, "track2"))
SCALES3 = np.array([0.875, 1.0625, 1.3], dtype=f32)        # 1.3 is not a float32: the oracles get float32(1.3)
LENS3 = (1, 64, 65)                                        # one row; exactly one FK batch of the wave; one batch and one row
Engine = tip_amd.streaming.StaggeredStreamingEngine


@pytest.fixture(scope="module")
def skel():
    return kin.Skeleton.from_table(GOLDEN)


def _np(*tensors):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_bits(got, ref, who):
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (who, k)


def _rule(name, got, low, ref):
    noise, err = float(np.abs(low.astype(np.float64) - ref).max()), float(np.abs(got.astype(np.float64) - ref).max())
    print(f"    {name}: fp32 noise {noise:.3e} device error {err:.3e}")
    assert np.isfinite(got).all() and err <= 3.0 * noise, (name, err, noise)


# ---- 1. FK, one scale per row --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fk_case():
    rng = np.random.RandomState(23)
    q = np.concatenate([rng.randn(65, 3) * 2, rng.randn(65, 54) * 0.8, rng.randn(65, 3)], axis=1).astype(f32)      # ldq = 60
    sc = np.array([0.875, 1.0, 1.0625, 1.3], dtype=f32)[rng.randint(0, 4, 65)]
    sc[:4] = [1.3, 0.875, 1.0, 1.0625]
    ref = so.fk(TABLE, q.astype(np.float64), sc.astype(np.float64))
    low = so.fk(TABLE, q, sc.astype(np.float64), dtype=f32)
    return q, sc, ref, low


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_fk_with_a_scale_per_row(skel, fk_case, n):
    """One lane per pose, 64 per workgroup; the four scales mixed within one launch.  The rows at scale 1.0 are within the rule of the
    scaled kernel too, and a row at another scale is centimetres from the unscaled kernel's."""
    q, sc, ref, low = fk_case
    pq_g, pq_jf = kin.fk(skel, q[:n], out_jf=True, scale=sc[:n])
    assert pq_g.shape == pq_jf.shape == (n, 20, 7) and pq_g.dtype == torch.float32
    only_g = kin.fk(skel, torch.from_numpy(q[:n]).cuda(), scale=torch.from_numpy(sc[:n]).cuda())
    assert torch.equal(only_g, pq_g)                                    # from device tensors, without the link frames: the same bits
    if n == 1:
        assert torch.equal(kin.fk(skel, q[:1], scale=float(sc[0])), pq_g)      # one number for all rows
    plain = kin.fk(skel, q[:n]).cpu().numpy()
    for name, got, k in (("pq_g", pq_g, 0), ("pq_jf", pq_jf, 1)):
        got = got.cpu().numpy().astype(np.float64)
        noise_p, noise_q = _pose_err(low[k][:n].astype(np.float64), ref[k][:n])
        err_p, err_q = _pose_err(got, ref[k][:n])
        print(f"n={n} {name}: fp32 noise pos {noise_p:.3e} quat {noise_q:.3e}; device error pos {err_p:.3e} quat {err_q:.3e}")
        assert np.isfinite(got).all() and err_p <= 3.0 * noise_p and err_q <= 3.0 * noise_q
    assert np.abs(pq_g.cpu().numpy()[0, :, :3] - plain[0, :, :3]).max() > 0.05      # row 0 is at 1.3
    assert np.array_equal(pq_g.cpu().numpy()[:, :, 3:], plain[:, :, 3:])            # no rotation depends on the scale


# ---- 2. track and track_terrain on three sequences with three scales -------------------------------------------------------------------
def _kin_case(nc):
    """Sequences of 1, 64 and 65 rows generated like tip_kin_golden's track (c); the first two rows of the longer ones are not valid."""
    rows = [ko.scripted_rows(n, 90 + i, nc=nc, speed=1.0 if i % 2 else 0.5) for i, n in enumerate(LENS3)]
    s_rest = np.concatenate([r[0] for r in rows]).astype(f32)
    c_t = np.concatenate([r[1] for r in rows]).astype(f32)
    s_init = np.stack([r[2] for r in rows]).astype(f32)
    valid = np.concatenate([np.arange(n) >= min(2, n - 1) for n in LENS3])
    return s_init, s_rest, c_t, valid, np.concatenate([[0], np.cumsum(LENS3)]).astype(np.int64)


@pytest.mark.parametrize("nc", [20, 8])
def test_track_three_sequences_three_scales(skel, nc):
    s_init, s_rest, c_t, valid, offs = case = _kin_case(nc)
    sc64 = SCALES3.astype(np.float64)
    ref = so.track_ragged(TABLE, s_init.astype(np.float64), s_rest.astype(np.float64), c_t.astype(np.float64), valid, offs, sc64)
    low = so.track_ragged(TABLE, s_init, s_rest, c_t, valid, offs, sc64, dtype=f32)
    got = _np(*kin.track(skel, *case, scales=SCALES3))
    print(f"track nc={nc}:")
    _rule("root", got[0], low[0], ref[0])
    _rule("viz_locs", got[1], low[1], ref[1])
    plain = _np(*kin.track(skel, *case))
    assert np.abs(got[0] - plain[0]).max() > 1e-3                       # the scale reaches the root: not the unscaled track's
    _same_bits(_np(*kin.track(skel, *case, scales=SCALES3, chunk=7)), got, "chunk=7")
    for i in range(3):
        a, b = offs[i], offs[i + 1]
        one = _np(*kin.track(skel, s_init[i:i + 1], s_rest[a:b], c_t[a:b], valid[a:b], [0, b - a], scales=SCALES3[i:i + 1]))
        _same_bits(one, [g[a:b] for g in got], f"sequence {i} alone")


def _terrain_case():
    """Rows 5 .. 5 + n of three fixture tracks (their first valid rows), n = 1, 64, 65, at 0.875, 1.0625 and 1.3 — the first two the
    scales the reference ran them at, the third a scale it did not (the standing track, whose IK fires early, gets the long ones)."""
    seqs = []
    for (stag, _, tag), n in zip((FIXTURE[0], FIXTURE[3], FIXTURE[1]), LENS3):
        s_init, s_rest, ct, valid, _ = golden_track(GOLDEN, f"{stag}/{tag}", True)
        seqs.append((s_init.astype(f32), s_rest[5:5 + n].astype(f32), ct[5:5 + n].astype(f32), valid[5:5 + n]))
    offs = np.concatenate([[0], np.cumsum(LENS3)]).astype(np.int64)
    return (np.stack([s[0] for s in seqs]), np.concatenate([s[1] for s in seqs]), np.concatenate([s[2] for s in seqs]),
            np.concatenate([s[3] for s in seqs]), offs)


def _run_terrain(skel, case, multi, scales, **kw):
    out = terrain.track_terrain(skel, *case, multi_sbp=multi, scales=scales, **kw)
    return _np(*out[:4]), out[4].bytes


@pytest.mark.parametrize("multi", [False, True])
def test_track_terrain_three_sequences_three_scales(skel, multi):
    case = _terrain_case()
    s_init, s_rest, c_t, valid, offs = case
    sc64 = SCALES3.astype(np.float64)
    kw = dict(multi_sbp=multi)
    ref = so.track_terrain_ragged(TABLE, s_init.astype(np.float64), s_rest.astype(np.float64), c_t.astype(np.float64), valid, offs, sc64, **kw)
    low = so.track_terrain_ragged(TABLE, s_init, s_rest, c_t, valid, offs, sc64, dtype=f32, **kw)
    got, blocks = _run_terrain(skel, case, multi, SCALES3)
    print(f"track_terrain multi={int(multi)}: fired rows {(got[3] >= 0).sum()}")
    assert np.array_equal(got[3], ref[3])                               # fire, with the sequence's index
    for k, name in enumerate(("root", "viz_locs", "q_hist")):
        _rule(name, got[k], low[k], ref[k])
    for i, ost in enumerate(ref[4]):
        st = terrain.TerrainState(blocks[i], 100, 64)
        assert np.array_equal(st.region_map, ost.region_map) and np.array_equal(st.ticks, ost.ticks) and st.n_regions == len(ost.region_height)
    if multi:
        assert (got[3] >= 0).sum() >= 3                                 # the IK fired inside these rows
    got7, blocks7 = _run_terrain(skel, case, multi, SCALES3, chunk=7)
    _same_bits(got7, got, "chunk=7")
    assert np.array_equal(blocks7, blocks)
    for i in range(3):
        a, b = offs[i], offs[i + 1]
        one, b1 = _run_terrain(skel, (s_init[i:i + 1], s_rest[a:b], c_t[a:b], valid[a:b], [0, b - a]), multi, SCALES3[i:i + 1])
        _same_bits(one[:3], [g[a:b] for g in got[:3]], f"sequence {i} alone")
        assert np.array_equal(one[3] >= 0, got[3][a:b] >= 0) and np.array_equal(b1[0], blocks[i]), i


# ---- 3. the fixture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multi", [False, True])
def test_the_scaled_golden_tracks(skel, multi):
    """The four fixture tracks in ONE launch, two at 0.875 and two at 1.0625: region map, ticks, region count, region weights and fire
    equal to the real RTRunner.step's on the scaled character; root, viz_locs, q_hist, region heights and IK deltas within the rule."""
    cases = [golden_track(GOLDEN, f"{stag}/{tag}", multi) for stag, _, tag in FIXTURE]
    scales = np.array([s for _, s, _ in FIXTURE], dtype=f32)
    offs = np.concatenate([[0], np.cumsum([c[1].shape[0] for c in cases])]).astype(np.int64)
    ins = (np.stack([c[0] for c in cases]).astype(f32), np.concatenate([c[1] for c in cases]).astype(f32),
           np.concatenate([c[2] for c in cases]).astype(f32), np.concatenate([c[3] for c in cases]), offs)
    (root, viz, q_hist, fire), blocks = _run_terrain(skel, ins, multi, scales)
    for i, ((stag, scale, tag), (s_init, s_rest, ct, valid, exp)) in enumerate(zip(FIXTURE, cases)):
        a, b = offs[i], offs[i + 1]
        lo = so.track_terrain(TABLE, s_init.astype(f32), s_rest.astype(f32), ct.astype(f32), valid, scale, 5.0, 0.1, multi, 64, dtype=f32)
        st = terrain.TerrainState(blocks[i], 100, 64)
        print(f"{stag} {tag} multi={int(multi)}:")
        assert np.array_equal(fire[a:b] >= 0, exp["fire"]) and (fire[a:b][exp["fire"]] == i).all()
        assert np.array_equal(st.region_map, exp["region_map"]) and st.n_regions == len(exp["region_height"])
        assert np.array_equal(st.ticks, exp["ticks"][-1]) and st.off_map == 0 and st.regions_full == 0
        assert np.array_equal(st.region_weight, exp["region_weight"])
        rows = exp["fire_rows"]
        _rule("root", root[a:b], lo[0], exp["root"])
        _rule("viz_locs", viz[a:b], lo[1], exp["viz_locs"])
        if len(rows):
            _rule("q_hist", q_hist[a:b][rows], lo[2][rows], exp["q_hist"][rows])
        _rule("region_height", np.asarray(st.region_height), np.asarray(lo[4].region_height), exp["region_height"])
        _rule("ik_deltas", np.asarray(st.ik_deltas), np.asarray(lo[4].ik_deltas), exp["ik_deltas"])
        assert (viz[a:b][~valid] == 100).all() and (root[a:b][~valid] == s_init[:3].astype(f32)).all()
        assert np.array_equal(q_hist[a:b][~exp["fire"]], s_rest[~exp["fire"], :54].astype(f32))


# ---- 4. the live trackers ------------------------------------------------------------------------------------------------------------
def _live(tr, s_init, rows, scales, n_rows, reset_at=None):
    """`tr` (3 slots) reset with `scales` and stepped row by row on rows = (s_rest, c_t, valid) [n_rows, 3, ...]; reset_at = (t, slot,
    s_init_row, scale): that slot starts over in front of row t.  Returns its output tensors per row, [n_rows, 3, ...]."""
    tr.reset(None, s_init, scales=scales)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in rows]
    got = []
    for t in range(n_rows):
        if reset_at is not None and t == reset_at[0]:
            tr.reset([reset_at[1]], reset_at[2][None], scales=[reset_at[3]])
        tr.step({"s_rest": dev[0][t], "c_t": dev[1][t], "valid": dev[2][t]})
        got.append([x.clone() for x in tr._outs])
    return _np(*[torch.stack([g[k] for g in got]) for k in range(len(tr._outs))])


@pytest.mark.parametrize("which", ["root", "terrain"])
def test_live_trackers_of_three_wearers(skel, which):
    """Three slots, three scales, 60 frames, one launch per frame: the bits of the post-pass over the same rows.  Then the same run with
    slot 1 reset in front of frame 25 to another wearer (scale 1.2): slots 0 and 2 keep every bit, and slot 1 from there on has the
    bits of a post-pass over the rest of its rows at the new scale."""
    n = 60
    cases = [golden_track(GOLDEN, f"{stag}/{tag}", True) for stag, _, tag in (FIXTURE[1], FIXTURE[2], FIXTURE[0])]
    s_init = np.stack([c[0] for c in cases]).astype(f32)
    rows = tuple(np.stack([c[k][:n] for c in cases], axis=1).astype(d) for k, d in ((1, f32), (2, f32), (3, bool)))
    flat = (s_init, *(np.concatenate([r[:, i] for i in range(3)]) for r in rows), np.array([0, n, 2 * n, 3 * n]))
    if which == "root":
        make = lambda: kin.RootTracker(skel, 3, "cuda")
        post = _np(*kin.track(skel, *flat, scales=SCALES3))
        tail = _np(*kin.track(skel, s_init[2:3], rows[0][25:, 1], rows[1][25:, 1], rows[2][25:, 1], [0, n - 25], scales=[1.2]))
    else:
        make = lambda: terrain.TerrainTracker(skel, 3, "cuda", multi_sbp=True)
        post, post_bytes = _run_terrain(skel, flat, True, SCALES3)
        tail, _ = _run_terrain(skel, (s_init[2:3], rows[0][25:, 1], rows[1][25:, 1], rows[2][25:, 1], [0, n - 25]), True, [1.2])
    tr = make()
    assert tr.entries[1] in ("tip_kin_track", "tip_terrain_track") and (tr.scale == 1).all()      # until a reset gives scales
    live = _live(tr, s_init, rows, SCALES3, n)
    assert tr.entries[1].endswith("_scaled") and np.array_equal(tr.scale.cpu().numpy(), SCALES3)
    for k, (a, b) in enumerate(zip(live, post)):
        for i in range(3):
            x, y = a[:, i], b[i * n:(i + 1) * n]
            if k == 3:                                                  # fire: the slot's index, live and post-pass alike
                assert np.array_equal(x, y), (k, i)
            else:
                assert np.array_equal(_bits(x), _bits(y)), (k, i)
    if which == "terrain":
        assert np.array_equal(tr.state_bytes(), post_bytes) and (live[3] >= 0).sum() >= 3
    tr2 = make()
    again = _live(tr2, s_init, rows, SCALES3, n, reset_at=(25, 1, s_init[2], 1.2))
    assert np.array_equal(tr2.scale.cpu().numpy(), np.array([0.875, 1.2, 1.3], dtype=f32))
    for k, (a, b) in enumerate(zip(again, live)):
        assert np.array_equal(_bits(a[:, 0]), _bits(b[:, 0])) and np.array_equal(_bits(a[:, 2]), _bits(b[:, 2])), k
        assert np.array_equal(_bits(a[:25, 1]), _bits(b[:25, 1])), k
        if k < 3:
            assert np.array_equal(_bits(a[25:, 1]), _bits(tail[k])), k
    assert not np.array_equal(again[0][25:, 1], live[0][25:, 1])
    if which == "terrain":
        sb = tr2.state_bytes()
        assert np.array_equal(sb[0], post_bytes[0]) and np.array_equal(sb[2], post_bytes[2]) and not np.array_equal(sb[1], post_bytes[1])


# ---- 5. a scale the kernels refuse, through the C-ABI ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), -1.0])
def test_a_refused_scale_stays_in_its_sequence(skel, bad):
    """The host refuses such a scale; a caller of the C-ABI can still pass one.  The entries return TIP_OK; the sequence's rows are NaN
    with fire -1 and its map is as the reset left it; the other sequences keep every bit."""
    lib = tlib.load()
    case = _terrain_case()
    s_init, s_rest, c_t, valid, offs = case
    good, good_bytes = _run_terrain(skel, case, True, SCALES3)
    good_k = _np(*kin.track(skel, *case, scales=SCALES3))
    sc = torch.tensor([SCALES3[0], bad, SCALES3[2]], dtype=torch.float32, device="cuda")
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (s_init, s_rest, c_t, valid.astype(np.uint8))]
    od = torch.from_numpy(offs).cuda()
    n = int(offs[-1])
    stream = torch.cuda.current_stream().cuda_stream
    # terrain
    st = terrain._State(skel, 3, "cuda", 5.0, 0.1, True, 64, "test")
    outs = (torch.zeros(n, 3), torch.zeros(n, 5, 3), torch.zeros(n, 54), torch.zeros(n, dtype=torch.int32))
    outs = [o.cuda() for o in outs]
    assert lib.tip_terrain_reset_scaled(st.sk.data_ptr(), st.buf.data_ptr(), 3, st.G, st.M, None, 3, dev[0].data_ptr(), sc.data_ptr(), stream) == 0
    fresh = st.view(1)
    assert lib.tip_terrain_track_scaled(st.sk.data_ptr(), st.buf.data_ptr(), 3, st.G, st.M, st.D, st.grid_size, None, od.data_ptr(),
                                        od.data_ptr() + 8, 3, n, dev[1].data_ptr(), dev[2].data_ptr(), 20, dev[3].data_ptr(), 1,
                                        *(o.data_ptr() for o in outs), sc.data_ptr(), stream) == 0
    root, viz, q_hist, fire = _np(*outs)
    a, b = offs[1], offs[2]
    assert np.isnan(root[a:b]).all() and np.isnan(viz[a:b]).all() and np.isnan(q_hist[a:b]).all() and (fire[a:b] == -1).all()
    after = st.view(1)
    assert np.array_equal(after.region_map, fresh.region_map) and np.array_equal(after.d2_map, fresh.d2_map) and (after.d2_map == 10000).all()
    assert np.array_equal(after.bytes, fresh.bytes)                     # nothing of the block was written
    blocks = st.buf[:3 * st.stride].cpu().numpy().reshape(3, st.stride)
    for i in (0, 2):
        s = slice(offs[i], offs[i + 1])
        _same_bits([root[s], viz[s], q_hist[s], fire[s]], [g[s] for g in good], f"terrain sequence {i}")
        assert np.array_equal(blocks[i], good_bytes[i]), i
    # the flat-ground tracker
    cr = kin._Carry(skel, 3, "cuda")
    ko_, kv = torch.zeros(n, 3).cuda(), torch.zeros(n, 5, 3).cuda()
    assert lib.tip_kin_track_reset_scaled(cr.sk.data_ptr(), cr.buf.data_ptr(), 3, None, 3, dev[0].data_ptr(), sc.data_ptr(), stream) == 0
    assert lib.tip_kin_track_scaled(cr.sk.data_ptr(), cr.buf.data_ptr(), 3, None, od.data_ptr(), od.data_ptr() + 8, 3, n, dev[1].data_ptr(),
                                    dev[2].data_ptr(), 20, dev[3].data_ptr(), ko_.data_ptr(), kv.data_ptr(), sc.data_ptr(), stream) == 0
    kr, kvz = _np(ko_, kv)
    assert np.isnan(kr[a:b]).all() and np.isnan(kvz[a:b]).all()
    for i in (0, 2):
        s = slice(offs[i], offs[i + 1])
        _same_bits([kr[s], kvz[s]], [g[s] for g in good_k], f"track sequence {i}")
    # FK: the row is NaN whole, its neighbours keep their bits
    q = torch.from_numpy(np.concatenate([np.zeros((3, 3), f32), s_rest[[0, 1, 2], :54]], axis=1)).cuda()
    pq, ref = torch.zeros(3, 20, 7).cuda(), kin.fk(skel, q, scale=sc.cpu().numpy()[[0, 0, 2]])
    assert lib.tip_kin_fk_scaled(skel.on("cuda").data_ptr(), q.data_ptr(), 57, 3, pq.data_ptr(), None, sc.data_ptr(), stream) == 0
    pq, ref = _np(pq, ref)
    assert np.isnan(pq[1]).all() and np.array_equal(_bits(pq[[0, 2]]), _bits(ref[[0, 2]]))


# ---- 6. the metrics of files made at a scale ---------------------------------------------------------------------------------------------
def test_evaluate_with_scales(skel):
    pred, gt, offs = _metric_case([40, 40])
    scales = np.array([0.875, 1.3], dtype=f32)
    ref = so.evaluate(TABLE, pred.astype(np.float64), gt.astype(np.float64), offs, scales.astype(np.float64), start=8, end=2)
    low = so.evaluate(TABLE, pred.astype(np.float64), gt.astype(np.float64), offs, scales.astype(np.float64), start=8, end=2, dtype=f32)
    got = kin.evaluate(skel, pred, gt, offs, start=8, end=2, scales=scales)
    plain = kin.evaluate(skel, pred, gt, offs, start=8, end=2)
    noise, err = np.abs(low - ref).max(0), np.abs(got - ref).max(0)
    for k, name in enumerate(kin.METRICS):
        print(f"evaluate {name}: fp32 noise {noise[k]:.3e}; device error {err[k]:.3e}; scaled - unscaled {np.abs(got - plain)[:, k].max():.3e}")
    assert got.dtype == np.float64 and got.shape == (2, 7) and np.isfinite(got).all() and (err <= 3.0 * noise).all()
    j = kin.METRICS.index("j_pos")
    assert (np.abs(got[:, j] - plain[:, j]) > 3.0 * noise[j]).all()     # the unscaled table measures another body
    assert np.allclose(got[:, j] / plain[:, j], scales, rtol=1e-3)      # root-relative COM distances are linear in the scale


# ---- 7. the replay pool: one slot changes wearer -------------------------------------------------------------------------------------
def _alone(m, skel, rec, s0, scale):
    """One recording through a one-slot engine stepped from the host with TerrainTracker.reset(scales=) + step + feed_back, laid out by
    the script's row conventions (tests/test_replay_terrain_gpu.py's _alone, with the scale)."""
    eng = Engine(m, s0[None])
    tt = terrain.TerrainTracker(skel, 1, "cuda", 5.0, 0.1, multi_sbp=True)
    tt.reset(None, s0[None], scales=[scale])
    L = rec.shape[0]
    dev = dict(s_rest=torch.zeros(L, 111), c_t=torch.zeros(L, eng.nc), valid=torch.zeros(L, dtype=torch.bool), root=torch.zeros(L, 3),
               viz_locs=torch.full((L, 5, 3), 100.0), q_hist=torch.zeros(L, 54), fire=torch.zeros(L, dtype=torch.bool))
    dev = {k: v.cuda() for k, v in dev.items()}
    dev["s_rest"][:], dev["root"][:], dev["q_hist"][:] = (torch.tensor(s0[a:b]).cuda() for a, b in ((3, 114), (0, 3), (3, 57)))
    frames = torch.tensor(rec).cuda()
    for t in range(L - 1):
        out = eng.step(frames[t][None])
        tt.step(out)
        tt.feed_back(eng)
        ok = out["valid"][0]
        dev["valid"][t + 1] = ok
        for k, src in (("s_rest", out["s_rest"]), ("c_t", out["c_t"]), ("root", tt.root), ("viz_locs", tt.viz_locs), ("q_hist", tt.q_hist)):
            dev[k][t + 1] = torch.where(ok, src[0], dev[k][0])
        dev["fire"][t + 1] = ok & (tt.fire[0] >= 0)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dev.items()}


@pytest.fixture(scope="module", params=["load_synth", "shifted"])
def pool_case(skel, request):
    """load_synth: the synthetic weights as they are, on synth.make_recording's recordings.  shifted: tests/test_replay_terrain_gpu.py's
    model (contact logits of the feet and the root raised) on its upright recordings, where the contacts hold and the IK fires, so that
    the scale is seen to reach the root and the fed-back pose."""
    if request.param == "load_synth":
        m = make_model(synth.PAPER)
        load_synth(m, synth.PAPER, 0)
        m = m.cuda().eval()
        recs, s0 = zip(*(synth.make_recording(L, seed=400 + i) for i, L in enumerate((50, 64, 90))))
        recs, s0 = list(recs), np.stack(s0).astype(f32)
    else:
        m = _shifted_model().eval()
        recs, s0 = _recordings((50, 64, 90), seed0=720)
        s0 = s0.astype(f32)
    m.set_plan("fused")
    try:
        alone = [_alone(m, skel, r, s0[i], float(SCALES3[i])) for i, r in enumerate(recs)]
    finally:
        m.set_plan("auto")
    return m, recs, s0, alone, request.param == "shifted"


@pytest.mark.parametrize("use_graph", [False, True])
def test_pool_of_two_slots_three_wearers(skel, pool_case, use_graph):
    """Recordings of 50, 64 and 90 frames at 0.875, 1.0625 and 1.3 on two slots: slot 0 takes the third wearer when the first is done.
    Every recording has the bits it has alone; a run without scales afterwards is back on the unscaled entries."""
    m, recs, s0, alone, shifted = pool_case
    m.set_plan("fused")
    try:
        pool = replay.ReplayPool(m, slots=2, use_graph=use_graph, terrain=dict(skel=skel, map_bound=5.0, grid_size=0.1, multi_sbp=True))
        assert pool.tracker.entries == ("tip_terrain_reset", "tip_terrain_track")
        out = pool.run(recs, s0, scales=SCALES3)
        assert pool.plan.slot == [0, 1, 0] and pool.restarts == 0
        assert pool.tracker.entries == ("tip_terrain_reset_scaled", "tip_terrain_track_scaled")
        for i, (r, a) in enumerate(zip(out, alone)):
            for k in ("s_rest", "c_t", "valid", "root", "viz_locs", "q_hist", "fire"):
                x, y = getattr(r, k), a[k]
                assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (i, k)
        plain = pool.run(recs, s0)
        assert pool.tracker.entries == ("tip_terrain_reset", "tip_terrain_track") and (pool.tracker.scale == 1).all()
        moved = [float(np.abs(p.root - r.root).max()) for p, r in zip(plain, out)]
        print("fired rows", [int(r.fire.sum()) for r in out], "root moved by the scale", moved)
        if shifted:                                                     # contacts hold there: the scale reached every recording's root
            assert min(moved) > 1e-4 and sum(int(r.fire.sum()) for r in out) >= 3
    finally:
        m.set_plan("auto")
    with pytest.raises(ValueError, match="this pool has none"):
        replay.ReplayPool(m, slots=2, use_graph=False).run(recs, s0, scales=SCALES3)
