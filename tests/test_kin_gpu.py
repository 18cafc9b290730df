"""tip_amd.kinematics on the device (csrc/tip_kin.hip) against tests/kin_oracle.py and the reference-generated golden
(tests/golden/tip_kin_golden.npz).  The skeleton comes from the golden's table only.  The bound everywhere: the device may differ
from the fp64 oracle by at most 3 x the error of the same restatement in numpy float32 on the same inputs (test_sensor_gpu._noise's
rule), measured here, per kind of output."""
import numpy as np
import pytest
import torch

import kin_oracle as ko
from tip_amd import kinematics as kin
from tip_amd import replay, synth
from test_host_cpu import make_model, load_synth

pytestmark = pytest.mark.gpu
f32 = np.float32
GOLDEN = np.load(__file__.replace("test_kin_gpu.py", "golden/tip_kin_golden.npz"))
TABLE = {k[len("table/"):]: GOLDEN[k] for k in GOLDEN.files if k.startswith("table/")}
LENGTHS = (70, 48, 8, 7)          # 7: row 0, five priming rows and exactly one valid row
PRIMING = 6


@pytest.fixture(scope="module")
def skel():
    return kin.Skeleton.from_table(GOLDEN)


def _qdist(a, b):
    """|a - b| of quaternions up to sign, [..., 4] -> [...]."""
    return np.minimum(np.abs(a - b).max(-1), np.abs(a + b).max(-1))


def _pose_err(got, ref):
    return float(np.abs(got[..., :3] - ref[..., :3]).max()), float(_qdist(got[..., 3:], ref[..., 3:]).max())


# ---- 1. FK ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fk_case():
    """The golden's 32 poses (the zero pose first), then random ones, as the float32 the device gets; the fp64 oracle and the float32
    restatement on those."""
    rng = np.random.RandomState(11)
    q = np.concatenate([GOLDEN["poses/q"], np.concatenate([rng.randn(225, 3) * 2, rng.randn(225, 54) * 0.8], axis=1)]).astype(f32)
    q = np.concatenate([q, rng.randn(257, 3).astype(f32)], axis=1)          # ldq = 60: wider rows than the 57 that are read
    ref = ko.fk(TABLE, q.astype(np.float64))
    low = ko.fk(TABLE, q, dtype=f32)
    return q, ref, low


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_fk_matches_the_oracle(skel, fk_case, n):
    """One lane per pose, 64 per workgroup: 63 / 64 / 65 sit around the first workgroup's edge, 257 is five workgroups with one row in
    the last.  N = 1 is the zero pose alone."""
    q, ref, low = fk_case
    pq_g, pq_jf = kin.fk(skel, q[:n], out_jf=True)
    assert pq_g.shape == pq_jf.shape == (n, 20, 7) and pq_g.dtype == torch.float32
    only_g = kin.fk(skel, torch.from_numpy(q[:n]).cuda())
    assert torch.equal(only_g, pq_g)                                    # without the link frames, from a device tensor: the same bits
    for name, got, k in (("pq_g", pq_g, 0), ("pq_jf", pq_jf, 1)):
        got = got.cpu().numpy().astype(np.float64)
        noise_p, noise_q = _pose_err(low[k][:n].astype(np.float64), ref[k][:n])
        err_p, err_q = _pose_err(got, ref[k][:n])
        print(f"n={n} {name}: fp32 noise pos {noise_p:.3e} quat {noise_q:.3e}; device error pos {err_p:.3e} quat {err_q:.3e}")
        assert np.isfinite(got).all()
        assert err_p <= 3.0 * noise_p and err_q <= 3.0 * noise_q
        # the zero pose is exact: every product is by 0 or 1, A2Q(0) = (0, 0, 0, 1), and the position sums run in the oracle's order
        assert np.array_equal(got[0, :, 3:], np.tile([0.0, 0, 0, 1], (20, 1))) and np.array_equal(got[0], low[k][0].astype(np.float64))


def test_fk_a2q_below_1e_4_rad(skel):
    """A2Q's series branch: joint angles of 0, 1e-8, 1e-5, 1e-4 and around the switch at 1e-3, one link at a time."""
    angles = np.array([0.0, 1e-8, 1e-5, 1e-4, 0.999e-3, 1.001e-3])
    q = np.zeros((len(angles) * 3, 57), dtype=f32)
    for i, a in enumerate(angles):
        for ax in range(3):
            q[3 * i + ax, 6 + ax] = a                                   # lhip
    got = kin.fk(skel, q).cpu().numpy().astype(np.float64)
    ref = ko.fk(TABLE, q.astype(np.float64))[0]
    low = ko.fk(TABLE, q, dtype=f32)[0].astype(np.float64)
    noise_p, noise_q = _pose_err(low, ref)
    err_p, err_q = _pose_err(got, ref)
    print(f"small angles: fp32 noise pos {noise_p:.3e} quat {noise_q:.3e}; device error pos {err_p:.3e} quat {err_q:.3e}")
    # So close to the zero pose the float32 restatement is off by an ulp or two at most, too little to scale a bound from; the
    # bounds here are fp32's own.  Positions: sums of at most five offsets under 0.5 m and their rotations by almost nothing, each step
    # rounded at 2^-24 relative: under 1e-6.  Quaternions: x = angle / 2 to three roundings (the input's, the scale, the product).
    assert err_p <= 1e-6 and err_q <= 2.0 ** -23
    x = got[np.arange(len(q)), 1, 3 + np.arange(len(q)) % 3].reshape(len(angles), 3)
    assert np.allclose(x[1:], angles[1:, None] / 2, rtol=3 * 2.0 ** -24, atol=0) and (x[0] == 0).all()


# ---- 2. the tracker ------------------------------------------------------------------------------------------------------------------
def _sound(tr, valid):
    """The three properties of golden (c) on the oracle's trace, pooled over a case's sequences."""
    fl = tr["flags"][valid]
    combos = [int(((fl[:, 0] == a) & (fl[:, 1] == b)).sum()) for a in (0, 1) for b in (0, 1)]
    on = valid & (tr["flags"].max(1) == 1)
    clip, margin = tr["clip"], float(tr["margin"].min())
    assert min(combos) >= 5, combos
    assert int((clip & on).sum()) >= 5 and int((~clip & on).sum()) >= 20, (int((clip & on).sum()), int((~clip & on).sum()))
    assert margin > 0.1, margin


@pytest.mark.parametrize("tag", ["track0", "track1"])
def test_tracker_matches_the_golden_tracks(skel, tag):
    """Teacher-forced: the golden's qdq[3:114] and ct in, its qdq[:3] and viz_locs (the real RTRunnerMin.step) out."""
    qdq, ct, valid = GOLDEN[tag + "/qdq"], GOLDEN[tag + "/ct"], GOLDEN[tag + "/valid"]
    s_init = GOLDEN[tag + "/s_init"]
    n = qdq.shape[0]
    root, viz = kin.track(skel, s_init[None], qdq[:, 3:], ct, valid, [0, n])
    root, viz = root.cpu().numpy().astype(np.float64), viz.cpu().numpy().astype(np.float64)
    lr, lv, _ = ko.track(TABLE, s_init, qdq[:, 3:], ct, valid, dtype=f32)
    noise_r, noise_v = float(np.abs(lr - qdq[:, :3]).max()), float(np.abs(lv - GOLDEN[tag + "/viz_locs"]).max())
    err_r, err_v = float(np.abs(root - qdq[:, :3]).max()), float(np.abs(viz - GOLDEN[tag + "/viz_locs"]).max())
    print(f"{tag}: fp32 noise root {noise_r:.3e} viz_locs {noise_v:.3e}; device error root {err_r:.3e} viz_locs {err_v:.3e}")
    assert err_r <= 3.0 * noise_r and err_v <= 3.0 * noise_v
    assert (viz[~valid] == 100).all() and (root[~valid] == s_init[:3].astype(f32)).all()


def _ragged(R, nc, seed0=40):
    """R sequences of LENGTHS in turn, generated like golden (c), as the float32 the device gets."""
    lens = [LENGTHS[i % len(LENGTHS)] for i in range(R)]
    rows = [ko.scripted_rows(n, seed0 + i, nc=nc, speed=1.0 if i % 2 else 0.5) for i, n in enumerate(lens)]
    s_rest = np.concatenate([r[0] for r in rows]).astype(f32)
    c_t = np.concatenate([r[1] for r in rows]).astype(f32)
    s_init = np.stack([r[2] for r in rows]).astype(f32)
    valid = np.concatenate([np.arange(n) >= PRIMING for n in lens])
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return s_init, s_rest, c_t, valid, offs


def _oracle_ragged(case, dtype):
    s_init, s_rest, c_t, valid, offs = case
    r, v, tr = ko.track_ragged(TABLE, s_init.astype(np.float64), s_rest.astype(np.float64), c_t.astype(np.float64), valid, offs, dtype=dtype)
    return r.astype(np.float64), v.astype(np.float64), tr


@pytest.fixture(scope="module")
def three():
    """R = 3, c_t width 20: the case the carry and isolation tests share, with its one-call device result."""
    case = _ragged(3, 20)
    return case, _oracle_ragged(case, np.float64)


@pytest.mark.parametrize("R,nc", [(1, 20), (3, 20), (3, 8), (65, 20), (65, 8)])
def test_tracker_matches_the_oracle_on_ragged_sequences(skel, R, nc):
    case = _ragged(R, nc)
    s_init, s_rest, c_t, valid, offs = case
    ref_r, ref_v, traces = _oracle_ragged(case, np.float64)
    low_r, low_v, _ = _oracle_ragged(case, f32)
    _sound(traces, valid)
    root, viz = kin.track(skel, s_init, s_rest, c_t, valid, offs)
    root, viz = root.cpu().numpy().astype(np.float64), viz.cpu().numpy().astype(np.float64)
    noise_r, noise_v = float(np.abs(low_r - ref_r).max()), float(np.abs(low_v - ref_v).max())
    err_r, err_v = float(np.abs(root - ref_r).max()), float(np.abs(viz - ref_v).max())
    print(f"R={R} nc={nc}: fp32 noise root {noise_r:.3e} viz_locs {noise_v:.3e}; device error root {err_r:.3e} viz_locs {err_v:.3e}")
    assert np.isfinite(root).all() and np.isfinite(viz).all()
    assert err_r <= 3.0 * noise_r and err_v <= 3.0 * noise_v
    if nc == 8:                                                            # two SBPs: rows 2-4 stay at 100 (less vel_res DT, like every row)
        assert (viz[:, 2] == viz[:, 3]).all() and (viz[:, 3] == viz[:, 4]).all() and np.abs(viz[:, 2:] - 100).max() < 0.1
    if R == 65:                                                            # length 7: exactly one valid row, the last
        assert offs[4] - offs[3] == 7 and valid[offs[3]:offs[4]].sum() == 1 and valid[offs[4] - 1]


def test_carry_gives_the_same_bits_in_any_chunking(skel, three):
    """One call, chunks of 7, and chunks of 1 through RootTracker.step (the live form): bit-identical root and viz_locs."""
    (s_init, s_rest, c_t, valid, offs), _ = three
    whole = kin.track(skel, s_init, s_rest, c_t, valid, offs)
    sevens = kin.track(skel, s_init, s_rest, c_t, valid, offs, chunk=7)
    assert torch.equal(whole[0], sevens[0]) and torch.equal(whole[1], sevens[1])
    R, lens = 3, np.diff(offs)
    rt = kin.RootTracker(skel, R, "cuda")
    rt.reset(None, s_init)
    assert rt.step(None)[0] is rt.root
    s_d, c_d = torch.from_numpy(s_rest).cuda(), torch.from_numpy(c_t).cuda()
    firsts = torch.from_numpy(offs[:3] + PRIMING).cuda()
    live_r, live_v = torch.zeros_like(whole[0]), torch.zeros_like(whole[1])
    for t in range(int(lens.max())):
        idx = torch.tensor([int(min(offs[i] + t, offs[i + 1] - 1)) for i in range(R)], device="cuda")
        ok = torch.tensor([bool(t < lens[i] and valid[offs[i] + t]) for i in range(R)], device="cuda")
        root, viz = rt.step({"s_rest": s_d[idx].contiguous(), "c_t": c_d[idx].contiguous(), "valid": ok})
        for i in range(R):
            if t < lens[i]:
                live_r[offs[i] + t], live_v[offs[i] + t] = root[i], viz[i]
    assert torch.equal(whole[0], live_r) and torch.equal(whole[1], live_v)
    # slots=[...] steps the listed blocks only: the others keep their carry
    rt.reset([1], s_init[1])
    before = rt.root.clone()
    rt.step({"s_rest": s_d[firsts].contiguous(), "c_t": c_d[firsts].contiguous()}, slots=[1])
    assert torch.equal(rt.root[[0, 2]], before[[0, 2]]) and torch.equal(rt.root[1], whole[0][offs[1] + PRIMING])


def test_a_nan_row_stays_in_its_sequence(skel, three):
    (s_init, s_rest, c_t, valid, offs), _ = three
    clean = kin.track(skel, s_init, s_rest, c_t, valid, offs)
    bad = s_rest.copy()
    row = offs[1] + 20
    bad[row] = np.nan
    root, viz = kin.track(skel, s_init, bad, c_t, valid, offs)
    for i in (0, 2):
        assert torch.equal(root[offs[i]:offs[i + 1]], clean[0][offs[i]:offs[i + 1]])
        assert torch.equal(viz[offs[i]:offs[i + 1]], clean[1][offs[i]:offs[i + 1]])
    assert torch.equal(root[offs[1]:row], clean[0][offs[1]:row]) and torch.equal(viz[offs[1]:row], clean[1][offs[1]:row])
    assert torch.isnan(root[row:offs[2]]).all() and torch.isfinite(clean[0]).all()


# ---- 3. the metrics ------------------------------------------------------------------------------------------------------------------
def _metric_case(lengths, seed0=70):
    pred, gt = [], []
    for i, n in enumerate(lengths):
        rng = np.random.RandomState(seed0 + i)
        s_rest, _, s_init = ko.scripted_rows(n, seed0 + i)
        t = np.arange(n)[:, None] / 60.0
        p = np.zeros((n, 114))
        p[:, 3:] = s_rest
        p[:, :3] = s_init[:3] + 0.3 * np.sin(2 * np.pi * rng.uniform(0.1, 0.5, 3) * t + rng.uniform(0, 6, 3)) + 0.002 * rng.randn(n, 3)
        g = p.copy()
        g[:, :57] += 0.05 * np.sin(2 * np.pi * rng.uniform(0.2, 1.0, 57) * t + rng.uniform(0, 6, 57))
        g[:, :3] += t * rng.uniform(-0.2, 0.2, 3)
        pred.append(p)
        gt.append(g)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return np.concatenate(pred).astype(f32), np.concatenate(gt).astype(f32), offs


def _oracle_metrics(pred, gt, offs, dtype, **kw):
    return np.stack([ko.evaluate(TABLE, pred[a:b].astype(np.float64), gt[a:b].astype(np.float64), dtype=dtype, **kw)
                     for a, b in zip(offs[:-1], offs[1:])])


def test_metrics_match_the_golden(skel):
    """Golden (d): the reference's own loss_* functions over the script's FK loop, both tracks in one call."""
    pred = np.concatenate([GOLDEN["track0/pred_qdq"], GOLDEN["track1/pred_qdq"]])
    gt = np.concatenate([GOLDEN["track0/gt_qdq"], GOLDEN["track1/gt_qdq"]])
    offs = np.array([0, 60, 150])
    ref = np.stack([GOLDEN["track0/metrics"], GOLDEN["track1/metrics"]])
    got = kin.evaluate(skel, pred, gt, offs)
    noise = np.abs(_oracle_metrics(pred, gt, offs, f32) - ref).max(0)
    err = np.abs(got - ref).max(0)
    for k, name in enumerate(kin.METRICS):
        print(f"golden {name}: fp32 noise {noise[k]:.3e}; device error {err[k]:.3e}")
    assert got.dtype == np.float64 and got.shape == (2, 7) and (err <= 3.0 * noise).all()


def test_metrics_match_the_oracle_at_the_clamps(skel):
    """L = 40: 4 rows in range and one jerk sample; 100: all three root rows clamped (64 in range); 200: 2 s unclamped, 5 s and 10 s
    clamped (164 in range).  One call, one workgroup per file."""
    pred, gt, offs = _metric_case([40, 100, 200])
    assert [ko.root_indices(n) for n in (4, 64, 164)] == [[3, 3, 3], [63, 63, 63], [119, 163, 163]]
    ref = _oracle_metrics(pred, gt, offs, np.float64)
    noise = np.abs(_oracle_metrics(pred, gt, offs, f32) - ref).max(0)
    got = kin.evaluate(skel, pred, gt, offs)
    err = np.abs(got - ref).max(0)
    for k, name in enumerate(kin.METRICS):
        print(f"oracle {name}: fp32 noise {noise[k]:.3e}; device error {err[k]:.3e}")
    assert np.isfinite(got).all() and (got > 0).all() and (err <= 3.0 * noise).all()
    assert ref[2, 2] != ref[2, 3] and ref[2, 3] == ref[2, 4] and ref[1, 2] == ref[1, 4]
    with pytest.raises(ValueError, match="must leave at least 4"):
        kin.evaluate(skel, pred[:39], gt[:39], [0, 39])
    with pytest.raises(ValueError, match="offsets is"):
        kin.evaluate(skel, pred, gt, [0, 40, 100])


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------
def test_replay_then_track_then_evaluate(skel):
    """ReplayPool -> track_replay -> evaluate on three short synthetic recordings equals the oracle fed the same device rows, and the
    replay itself is untouched by the post-pass: the same frames and the same bits before and after it."""
    cfg = synth.PAPER
    m = make_model(cfg)
    load_synth(m, cfg, 0)
    m = m.cuda().eval()
    recs, s0 = zip(*(synth.make_recording(L, seed=300 + i) for i, L in enumerate((20, 26, 30))))
    recs, s0 = list(recs), np.stack(s0).astype(f32)
    pool = replay.ReplayPool(m, slots=4, use_graph=False)
    first = pool.run(recs, s0)
    frames = pool.frames
    traj = kin.track_replay(skel, first, s0)
    pred = np.concatenate([replay.trim_like_reference(q) for q, _ in traj])
    gt = pred.copy()
    gt[:, :57] += 0.03
    gt[:, :3] += np.concatenate([np.arange(q.shape[0]) for q, _ in traj])[:, None] * f32(0.004)      # and drifting away
    offs = np.concatenate([[0], np.cumsum([q.shape[0] for q, _ in traj])])
    got = kin.evaluate(skel, pred, gt, offs, start=8, end=2)
    again = pool.run(recs, s0)
    assert pool.frames == frames == 29
    for a, b in zip(first, again):
        assert np.array_equal(a.valid, b.valid)
        assert np.array_equal(a.s_rest.view(np.int32), b.s_rest.view(np.int32)) and np.array_equal(a.c_t.view(np.int32), b.c_t.view(np.int32))
    noise_r = noise_v = err_r = err_v = 0.0
    for i, (r, (qdq, viz)) in enumerate(zip(first, traj)):
        assert qdq.shape == (r.s_rest.shape[0], 114) and np.array_equal(qdq[:, 3:], r.s_rest) and r.valid.sum() == r.s_rest.shape[0] - PRIMING
        ref_r, ref_v, _ = ko.track(TABLE, s0[i].astype(np.float64), r.s_rest.astype(np.float64), r.c_t.astype(np.float64), r.valid)
        low_r, low_v, _ = ko.track(TABLE, s0[i].astype(np.float64), r.s_rest.astype(np.float64), r.c_t.astype(np.float64), r.valid, dtype=f32)
        noise_r, noise_v = max(noise_r, float(np.abs(low_r - ref_r).max())), max(noise_v, float(np.abs(low_v - ref_v).max()))
        err_r, err_v = max(err_r, float(np.abs(qdq[:, :3] - ref_r).max())), max(err_v, float(np.abs(viz - ref_v).max()))
        assert (qdq[:PRIMING, :3] == s0[i, :3]).all() and (viz[:PRIMING] == 100).all()
    print(f"end to end: fp32 noise root {noise_r:.3e} viz_locs {noise_v:.3e}; device error root {err_r:.3e} viz_locs {err_v:.3e}")
    assert err_r <= 3.0 * noise_r and err_v <= 3.0 * noise_v
    ref_m = _oracle_metrics(pred, gt, offs, np.float64, start=8, end=2)
    noise_m = np.abs(_oracle_metrics(pred, gt, offs, f32, start=8, end=2) - ref_m).max(0)
    err_m = np.abs(got - ref_m).max(0)
    print("end to end metrics: fp32 noise", noise_m, "device error", err_m)
    assert (err_m <= 3.0 * noise_m).all()
