"""CPU: the training-loss oracle (oracle/loss_oracle.py) against losses and autograd gradients of the REAL reference
functions (tests/golden/make_loss_golden.py -> tip_loss_golden.npz; fp32 torch)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from make_loss_golden import CASES, N_SBPS, make_case   # noqa: E402  (synthetic input generator: data, not reference code)
from oracle import loss_oracle                           # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden", "tip_loss_golden.npz")
REL = 2e-5    # the golden side is fp32 torch (fp32 means over up to 8640 squares); the oracle is fp64


def case_inputs(z, tag):
    B, T, seed = CASES[tag]
    pred, gt = make_case(tag, B, T, seed)
    chk = np.array([pred.astype(np.float64).sum(), np.nansum(gt.astype(np.float64)), np.isnan(gt).sum()])
    assert np.allclose(chk, z[tag + "/insum"], rtol=0, atol=1e-9), "synthetic inputs drifted from the golden run"
    return pred, gt


def close(a, b, rel=REL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(a)
    scale = max(1.0, float(np.abs(b[m]).max())) if m.any() else 1.0
    return (not m.any()) or float(np.abs(a[m] - b[m]).max()) <= rel * scale


def test_train_loss_matches_reference():
    z = np.load(GOLD)
    for tag in CASES:
        pred, gt = case_inputs(z, tag)
        total, parts, grad = loss_oracle.train_loss(pred, gt, N_SBPS)
        ref = z[tag + "/losses"]
        assert close([total, *parts], ref), (tag, total, parts, ref)
        g = z[tag + "/grad"]
        assert np.isfinite(grad).all()
        assert np.abs(grad - g).max() <= REL * max(1.0, np.abs(g).max()), tag


def test_nan_cases_are_nan_like_the_reference():
    z = np.load(GOLD)
    assert np.isnan(z["t3/losses"][[0, 3]]).all() and np.isfinite(z["t3/losses"][[1, 2]]).all()      # no jerk sample at T = 3
    assert np.isnan(z["allmask/losses"][[0, 1]]).all() and np.isfinite(z["allmask/losses"][[2, 3]]).all()
    # rows dropped by a mask get exactly zero gradient, in the reference and in the oracle
    pred, gt = case_inputs(z, "allmask")
    assert np.all(z["allmask/grad"][:, :, 108:111] == 0.0)
    assert np.all(loss_oracle.train_loss(pred, gt, N_SBPS)[2][:, :, 108:111] == 0.0)


def test_saturated_sigmoid_costs_100_and_has_no_gradient():
    z = np.load(GOLD)
    pred, gt = case_inputs(z, "sat")
    g = z["sat/grad"][:, :, 111::4]
    x = pred[:, :, 111::4]
    dead = (x >= 30.0) | (x <= -100.0)                        # sigmoid == 1.0f / 0.0f exactly; at -30 p = 9.4e-14 survives
    assert dead.any() and np.all(g[dead] == 0.0)              # torch: BCE backward (eps 1e-12) times p (1 - p) = 0
    assert np.all(loss_oracle.train_loss(pred, gt, N_SBPS)[2][:, :, 111::4][dead] == 0.0)
    # the fp64-sigmoid variant differs there, which is why the oracle restates the fp32 rounding
    assert abs(loss_oracle.train_loss(pred, gt, N_SBPS, f32_sigmoid=False)[1][1] - z["sat/losses"][2]) > 1.0


def test_separate_functions_match_reference():
    z = np.load(GOLD)
    pred, gt = case_inputs(z, "mix")
    p2, g2 = pred.reshape(-1, 131), gt.reshape(-1, 131)
    lq, gq = loss_oracle.loss_q_only_2axis(g2[:, :-20], p2[:, :-20])
    lc, gc = loss_oracle.loss_constr_multi(g2[:, -20:], p2[:, -20:])
    lj, gj = loss_oracle.loss_jerk(pred[:, :, :-23])
    for name, l, g, sl in (("q", lq, gq.reshape(3, 12, 111), np.s_[:, :, :111]), ("c", lc, gc.reshape(3, 12, 20), np.s_[:, :, 111:]),
                           ("j", lj, gj, np.s_[:, :, :108])):
        assert close([l], z[f"mix_{name}/loss"]), name
        full = np.zeros((3, 12, 131))
        full[sl] = g
        ref = z[f"mix_{name}/grad"]
        assert np.abs(full - ref).max() <= REL * max(1.0, np.abs(ref).max()), name


def test_constraint_loss_with_many_constraints_matches_reference():
    """loss_constr_multi for N = 17 / 24 / 64 constraints per row (the model emits 5): reference-generated golden."""
    from make_loss_golden import WIDE_CASES, make_constr_case
    z = np.load(GOLD)
    for tag, args in WIDE_CASES.items():
        gt, pred = make_constr_case(*args)
        chk = np.array([pred.astype(np.float64).sum(), np.nansum(gt.astype(np.float64)), np.isnan(gt).sum()])
        assert np.allclose(chk, z[tag + "/insum"], rtol=0, atol=1e-9)
        l, g = loss_oracle.loss_constr_multi(gt, pred)
        assert close([l], z[tag + "/loss"]), tag
        ref = z[tag + "/grad"]
        assert np.abs(g - ref).max() <= REL * max(1.0, np.abs(ref).max()), tag
        assert np.all(g[7] == 0.0) and np.all(ref[7] == 0.0)


# ---- layouts narrower than the reference's 108 + 3 + 20 (shared with tests/test_loss_edges_gpu.py) --------------------------
NARROW_LAYOUTS = ((12, 2), (60, 1))       # (n_pose, n_sbps): W = 23 and 67
NARROW_SHAPES = ((3, 12), (2, 19))        # (B, T)


def make_narrow_case(n_pose, n_sbps, B, T, seed):
    """make_case's value ranges and NaN masks on rows of n_pose + 3 + 4 * n_sbps columns (float32 values)."""
    rng = np.random.RandomState(seed)
    nq, W = n_pose + 3, n_pose + 3 + 4 * n_sbps
    pred = rng.standard_normal((B, T, W)).astype(np.float32)
    gt = rng.standard_normal((B, T, W)).astype(np.float32) * 0.5
    c = gt[:, :, nq:].reshape(B, T, n_sbps, 4)
    c[..., 0] = (rng.rand(B, T, n_sbps) < 0.4).astype(np.float32)
    c[..., 1:] = rng.uniform(-0.25, 0.25, (B, T, n_sbps, 3)).astype(np.float32)
    rows_v = rng.rand(B, T) < 0.3
    rows_c = rng.rand(B, T) < 0.2
    gt[rows_v, n_pose:n_pose + 2] = np.nan
    gt[rows_v & (rng.rand(B, T) < 0.5), n_pose + 2] = np.nan
    gt[rows_c, nq + 4 * rng.randint(0, n_sbps)] = np.nan
    return pred, gt


def autograd_train_loss(pred, gt, n_sbps):
    """The three loss formulas (learning_utils.py:13-78, summed as train_model.py:185-187) stated once more in float64 torch, on
    rows of any width, with the gradient from autograd: (total, [loss_q, loss_c, loss_j], d total / d pred)."""
    import torch
    yp = torch.tensor(np.asarray(pred, np.float64), requires_grad=True)
    y = torch.tensor(np.asarray(gt, np.float64))
    W = yp.shape[-1]
    nq = W - 4 * n_sbps
    pose = yp[:, :, :nq - 3]
    jerk = pose[:, 3:] - 3 * pose[:, 2:-1] + 3 * pose[:, 1:-2] - pose[:, :-3]
    lj = (jerk ** 2).mean() * 100.0
    p2, g2 = yp.reshape(-1, W), y.reshape(-1, W)
    lq = ((p2[:, :nq - 3] - g2[:, :nq - 3]) ** 2).mean() * 100.0
    keep = ~torch.isnan(g2[:, nq - 3:nq - 1]).any(dim=1)
    lq = lq + ((p2[keep, nq - 3:nq - 1] - g2[keep, nq - 3:nq - 1]) ** 2).mean() * 6.0
    lq = lq + ((p2[keep, nq - 1:nq] - g2[keep, nq - 1:nq]) ** 2).mean() * 12.0
    keep = ~torch.isnan(g2[:, nq:]).any(dim=1)
    pc, gc = p2[keep, nq:], g2[keep, nq:]
    lc = 0.0
    for i in range(n_sbps):
        prob, t = torch.sigmoid(pc[:, 4 * i]), gc[:, 4 * i]
        bce = -(t * torch.log(prob).clamp(min=-100.0) + (1.0 - t) * torch.log(1.0 - prob).clamp(min=-100.0)).mean()
        lc = lc + bce + ((pc[:, 4 * i + 1:4 * i + 4] - gc[:, 4 * i + 1:4 * i + 4] * 5.0) ** 2).mean() * 4.0
    lc = lc / n_sbps * 2.5
    total = (lc + lq) + lj
    total.backward()
    return total.item(), np.array([lq.item(), lc.item(), lj.item()]), yp.grad.numpy()


def test_oracle_at_other_widths_matches_an_autograd_restatement():
    """The oracle takes its widths from its arguments; at W = 23, 67 (and 131, where the golden file pins it too) it equals the
    autograd restatement to fp64 rounding."""
    cases = [(n_pose, n_sbps, B, T, make_narrow_case(n_pose, n_sbps, B, T, 40 + B + n_pose))
             for n_pose, n_sbps in NARROW_LAYOUTS for B, T in NARROW_SHAPES]
    cases.append((108, N_SBPS, 3, 12, make_case("mix", 3, 12, 0)))
    for n_pose, n_sbps, B, T, (pred, gt) in cases:
        assert pred.shape == (B, T, n_pose + 3 + 4 * n_sbps)
        total, parts, grad = loss_oracle.train_loss(pred, gt, n_sbps, f32_sigmoid=False)
        a_total, a_parts, a_grad = autograd_train_loss(pred, gt, n_sbps)
        assert np.isfinite(a_total) and np.abs(a_grad).max() > 0
        assert abs(total - a_total) <= 1e-12 * abs(a_total), (n_pose, B, T)
        assert np.abs(parts - a_parts).max() <= 1e-12 * np.abs(a_parts).max()
        assert np.abs(grad - a_grad).max() <= 1e-12 * np.abs(a_grad).max()
        # the separate functions on the column slices train_model.py:177-183 takes
        nq = n_pose + 3
        p2, g2 = pred.reshape(-1, pred.shape[-1]), gt.reshape(-1, gt.shape[-1])
        lq, gq = loss_oracle.loss_q_only_2axis(g2[:, :nq], p2[:, :nq])
        lc, gc = loss_oracle.loss_constr_multi(g2[:, nq:], p2[:, nq:], f32_sigmoid=False)
        lj, gj = loss_oracle.loss_jerk(pred[:, :, :n_pose])
        assert np.abs(np.array([lq, lc, lj]) - a_parts).max() <= 1e-12 * np.abs(a_parts).max()
        full = np.concatenate([gq, gc], axis=1).reshape(B, T, -1)
        full[:, :, :n_pose] += gj
        assert np.abs(full - a_grad).max() <= 1e-12 * np.abs(a_grad).max()
