"""CPU: the training-step oracle (oracle/train_oracle.py) against digests of the REAL reference's gradients
(tests/golden/make_train_golden.py), and the module's torch-op composite against the same oracle."""
import os

import numpy as np
import pytest
import torch

import tip_amd
from tip_amd import synth
from oracle import train_oracle
from test_host_cpu import make_model, load_synth

GOLD = os.path.join(os.path.dirname(__file__), "golden", "tip_train_golden.npz")
CASES = {"train_s0_B2_T40": 0, "train_s1_B3_T17": 1, "train_s2_B12_T40": 2}   # tag -> weight / input seed


# the model train_model.py builds at its argparse defaults (synth.TRAIN_DEFAULT: 8 heads, no acc-sum), same recipe
# (tests/golden/make_train_golden.py --train-default)
DEFAULT_GOLD = os.path.join(os.path.dirname(__file__), "golden", "tip_train_default_golden.npz")
DEFAULT_CASES = {"tdef_s0_B2_T40": 0, "tdef_s1_B3_T17": 1, "tdef_s2_B12_T40": 2}
DEFAULT_FWD_SEED = 3                                  # weights seed of the forward golden ("fwd/*"; inputs: seed 600 + 3, B=1, T=40)


def default_fwd_inputs(z):
    """(x_imu, x_s) of the TRAIN_DEFAULT forward golden, regenerated and checked against its checksum."""
    x_imu, x_s = synth.make_inputs(synth.TRAIN_DEFAULT, 1, 40, seed=600 + DEFAULT_FWD_SEED)
    chk = np.array([x_imu.astype(np.float64).sum(), np.nansum(x_s.astype(np.float64))])
    assert np.allclose(chk, z["fwd/insum"], rtol=0, atol=1e-6), "synthetic inputs drifted from the golden run"
    return x_imu, x_s


def case_inputs(z, tag, cfg=synth.PAPER, cases=CASES):
    """(x_imu, x_s, cot) of a golden case: stored for the small ones, regenerated from the generator's seeds (and checked
    against its checksum) for the larger one."""
    if tag + "/x_imu" in z.files:
        return z[tag + "/x_imu"], z[tag + "/x_s"], z[tag + "/cot"]
    seed = cases[tag]
    B, T = int(tag.split("_B")[1].split("_")[0]), int(tag.split("_T")[1])
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=500 + seed)
    cot = synth.normal(900 + seed, "train/cot", B * T * cfg["size_s"]).reshape(B, T, cfg["size_s"]).astype(np.float32)
    chk = np.array([x_imu.astype(np.float64).sum(), np.nansum(x_s.astype(np.float64)), cot.astype(np.float64).sum()])
    assert np.allclose(chk, z[tag + "/insum"], rtol=0, atol=1e-6), "synthetic inputs drifted from the golden run"
    return x_imu, x_s, cot


def check_y(z, tag, y, tol):
    if tag + "/y" in z.files:
        assert np.abs(y - z[tag + "/y"]).max() < tol
    else:
        assert np.abs(y[-1] - z[tag + "/y_last_window"]).max() < tol


def digest_close(name, got, want, rtol=2e-4):
    """digest entries are sums over up to 262144 terms of fp32 reference gradients: compare relative to the tensor's
    L2 norm (sqrt of entry 1), which is what bounds their rounding."""
    scale = np.sqrt(max(want[1], 1e-30))
    n_dir = scale * 1.0
    assert abs(got[1] - want[1]) <= 4 * rtol * want[1] + 1e-12, (name, "sumsq", got[1], want[1])
    assert abs(got[2] - want[2]) <= rtol * n_dir * 8 + 1e-9, (name, "projection", got[2], want[2])
    assert np.all(np.abs(got[3:] - want[3:]) <= rtol * scale + 1e-7), (name, "entries", got[3:], want[3:])


@pytest.mark.parametrize("tag", list(CASES))
def test_oracle_matches_reference_gradients(tag):
    z = np.load(GOLD)
    cfg = synth.PAPER
    w = synth.make_weights(cfg, seed=CASES[tag])
    x_imu, x_s, cot = case_inputs(z, tag)
    y, grads = train_oracle.step(cfg, w, x_imu, x_s, cot)
    check_y(z, tag, y, 5e-6)
    names = list(w.keys())
    gn = np.sqrt(sum((g.astype(np.float64) ** 2).sum() for g in grads.values()))
    assert abs(gn - z[tag + "/gnorm"][0]) < 1e-4 * gn
    for i, n in enumerate(names):
        digest_close(n, train_oracle.digest(n, grads[n]), z[tag + "/digests"][i])


@pytest.mark.parametrize("tag", list(DEFAULT_CASES))
def test_oracle_matches_reference_gradients_at_train_model_defaults(tag):
    """The same pin at train_model.py's default model (--n_heads 8: head width 32; no --with_acc_sum: 203 input columns), which
    the GPU tests of the layer-by-layer training path (tests/test_train_regimes_gpu.py) are held to."""
    z = np.load(DEFAULT_GOLD)
    cfg = synth.TRAIN_DEFAULT
    w = synth.make_weights(cfg, seed=DEFAULT_CASES[tag])
    x_imu, x_s, cot = case_inputs(z, tag, cfg, DEFAULT_CASES)
    assert x_imu.shape[2] == 72 and len(w) == 56
    y, grads = train_oracle.step(cfg, w, x_imu, x_s, cot)
    check_y(z, tag, y, 5e-6)
    names = list(w.keys())
    gn = np.sqrt(sum((g.astype(np.float64) ** 2).sum() for g in grads.values()))
    assert abs(gn - z[tag + "/gnorm"][0]) < 1e-4 * gn
    for i, n in enumerate(names):
        digest_close(n, train_oracle.digest(n, grads[n]), z[tag + "/digests"][i])


def test_forward_oracles_match_the_reference_at_train_model_defaults():
    """The reference's .eval() forward of the default model in fp32 and fp64 against oracle/oracle.py (C, fp64) and the training
    oracle's forward."""
    from oracle import oracle
    z = np.load(DEFAULT_GOLD)
    cfg = synth.TRAIN_DEFAULT
    w = synth.make_weights(cfg, seed=DEFAULT_FWD_SEED)
    x_imu, x_s = default_fwd_inputs(z)
    yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64)
    assert np.abs(yo - z["fwd/y64"]).max() < 1e-10
    assert np.abs(yo - z["fwd/y32"]).max() < 5e-6
    params = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in w.items()}
    assert np.abs(train_oracle.forward(cfg, params, x_imu, x_s).numpy() - z["fwd/y64"]).max() < 1e-10


SPARSE_PROBE = (0, 1, 15, 16, 63, 64, 255, 256)


def sparse_windows(B):
    """The windows a sparse-cotangent case differentiates: first and last, 16-window tile edges, round edges, the remainder."""
    return np.array(sorted({w for w in SPARSE_PROBE + (B - 2, B - 1) if 0 <= w < B}), dtype=np.int64)


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_sparse_cotangent_premise(p_drop):
    """Windows are independent: with a cotangent that is zero outside a set S of windows, every weight gradient of the full batch is
    the gradient of S alone (the oracle run on S, its encoder dropout hashed at the windows' full-batch indices: window_ids), and
    the input gradients of every other window are exactly zero.  What lets the GPU tests run the HIP step at B = 777 against an
    fp64 oracle on <= 10 windows."""
    cfg = dict(synth.TRAIN_DEFAULT, tf_layers=2)
    B, T, seed = 40, 12, 31337
    w = synth.make_weights(cfg, seed=6)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=61)
    S = sparse_windows(B)
    assert list(S) == [0, 1, 15, 16, 38, 39]
    cot = np.zeros((B, T, cfg["size_s"]), dtype=np.float32)
    cot[S] = synth.normal(62, "cot", len(S) * T * cfg["size_s"]).reshape(len(S), T, -1)
    mask = (synth.uniform01(63, "keep", x_s.size).reshape(x_s.shape) >= 0.8).astype(np.float32)
    y, g, (dxi, dxs) = train_oracle.step(cfg, w, x_imu, x_s, cot, keep_mask=mask, keep_scale=5.0, p_drop=p_drop, seed=seed,
                                         input_grads=True)
    ys, gs, (dxis, dxss) = train_oracle.step(cfg, w, x_imu[S], x_s[S], cot[S], keep_mask=mask[S], keep_scale=5.0, p_drop=p_drop,
                                             seed=seed, window_ids=S, input_grads=True)
    assert np.abs(y[S] - ys).max() < 1e-12
    for n in g:
        assert np.abs(g[n] - gs[n]).max() <= 1e-12 * (1.0 + np.abs(g[n]).max()), n
    assert np.abs(dxi[S] - dxis).max() < 1e-12 and np.abs(dxs[S] - dxss).max() < 1e-12
    rest = np.setdiff1d(np.arange(B), S)
    assert (dxi[rest] == 0).all() and (dxs[rest] == 0).all()
    assert np.isnan(x_s).any() and (dxs[np.isnan(x_s)] == 0).all()
    if p_drop > 0:
        # window_ids matters: the masks of windows 0.. of a batch of |S| are other masks
        _, g0 = train_oracle.step(cfg, w, x_imu[S], x_s[S], cot[S], keep_mask=mask[S], keep_scale=5.0, p_drop=p_drop, seed=seed)
        d = max(np.abs(g0[n] - gs[n]).max() / (np.abs(gs[n]).max() + 1e-30) for n in gs)
        assert d > 1e-3, d


def test_drop_scale_at_given_indices():
    full = train_oracle.drop_scale(77, 3, 5000, 0.1)
    idx = np.array([0, 17, 4096, 4999])
    assert np.array_equal(train_oracle.drop_scale(77, 3, 4, 0.1, idx), full[idx])


COND_GOLD = os.path.join(os.path.dirname(__file__), "golden", "tip_train_cond_golden.npz")
COND_GAINS = (2.0, 3.0)


@pytest.mark.parametrize("gain", COND_GAINS)
def test_oracle_matches_reference_gradients_outside_random_init(gain):
    """The training conditioning cases (tests/golden/make_train_golden.py --cond: weights x gain 2 / 3): the fp64 oracle against
    digests of the reference's fp64 gradients (tight) and of its fp32 gradients (to the reference's own fp32 noise)."""
    z = np.load(COND_GOLD)
    cfg = synth.PAPER
    w = synth.make_weights(cfg, seed=0, gain=gain)
    tag = f"traincond_g{gain:g}"
    y, grads = train_oracle.step(cfg, w, z["x_imu"], z["x_s"], z["cot"])
    assert np.abs(y - z[tag + "/y64"]).max() < 1e-10
    names = list(w.keys())
    gn = np.sqrt(sum((g.astype(np.float64) ** 2).sum() for g in grads.values()))
    assert abs(gn - z[tag + "/gnorm"][0]) < 1e-9 * gn
    noise = z[tag + "/ref_grad_noise"]
    assert noise.max() < 1e-4
    for i, n in enumerate(names):
        d = train_oracle.digest(n, grads[n])
        digest_close(n, d, z[tag + "/digests64"][i], rtol=1e-9)
        digest_close(n, d, z[tag + "/digests"][i], rtol=max(2e-4, 20 * float(noise[i])))


def test_dropout_hash_statistics_and_determinism():
    a = train_oracle.drop_scale(1234, 5, 200000, 0.1)
    b = train_oracle.drop_scale(1234, 5, 200000, 0.1)
    c = train_oracle.drop_scale(1234, 6, 200000, 0.1)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    keep = (a > 0).mean()
    assert abs(keep - 0.9) < 0.004
    assert np.allclose(a[a > 0], 1.0 / 0.9)
    assert np.all(train_oracle.drop_scale(1, 0, 10, 0.0) == 1.0)


def test_module_composite_matches_oracle_gradients():
    """The torch-op composite the module differentiates when the HIP training path does not apply (CPU tensors,
    unsupported configuration) computes the same gradients as the oracle."""
    cfg = synth.PAPER
    m = make_model(cfg)
    w = load_synth(m, cfg, 0)
    m = m.double().train()
    m.ENCODER_DROPOUT = 0.0
    x_imu, x_s = synth.make_inputs(cfg, 2, 9, seed=3)
    cot = np.random.RandomState(0).randn(2, 9, cfg["size_s"])
    y = m(torch.tensor(x_imu, dtype=torch.float64), torch.tensor(x_s, dtype=torch.float64))
    (y * torch.tensor(cot)).sum().backward()
    yo, go = train_oracle.step(cfg, w, x_imu, x_s, cot)
    assert np.abs(y.detach().numpy() - yo).max() < 1e-9
    for n, p in m.named_parameters():
        assert np.abs(p.grad.numpy() - go[n]).max() <= 1e-8 * (1 + np.abs(go[n]).max()), n


def test_train_oracle_without_rnn_and_other_widths_matches_forward_oracle():
    """The training oracle's forward (autograd graph) for the configurations the reference's constructor also builds
    (simple_transformer_with_state.py:43-46 with_rnn=False; --rnn_nhid other than 512, train_model.py:47-48) against the C / numpy
    forward oracle that the reference's goldens pin (tiny_nornn, tiny cases): same function, so the gradients it yields are those
    of the pinned forward."""
    import torch
    from oracle import oracle
    for cfg in (dict(synth.TINY, with_rnn=False), dict(synth.PAPER, with_rnn=False, tf_layers=1),
                dict(synth.PAPER, rnn_hid_size=192, tf_layers=1)):
        w = synth.make_weights(cfg, seed=4)
        x_imu, x_s = synth.make_inputs(cfg, 2, 9, seed=5)
        params = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in w.items()}
        y = train_oracle.forward(cfg, params, x_imu, x_s).numpy()
        yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64)
        assert np.abs(y - yo).max() < 1e-12, cfg
