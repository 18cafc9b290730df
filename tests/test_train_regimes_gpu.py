"""GPU: the HIP training step held to the fp64 training oracle (oracle/train_oracle.py) in the regimes the paper-config tests of
tests/test_train_gpu.py do not reach: the model train_model.py builds at its argparse defaults (synth.TRAIN_DEFAULT: 8 heads,
head width 32, no acc-sum, past-state dropout 0.8, batch 128 — the layer-by-layer path, the fused one needs 16 heads), batches
up to 777 windows, windows longer than 40 frames and the scaled widths' panel GEMM.

Large batches are compared through a SPARSE COTANGENT: dL/dy is non-zero only on a set S of <= 10 windows (tile and round edges,
the remainder), so every weight gradient of the B-window step is the gradient of S alone and the input gradients of every other
window are exactly zero (windows are independent; tests/test_train_oracle.py:test_sparse_cotangent_premise).  The fp64 oracle then
runs on S only.  Each sparse case also shows that it could see a lost window: the oracle on S minus one window must be > 1e-3 away.

Regime comments name what tip_train.hip / tip_attn.hip dispatch for the case (M = B * T rows; 256 CUs on an MI355X).
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from tip_amd import synth, lib as tlib
from oracle import oracle, train_oracle
from test_host_cpu import make_model, load_synth
from test_train_gpu import REL, _train_model, _hip_step, _gates, _check_grads
from test_train_oracle import (DEFAULT_GOLD, DEFAULT_CASES, DEFAULT_FWD_SEED, case_inputs, check_y, default_fwd_inputs,
                               digest_close, sparse_windows)

pytestmark = pytest.mark.gpu

TRAIN_DEFAULT = synth.TRAIN_DEFAULT        # dict(synth.PAPER, n_heads=8, with_acc_sum=False): train_model.py:44-66,95-107
HD64 = dict(synth.PAPER, n_heads=4)        # d = 256, head width 64
SCALED2 = dict(synth.SCALED, tf_layers=2)  # D = 1024, F = 4096, 16 heads (head width 64)
TOL_TIGHT = 2e-5                           # fp32 plans against the fp64 forward oracle (tests/test_hip_parity.py)
P_STATE_DEFAULT = 0.8                      # train_model.py:64 --past_dropout


def _step(m, x_imu, x_s, cot, seed, input_grads=False):
    """_hip_step with the torch-op composite's warning turned into an error: the case must run on the HIP training function."""
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*torch-op training composite")
        return _hip_step(m, x_imu, x_s, cot, seed=seed, input_grads=input_grads)


def _keep_mask(m, x_s, seed):
    """(keep mask, scale) the step applied to x_s: the module's hashed past-state mask for seed (its _draw_seeds gives [seed, seed])."""
    p = m.past_state_dropout
    if p <= 0.0:
        return None, 1.0
    mask = m._hash_keep_mask(torch.tensor(x_s).cuda(), seed).cpu().numpy()
    return mask, 1.0 / (1.0 - p)


def _rel_all(g, go):
    """relative L2 distance of the whole gradient set"""
    num = sum(float(((g[n].astype(np.float64) - go[n]) ** 2).sum()) for n in go)
    den = sum(float((go[n] ** 2).sum()) for n in go)
    return (num / den) ** 0.5


def _pgemm_launches():
    n = ctypes.c_ulonglong(0)
    assert tlib.load().tip_debug_pgemm_launches(ctypes.byref(n)) == 0
    return n.value


def _sparse_case(cfg, B, T, p_enc, wseed, p_state=0.0, fp64=False, rel=REL, ytol=2e-5):
    """One sparse-cotangent case: the HIP step on B windows, the fp64 oracle on S = sparse_windows(B).  Returns the worst tensor."""
    if fp64:
        m = make_model(cfg, p_state=p_state)
        w = load_synth(m, cfg, wseed)
        m = m.double().cuda().train()
        m.ENCODER_DROPOUT = p_enc
    else:
        m, w = _train_model(cfg, wseed, p_enc, p_state)
    dt = np.float64 if fp64 else np.float32
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=1000 + B + T)
    x_imu, x_s = x_imu.astype(dt), x_s.astype(dt)
    S = sparse_windows(B)
    cot = np.zeros((B, T, cfg["size_s"]), dtype=dt)
    cot[S] = synth.normal(2000 + B, "cot", len(S) * T * cfg["size_s"]).reshape(len(S), T, -1)
    seed = 424242 + 7 * B + T
    y, g, ex = _step(m, x_imu, x_s, cot, seed, input_grads=not fp64)   # (input gradients: fp32 step only)
    assert len(g) == 56 - 12 * (4 - cfg["tf_layers"])
    gates = None if fp64 else [a[S] for a in _gates(m, cfg, B, T)]
    mask, scale = _keep_mask(m, x_s, seed)
    ms = None if mask is None else mask[S]
    yo, go, (dxi_o, dxs_o) = train_oracle.step(cfg, w, x_imu[S], x_s[S], cot[S], keep_mask=ms, keep_scale=scale, p_drop=p_enc,
                                               seed=seed, relu_gates=gates, window_ids=S, input_grads=True)
    ey = np.abs(y[S] - yo).max()
    assert ey < ytol, ey
    worst = _check_grads(g, go, rel)
    if not fp64:
        rest = np.setdiff1d(np.arange(B), S)
        for name, a, b in (("x_imu", ex["dx_imu"], dxi_o), ("x_s", ex["dx_s"], dxs_o)):
            for i, wi in enumerate(S):
                e = np.linalg.norm(a[wi].astype(np.float64) - b[i]) / (np.linalg.norm(b[i]) + 1e-30)
                assert e < rel, (name, int(wi), e)
            assert (a[rest] == 0).all(), name                      # exact zeros outside S, bit for bit
    # sensitivity: the oracle without S's last window is far from what the step computed
    S1 = S[:-1]
    _, go1 = train_oracle.step(cfg, w, x_imu[S1], x_s[S1], cot[S1], keep_mask=None if ms is None else ms[:-1], keep_scale=scale,
                               p_drop=p_enc, seed=seed, relu_gates=None if gates is None else [a[:-1] for a in gates], window_ids=S1)
    lost = _rel_all(g, go1)
    assert lost > 1e-3, lost
    print(f"B={B} T={T} |S|={len(S)} p_enc={p_enc} p_state={p_state}: max|dy| {ey:.2e}, worst tensor {worst[0]} {worst[1]:.2e}, "
          f"minus one window {lost:.2e}")
    return m, worst


# ---- a. TRAIN_DEFAULT, dense, at its literal defaults ------------------------------------------------------------------------

def test_train_model_defaults_dense_step():
    """train_model.py's default model and batch (B = 128, T = 40): encoder dropout 0.1 and past-state dropout 0.8 live, the full fp64
    oracle step (y, all 56 tensors) and the input gradients (tip_train_input_grads); the step re-run is bit-identical.
    Regimes: 8 heads -> layer-by-layer path (tip_fused.hip needs 16), D/256 == 1 LayerNorm instantiations, mattn_fwd/bwd<32, 3>
    with the q-scale applied in the kernel (tip_abi.hip folds it into the weights for head widths 16 and 64 only); M = 5120:
    dwgemm (128 x 64 wave tile, splits from dw_choose_splits) for the encoder weights, split tgemm for dW_out (131 rows, not
    128-aligned)."""
    cfg = TRAIN_DEFAULT
    B, T, seed = 128, 40, 987654
    m, w = _train_model(cfg, 7, 0.1, P_STATE_DEFAULT)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=128)
    assert x_imu.shape[2] == 72
    cot = synth.normal(128, "cot", B * T * cfg["size_s"]).reshape(B, T, -1).astype(np.float32)
    y, g, ex = _step(m, x_imu, x_s, cot, seed, input_grads=True)
    gates = _gates(m, cfg, B, T)
    mask, scale = _keep_mask(m, x_s, seed)
    assert 0.15 < mask.mean() < 0.25
    yo, go, (dxi_o, dxs_o) = train_oracle.step(cfg, w, x_imu, x_s, cot, keep_mask=mask, keep_scale=scale, p_drop=0.1, seed=seed,
                                               relu_gates=gates, input_grads=True)
    assert np.abs(y - yo).max() < 2e-5, np.abs(y - yo).max()
    worst = _check_grads(g, go)
    for name, a, b in (("x_imu", ex["dx_imu"], dxi_o), ("x_s", ex["dx_s"], dxs_o)):
        e = np.linalg.norm(a.astype(np.float64) - b) / (np.linalg.norm(b) + 1e-30)
        assert e < REL, (name, e)
    print("train_model defaults B=128 T=40: max|dy|", np.abs(y - yo).max(), "worst tensor", worst)
    y2, g2, ex2 = _step(m, x_imu, x_s, cot, seed, input_grads=True)
    assert np.array_equal(y, y2) and all(np.array_equal(g[n], g2[n]) for n in g)
    assert np.array_equal(ex["dx_imu"], ex2["dx_imu"]) and np.array_equal(ex["dx_s"], ex2["dx_s"])
    m.check_handoffs()


# ---- b. TRAIN_DEFAULT vs the reference's own gradients -----------------------------------------------------------------------

@pytest.mark.parametrize("tag", list(DEFAULT_CASES))
def test_train_model_defaults_against_reference_golden(tag):
    z = np.load(DEFAULT_GOLD)
    cfg = TRAIN_DEFAULT
    m, w = _train_model(cfg, DEFAULT_CASES[tag], 0.0)
    x_imu, x_s, cot = case_inputs(z, tag, cfg, DEFAULT_CASES)
    y, g, _ = _step(m, x_imu, x_s, cot, None)
    check_y(z, tag, y, 2e-5)
    for i, n in enumerate(w.keys()):
        digest_close(n, train_oracle.digest(n, g[n]), z[tag + "/digests"][i], rtol=4e-4)


# ---- c. batch regimes, sparse ------------------------------------------------------------------------------------------------
# M = B * T rows feed every weight gradient.  T = 40: M % 4 == 0, so dwgemm_ok holds for the encoder / recurrence weights
# (n_store 768 / 1024 / 256 / 512, all 128-aligned; K 256 / 1024 / 512) and dw_choose_splits picks split-K from M / 128 upward as
# M grows (B = 17: one or a few splits; B >= 129: many, the last one a remainder of klen); dW_out (131 rows) and dW_in (203 / 221
# columns, padded to K = 224: K % 64 != 0) always take the split tgemm.  B * T odd ((257, 33), (777, 37)): dwgemm_ok is false for every weight gradient -> the
# LDS-tiled split tgemm + splitk_reduce for all of them.  PAPER (16 heads, T <= 40) runs the fused encoder and fused backward
# (win_g); TRAIN_DEFAULT (8 heads) the layer-by-layer path with mattn<32, 3>.  B = 17 / 65 / 129 / 257 / 513 / 777: remainders of
# the 16-window recurrence tiles and of a 256-CU round.

BATCH_CASES = [(B, 40) for B in (17, 64, 65, 129, 255, 257, 300, 513, 777)] + [(257, 33), (777, 37)]


@pytest.mark.parametrize("cname", ["paper", "train_default"])
@pytest.mark.parametrize("B,T", BATCH_CASES)
def test_batch_regimes_sparse(cname, B, T):
    cfg = synth.PAPER if cname == "paper" else TRAIN_DEFAULT
    p_enc = 0.1 if B in (257, 777) else 0.0                                # encoder dropout live: masks of windows far into the batch
    p_state = P_STATE_DEFAULT if cname == "train_default" else 0.0
    _sparse_case(cfg, B, T, p_enc, 11, p_state)


# ---- d. window lengths, dense ------------------------------------------------------------------------------------------------
# T > 40 leaves the fused path (fz::TMAX = 40; win_g needs T <= 40).  Attention (tip_attn.hip mattn_fwd_dh / mattn_bwd_dh):
# T <= 48 -> <DH, 3>, 49..80 -> <DH, 5>, 81..128 -> <DH, 8>; DH = 16 (PAPER), 32 (TRAIN_DEFAULT), 64 (HD64).  T = 128 is the
# largest window tip_train accepts (train_supported).

LONG_T = (41, 48, 49, 64, 80, 81, 100, 128)
LONG_CASES = ([("paper", T, B) for T in LONG_T for B in (3, 17)] + [("train_default", T, B) for T in LONG_T for B in (3, 17)]
              + [("hd64", T, B) for T in (81, 128) for B in (3, 17)])


@pytest.mark.parametrize("cname,T,B", LONG_CASES)
def test_long_windows_dense(cname, T, B):
    cfg = {"paper": synth.PAPER, "train_default": TRAIN_DEFAULT, "hd64": HD64}[cname]
    p_enc = 0.1 if T in (49, 128) else 0.0                                 # dropout-live mattn_fwd / bwd at <DH,5> and <DH,8>
    m, w = _train_model(cfg, 13, p_enc)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=3000 + T + B)
    cot = synth.normal(3000 + T, "cot", B * T * cfg["size_s"]).reshape(B, T, -1).astype(np.float32)
    seed = 5550 + T + B
    y, g, _ = _step(m, x_imu, x_s, cot, seed)
    yo, go = train_oracle.step(cfg, w, x_imu, x_s, cot, p_drop=p_enc, seed=seed, relu_gates=_gates(m, cfg, B, T))
    assert np.abs(y - yo).max() < 2e-5, np.abs(y - yo).max()
    print(cname, f"B={B} T={T} p_enc={p_enc}: max|dy| {np.abs(y - yo).max():.2e}, worst tensor", _check_grads(g, go))


# ---- e. scaled widths on the panel GEMM, sparse ------------------------------------------------------------------------------
# D = 1024, F = 4096, T = 80.  lin_launch takes pgemm_tg_kernel once panel_ok holds ((N / 512) * ceil(M / 80) >= 2 x 256 CUs):
# B = 128 -> the QKV (N = 3072) and FFN-1 (N = 4096) forward linears and the backward's dX through linear2 (N = 4096); B = 256 ->
# every 1024-wide linear too.  dwgemm: K % 128 == 0 and (n_store / 128) * (K / 128) >= 256 for the FFN weights -> the 128 x 128
# wave tile (NB = 2), with split-K over M = 10 240 / 20 480 rows.  mattn<64, 5>.

@pytest.mark.parametrize("B", [128, 256])
def test_scaled_widths_panel_gemm_sparse(B):
    n0 = _pgemm_launches()
    _sparse_case(SCALED2, B, 80, 0.0, 4)
    n = _pgemm_launches() - n0
    print(f"scaled B={B}: {n} panel-GEMM launches")
    # per layer: QKV and FFN-1 forward, dX through linear2 (B = 128); all four forward linears and their four dX GEMMs (B = 256)
    assert n >= (3 if B == 128 else 8) * SCALED2["tf_layers"], "the training step did not take the panel GEMM"


# ---- f. the fp64 step, sparse ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname", ["paper", "train_default"])
@pytest.mark.parametrize("B", [17, 100, 257])
def test_f64_step_sparse(cname, B):
    cfg = synth.PAPER if cname == "paper" else TRAIN_DEFAULT
    _sparse_case(cfg, B, 40, 0.1 if B == 257 else 0.0, 12, fp64=True, rel=1e-11, ytol=1e-11)


# ---- g. inference at TRAIN_DEFAULT -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T", [(1, 1), (1, 40), (3, 17), (128, 40), (300, 40), (2, 100)])
def test_train_model_defaults_inference(B, T):
    """.eval() forward of the default model (plans auto and general, and forward_last) against the fp64 forward oracle."""
    cfg = TRAIN_DEFAULT
    m = make_model(cfg)
    w = load_synth(m, cfg, 21)
    m = m.cuda().eval()
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=4000 + B + T)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64)
    for plan in ("auto", "general"):
        m.set_plan(plan)
        n0 = m.hip_forward_count()
        with torch.no_grad():
            y = m(xi, xs).cpu().numpy()
            yl = m.forward_last(xi, xs).cpu().numpy()
        assert m.hip_forward_count() == n0 + 2
        e = np.abs(y - yo).max()
        assert e < TOL_TIGHT, (plan, e)
        assert np.abs(yl - yo[:, -1]).max() < TOL_TIGHT, plan
    m.check_handoffs()


def test_train_model_defaults_f64_forward_against_reference_golden():
    z = np.load(DEFAULT_GOLD)
    cfg = TRAIN_DEFAULT
    m = make_model(cfg)
    load_synth(m, cfg, DEFAULT_FWD_SEED)
    m = m.double().cuda().eval()
    x_imu, x_s = default_fwd_inputs(z)
    n0 = m.hip_forward_count()
    with torch.no_grad():
        y = m(torch.tensor(x_imu, dtype=torch.float64).cuda(), torch.tensor(x_s, dtype=torch.float64).cuda()).cpu().numpy()
    assert m.hip_forward_count() == n0 + 1
    assert np.abs(y - z["fwd/y64"]).max() < 1e-11, np.abs(y - z["fwd/y64"]).max()


def test_train_model_defaults_few_window_train_mode_call():
    """The unedited runner's call on the default model: .train() mode, one window, no autograd.  The stash-free few-stream kernels
    (tip_forward_dropout) serve the 16-head model only (latency_supported -> fused_supported), so at 8 heads the call is
    tip_train_forward itself: the same y, bit for bit, as the autograd call of tip_train_forward with the same seeds (not the
    torch-op composite), and that y is the fp64 oracle's with both dropouts applied."""
    cfg = TRAIN_DEFAULT
    m = make_model(cfg, p_state=P_STATE_DEFAULT)
    w = load_synth(m, cfg, 0)
    m = m.cuda().train()
    m.ENCODER_DROPOUT = 0.1
    x_imu, x_s = synth.make_inputs(cfg, 1, 40, seed=4321)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    seed = 777001
    m._draw_seeds = lambda: [seed, seed]
    try:
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore", message=".*under torch.no_grad")
            warnings.filterwarnings("error", message=".*torch-op training composite")
            n0 = m.hip_forward_count()
            with torch.no_grad():
                y_ng = m(xi, xs)
            assert m.hip_forward_count() == n0 + 1
            y_tr = m(xi, xs)
            assert type(y_tr.grad_fn).__name__.startswith("_HipTrainFunction") and y_tr.grad_fn.lazy is None   # tip_train_forward
    finally:
        del m._draw_seeds
    torch.cuda.synchronize()
    assert torch.equal(y_ng, y_tr.detach())
    mask, scale = _keep_mask(m, x_s, seed)
    params = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in w.items()}
    yo = train_oracle.forward(cfg, params, x_imu, x_s, keep_mask=mask, keep_scale=scale, p_drop=0.1, seed=seed).numpy()
    e = float(np.abs(y_ng.cpu().numpy() - yo).max())
    assert e < 2e-5, e
    m.check_handoffs()
