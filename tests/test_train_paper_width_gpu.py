"""GPU: the HIP training step OFF the paper model, held to the fp64 training oracle (oracle/train_oracle.py) on the members of the
paper-width family (csrc/tip_fused.hip, fused_supported: tf_in_dim 256, 16 heads, tf_hid_size 1024, at most 224 input columns,
T <= 40, any depth) whose free axes — tf_layers, size_s, with_acc_sum, the input width — leave the paper's values.  The suite ran the
fused training step at L = 4, S = 131, In = 221 only; tests/test_paper_width_shapes_gpu.py did the same sweep for the inference plans.

Every case runs through _step (the torch-op composite's warning is an error) and checks: y against the oracle under 2e-5; every
gradient tensor under REL = 1e-5 (relative L2; the oracle differentiates the ReLU piece the run was on); the number of tensors;
a second step repeats y and every gradient bit for bit; no hand-off was lost.  tests/test_train_paper_width_cpu.py holds the premises:
a dropped output column moves the gradient set by 6e-2 .. 1e-1, and the oracle's own fp32 form stays under REL / 3 at every depth.
The comment beside a case names the branch of csrc/tip_train.hip / csrc/tip_fused.hip it is there for."""
import warnings

import numpy as np
import pytest
import torch

from tip_amd import synth, lib as tlib
from oracle import train_oracle
from test_host_cpu import make_model, load_synth
from test_train_gpu import REL, _train_model, _hip_step, _gates, _check_grads
from test_train_regimes_gpu import _step, _sparse_case, _keep_mask, _rel_all
from test_train_paper_width_cpu import TABLE as _TABLE, DEPTHS, WIDTHS, YTOL, cotangent, n_tensors, _cfg

pytestmark = pytest.mark.gpu

TABLE = dict(_TABLE, **{
    "L2_S143n": _cfg(tf_layers=2, size_s=143, with_acc_sum=False),
    "L7_S127": _cfg(tf_layers=7, size_s=127),
    "noRNN_S143n": _cfg(with_rnn=False, size_s=143, with_acc_sum=False),
    "R256_S143n": _cfg(rnn_hid_size=256, size_s=143, with_acc_sum=False),
})
WSEED = 5
SHAPES = [(3, 40), (17, 23), (5, 37)]      # (5, 37): a partly filled 4x4x1 tail block in every hybrid kernel and in win_gemm_kernel

# one model per (configuration, past-state dropout), shared by every case of the file; the weights are never changed
_models = {}


def _model(name, p_state=0.0):
    if (name, p_state) not in _models:
        _models[(name, p_state)] = _train_model(TABLE[name], WSEED, 0.0, p_state)
    return _models[(name, p_state)]


def _rel(a, b):
    return np.linalg.norm(a.astype(np.float64) - b) / (np.linalg.norm(b) + 1e-30)


def _case(name, B, T, p_enc=0.0, p_state=0.0, input_grads=False, depth=False):
    cfg = TABLE[name]
    L, S = cfg["tf_layers"], cfg["size_s"]
    m, w = _model(name, p_state)
    m.ENCODER_DROPOUT = p_enc
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=60 + B + T)
    assert x_s.shape[2] == S and x_imu.shape[2] + S == w["in_linear.weight"].shape[1]
    cot = cotangent(cfg, B, T, 9 + B)
    seed = 20261020 + 31 * B + T
    y, g, ex = _step(m, x_imu, x_s, cot, seed, input_grads=input_grads)
    assert y.shape == (B, T, S) and len(g) == n_tensors(cfg) == (8 if cfg["with_rnn"] else 4) + 12 * L
    gates = _gates(m, cfg, B, T)
    mask, scale = _keep_mask(m, x_s, seed)
    out = train_oracle.step(cfg, w, x_imu, x_s, cot, keep_mask=mask, keep_scale=scale, p_drop=p_enc, seed=seed, relu_gates=gates,
                            input_grads=input_grads)
    yo, go = out[0], out[1]
    ey = float(np.abs(y - yo).max())
    note = ""
    if input_grads:
        dxi_o, dxs_o = out[2]
        assert ex["dx_imu"].shape == x_imu.shape and ex["dx_s"].shape == (B, T, S)
        # the last state column is a visible part of d x_s (2.4 .. 3.3 in norm): an input gradient that stops a column early is > REL.
        # (S = 111 has no SBP columns: its last three are the root velocity, whose gradient is zero by :75 — the column before them)
        last = np.linalg.norm(dxs_o[..., S - 1 if S > 111 else 107])
        assert last > 0.5 and last / np.linalg.norm(dxs_o) > 1e-2, (last, np.linalg.norm(dxs_o))
        ei, es = _rel(ex["dx_imu"], dxi_o), _rel(ex["dx_s"], dxs_o)
        note = f", dx_imu {ei:.2e}, dx_s {es:.2e} (|last column| {last:.2f})"
    if depth:
        # the oracle of the model WITHOUT its last layer is far in the tensors both have: a layer loop that stops early is visible
        last_layer = f"tf_encode.layers.{L - 1}."
        w1 = type(w)((k, v) for k, v in w.items() if not k.startswith(last_layer))
        assert len(w1) == len(w) - 12
        _, go1 = train_oracle.step(dict(cfg, tf_layers=L - 1), w1, x_imu, x_s, cot, keep_mask=mask, keep_scale=scale, p_drop=p_enc,
                                   seed=seed, relu_gates=gates[:L - 1])
        far = _rel_all(g, go1)
        note += f", without the last layer {far:.2e}"
    # (figures first: a failing case prints what it measured)
    errs = {n: _rel(g[n], ref) for n, ref in go.items()}
    wn = max(errs, key=errs.get)
    print(f"train paper-width {name} B={B} T={T} p_enc={p_enc} p_state={p_state}: max|dy| {ey:.2e}, worst tensor {wn} {errs[wn]:.2e}{note}")
    assert ey < YTOL, ey
    _check_grads(g, go)
    if input_grads:
        assert ei < REL and es < REL, (ei, es)
        nan = np.isnan(x_s)
        assert (ex["dx_s"][nan] == 0).all() and (ex["dx_s"][..., 108:111] == 0).all()
    if depth:
        assert far > 1e-3, far
    y2, g2, ex2 = _step(m, x_imu, x_s, cot, seed, input_grads=input_grads)
    assert np.array_equal(y, y2) and all(np.array_equal(g[n], g2[n]) for n in g), "the step does not repeat its bits"
    if input_grads:
        assert np.array_equal(ex["dx_imu"], ex2["dx_imu"]) and np.array_equal(ex["dx_s"], ex2["dx_s"])
    m.check_handoffs()
    return ey, (wn, errs[wn])


# ---- a. depth, fused path ------------------------------------------------------------------------------------------------------------
# The fused forward's layer loop over the image (fused_ih_off = LAYER0 + L * LAYER_FLOATS), the gate bits behind t.hid of every layer,
# lnwin sized L * B * (9 D + F).  tip_train_backward: col_multi = fbwd && 2 L + 3 <= kColMulti (16) — true up to L = 6, which fills 15 of
# the 16 ColSrc slots (colreduce_multi_kernel, grid y = 15); from L = 7 the fused backward reduces each layer's partials with its own
# two colreduce launches and the three batch-wide bias sums by colsum's own second stage.  train_supported: 4 L + 2 <= kMaxTr (64) —
# L = 15 is the last depth served.

@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("name", DEPTHS)
def test_depth_on_the_fused_path(name, B, T):
    _case(name, B, T, depth=True)


@pytest.mark.parametrize("input_grads", [False, True])
@pytest.mark.parametrize("name", ["L6", "L7", "L15"])       # either side of col_multi's edge and the last supported depth
def test_depth_at_1600_rows(name, input_grads):
    """(40, 40): 1 600 rows — more than one row block of every weight-gradient launch — without and with tip_train_input_grads behind
    the backward (input_grads_kernel at the paper's In = 221)."""
    _case(name, 40, 40, input_grads=input_grads, depth=True)


@pytest.mark.parametrize("name", ["L7", "L2"])
def test_depth_with_live_encoder_dropout(name):
    """Encoder dropout 0.1: the gate bits of every layer and ffn_bwd_kernel's gate_scale = 1 / (1 - p) — at L = 7 WITHOUT col_multi (the
    per-layer colreduce launches), at L = 2 with it (7 of 16 sources)."""
    _case(name, 5, 40, p_enc=0.1, depth=True)


def test_depth_with_past_state_dropout():
    """Past-state dropout 0.8 (train_model.py's default) at L = 7: the keep mask reaches the fused forward's prologue."""
    ey, worst = _case("L7", 3, 40, p_state=0.8, depth=True)
    m, _ = _model("L7", 0.8)
    x_s = synth.make_inputs(TABLE["L7"], 3, 40, seed=60 + 43)[1]
    mask, scale = _keep_mask(m, x_s, 20261020 + 31 * 3 + 40)
    assert 0.1 < mask.mean() < 0.3 and scale == pytest.approx(5.0)


# ---- b. state and input width, four layers -------------------------------------------------------------------------------------------
# win_gemm_shapes: 128 < S <= 144 allocates wih_tf / wout_tf / wout_f; win_g needs wout_tf, Sp = round_up(S, 16) <= 160, Sp % 4 == 0.
#   S135n / S139n / S143n: win_gemm_kernel<4, 10> for dH with kvalid = Sp = 144 of K = 160 on a wout_tf packed [R][160] from an S-row weight,
#     win_gemm_kernel<2, 32> for d_enc; the forward's head: launch_head_ksplit refuses S >= 132 -> tgemm16_launch after hipErrorInvalidValue.
#   S147n / S151n (Sp = 160) and S111 / S115 / S127 (Sp = 112 / 128): no wout_tf — tgemm16 for dH, lin_launch for d_enc.
# grad_weight for dW_out: n_rows_pad = Sp, n_store = S (the split tgemm with a cropped store); colpart_out = kColZ * round_up(S, 64)
# changes at S > 128; colreduce_multi_kernel's grid x covers (S + 63) / 64.  The input side: prep_in / u_in_kernel (InPad == 224) /
# finish_in_kernel / input_grads_kernel at In = 201 .. 223 — In = 223 (S151n) leaves ONE pad column.

@pytest.mark.parametrize("B,T", SHAPES + [(1, 1), (40, 40)])
@pytest.mark.parametrize("name", WIDTHS)
def test_state_and_input_width(name, B, T):
    _case(name, B, T, input_grads=(B, T) in ((3, 40), (5, 37)))      # d x_s has S columns: input_grads_kernel's In .. InPad padding


@pytest.mark.parametrize("name", ["S143n", "S151n"])
def test_state_width_with_live_encoder_dropout(name):
    _case(name, 5, 40, p_enc=0.1)


@pytest.mark.parametrize("name", ["S143n", "S127"])
def test_state_width_at_257_windows_sparse(name):
    """B = 257 > 256 CUs: the grid-stride second round of win_gemm_kernel (win += gridDim.x; S143n) and the split dW_out over 10 280 rows
    off S = 131; a sparse cotangent, the oracle on <= 10 windows, and _sparse_case's own lost-window assertion."""
    m, worst = _sparse_case(TABLE[name], 257, 40, 0.0, WSEED)
    m.check_handoffs()


# ---- c. both axes, and the family's edge ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B,T,ig", [
    ("L2_S143n", 17, 23, False), ("L2_S143n", 40, 40, False),    # col_multi at 7 sources with the 143-column output sums; win_gemm at L = 2
    ("L7_S127", 5, 37, False),                                   # no col_multi, no wout_tf
    # In = 225 / 233 > 224: outside fused_supported — layer by layer (prep_in_kernel, transpose_batch_kernel, launch_prologue with
    # another InPad), which is NOT the composite
    ("S135", 3, 40, True), ("S135", 17, 23, True), ("S143", 3, 40, True), ("S143", 17, 23, True),
    # no RNN: bwd_d_enc = tgemm16 on dyp [M][Sp] at Sp = 144 / 112, fbwd without the per-window kernels (4 + 12 L tensors)
    ("noRNN_S143n", 5, 40, False), ("noRNN_L1_S111", 5, 40, False),
    ("R256_S143n", 5, 37, False),                                # another RNN width: no fused forward, K = 256 head, fbwd
])
def test_both_axes_and_the_edge_of_the_family(name, B, T, ig):
    _case(name, B, T, input_grads=ig, depth=TABLE[name]["tf_layers"] != 4)


# ---- d. the depth limit --------------------------------------------------------------------------------------------------------------

def test_sixteen_layers_fall_back_to_the_composite():
    """train_supported: 4 * 16 + 2 > kMaxTr — tip_train_bytes refuses, the module says so and differentiates its torch-op composite,
    which still meets the oracle (bounds of test_unsupported_configuration_falls_back_to_the_composite: 2e-5 on y, 1e-3 per tensor).
    The oracle differentiates the ReLU piece the composite was on (its F.relu calls are recorded), as for every HIP step here: at 16
    layers and 122 880 hidden units per layer the fp32 run and the fp64 oracle otherwise disagree on a handful of units whose
    pre-activation rounds to either side of zero — one such unit is 5.3e-3 of layer 0's dW1 — which says nothing about the composite."""
    import torch.nn.functional as F
    from unittest import mock
    cfg = TABLE["L16"]
    m, w = _model("L16")
    B, T = 3, 40
    with pytest.raises(tlib.TipStatusError) as ei:
        m._ensure_handle().train_bytes(B, T)
    assert ei.value.status == tlib.TIP_ERR_UNSUPPORTED_CONFIG
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=2)
    cot = cotangent(cfg, B, T, 3)
    m.zero_grad(set_to_none=True)
    gates, relu = [], F.relu

    def recording_relu(f, *a, **kw):
        out = relu(f, *a, **kw)
        gates.append((out.detach() > 0).cpu().numpy())
        return out

    n0 = m.hip_forward_count()
    with mock.patch.object(F, "relu", recording_relu), pytest.warns(UserWarning, match="torch-op training composite"):
        y = m(torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda())
    assert m.hip_forward_count() == n0 and not type(y.grad_fn).__name__.startswith("_HipTrainFunction")
    assert len(gates) == 16 and gates[0].shape == (B, T, cfg["tf_hid_size"])
    (y * torch.tensor(cot).cuda()).sum().backward()
    yo, go = train_oracle.step(cfg, w, x_imu, x_s, cot, relu_gates=gates)
    assert len(go) == 8 + 12 * 16
    ey = np.abs(y.detach().cpu().numpy() - yo).max()
    errs = {n: _rel(p.grad.cpu().numpy(), go[n]) for n, p in m.named_parameters()}
    wn = max(errs, key=errs.get)
    print(f"train paper-width L16 (composite) B={B} T={T}: max|dy| {ey:.2e}, worst tensor {wn} {errs[wn]:.2e}")
    assert ey < 2e-5 and errs[wn] < 1e-3, (ey, wn, errs[wn])


def test_fifteen_layers_do_not_warn():
    """L = 15: 62 of the 64 transposes — the last depth on the HIP step, and it says nothing."""
    cfg = TABLE["L15"]
    m, _ = _model("L15")
    saved, scratch = m._ensure_handle().train_bytes(3, 40)
    assert saved > 0 and scratch > 0
    x_imu, x_s = synth.make_inputs(cfg, 3, 40, seed=2)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        y, g, _ = _hip_step(m, x_imu, x_s, cotangent(cfg, 3, 40, 3))       # (asserts _HipTrainFunction and the forward count)
    assert not [str(r.message) for r in rec if "torch-op training composite" in str(r.message)]
    assert len(g) == 8 + 12 * 15 and all(np.isfinite(v).all() for v in g.values())


# ---- e. the fp64 step (csrc/tip_f64.hip) ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B,T", [("L7", 5, 37), ("S143n", 17, 23)])
def test_f64_step(name, B, T):
    """A module built under --double, as test_f64_step_sparse runs it (rel 1e-11, ytol 1e-11), with a dense cotangent: seven layers
    (kMaxLayersF64 = 16 serves them) and 143 state columns on 215 input columns."""
    cfg = TABLE[name]
    m = make_model(cfg)
    w = load_synth(m, cfg, WSEED)
    m = m.double().cuda().train()
    m.ENCODER_DROPOUT = 0.0
    saved, scratch = m._ensure_handle().train_bytes(B, T, fp64=True)          # tip_train_bytes_f64 serves the configuration
    assert saved > 0 and scratch > 0
    x_imu, x_s = (a.astype(np.float64) for a in synth.make_inputs(cfg, B, T, seed=60 + B + T))
    cot = cotangent(cfg, B, T, 9 + B).astype(np.float64)
    y, g, _ = _step(m, x_imu, x_s, cot, 77)
    assert y.dtype == np.float64 and len(g) == n_tensors(cfg)
    yo, go = train_oracle.step(cfg, w, x_imu, x_s, cot)
    ey = float(np.abs(y - yo).max())
    errs = {n: _rel(g[n], ref) for n, ref in go.items()}
    wn = max(errs, key=errs.get)
    print(f"train paper-width fp64 {name} B={B} T={T}: max|dy| {ey:.2e}, worst tensor {wn} {errs[wn]:.2e}")
    assert ey < 1e-11, ey
    _check_grads(g, go, 1e-11)
    y2, g2, _ = _step(m, x_imu, x_s, cot, 77)
    assert np.array_equal(y, y2) and all(np.array_equal(g[n], g2[n]) for n in g)
    m.check_handoffs()
