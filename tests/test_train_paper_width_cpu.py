"""The training step OFF the paper model, without a GPU: the table of tests/test_train_paper_width_gpu.py (the paper-width family of
csrc/tip_fused.hip, fused_supported, with tf_layers / size_s / with_acc_sum moved off the paper's values) and the premises that file's
bounds rest on, from oracle/train_oracle.py alone:
  * the table's input widths and the number of gradient tensors per depth;
  * a dropped output column shows: zeroing the cotangent's last column moves the whole gradient set, and the last row of dW_out
    carries a visible share of its norm, at every state width of the table;
  * the bounds need no widening with depth or width: the oracle's own fp32 form stays a third under REL (and a third under 2e-5 for
    y) of its fp64 form on the same ReLU piece at 1 .. 15 layers and at the widest state."""
import numpy as np
import pytest
import torch

from tip_amd import synth
from oracle import train_oracle
from test_paper_width_schedule_cpu import CONFIGS, in_columns
from test_train_gpu import REL
from test_train_regimes_gpu import _rel_all

YTOL = 2e-5          # tests/test_train_gpu.py: y of a step against the fp64 oracle


def _cfg(**kw):
    return dict(synth.PAPER, **kw)


# what the training tests add to CONFIGS of tests/test_paper_width_schedule_cpu.py ("n": with_acc_sum = False)
LOCAL = {
    "L6": _cfg(tf_layers=6), "L15": _cfg(tf_layers=15), "L16": _cfg(tf_layers=16),
    "S135n": _cfg(size_s=135, with_acc_sum=False), "S139n": _cfg(size_s=139, with_acc_sum=False), "S115": _cfg(size_s=115),
}
TABLE = dict(CONFIGS, **LOCAL)
WIDTHS = ["S111", "S115", "S127", "S135n", "S139n", "S143n", "S147n", "S151n"]      # section b of the GPU file: four layers, fused
DEPTHS = ["L1", "L2", "L6", "L7", "L8", "L12", "L15"]                                # section a


def n_tensors(cfg):
    return (8 if cfg.get("with_rnn", True) else 4) + 12 * cfg["tf_layers"]


def cotangent(cfg, B, T, seed):
    return synth.normal(seed, "cot", B * T * cfg["size_s"]).reshape(B, T, -1).astype(np.float32)


def test_the_table_is_what_the_issue_says():
    names = WIDTHS + ["S135", "S143"]
    assert [in_columns(TABLE[n]) for n in names] == [201, 205, 217, 207, 211, 215, 219, 223, 225, 233]
    for n in names:
        assert (TABLE[n]["size_s"] - 111) % 4 == 0, n          # synth.make_inputs: whole SBPs only
    assert [n for n in names if in_columns(TABLE[n]) > 224] == ["S135", "S143"]      # csrc/tip_fused.hip, fz::KIN
    assert [TABLE[n]["tf_layers"] for n in DEPTHS + ["L16"]] == [1, 2, 6, 7, 8, 12, 15, 16]
    assert set(LOCAL).isdisjoint(CONFIGS)


@pytest.mark.parametrize("name", DEPTHS + ["L16", "S143n", "noRNN", "noRNN_L1_S111"])
def test_gradient_tensor_counts(name):
    cfg = TABLE[name]
    lay = synth.state_dict_layout(cfg)
    assert len(lay) == n_tensors(cfg) == (8 if cfg["with_rnn"] else 4) + 12 * cfg["tf_layers"]
    assert lay["linear.weight"] == (cfg["size_s"], cfg["rnn_hid_size"] if cfg["with_rnn"] else cfg["tf_in_dim"])
    assert lay["in_linear.weight"] == (256, in_columns(cfg))


@pytest.mark.parametrize("name", WIDTHS)
def test_a_dropped_output_column_moves_the_gradients(name):
    """Premises of the GPU file's width cases.  (1) The oracle's gradient set with the cotangent's last column zeroed is > 1e-2
    (relative L2 over all tensors; measured 6.2e-2 .. 9.9e-2) from the full one: a backward that never reads column S - 1 of dy (or a
    forward that never writes it) cannot pass REL = 1e-5.  (2) The last row of dW_out carries > 1e-2 of that tensor's norm (measured
    6.2 .. 10.1 %): a cropped store that stops a row early cannot pass either."""
    cfg = TABLE[name]
    B, T = 3, 40
    w = synth.make_weights(cfg, seed=5)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=60 + B)
    cot = cotangent(cfg, B, T, 9)
    gates = []
    _, go = train_oracle.step(cfg, w, x_imu, x_s, cot, gates_out=gates)
    cot0 = cot.copy()
    cot0[..., -1] = 0.0
    _, g0 = train_oracle.step(cfg, w, x_imu, x_s, cot0, relu_gates=gates)
    moved = _rel_all(g0, go)
    dW = go["linear.weight"]
    assert dW.shape[0] == cfg["size_s"]
    share = np.linalg.norm(dW[-1]) / np.linalg.norm(dW)
    print(f"{name}: last cotangent column zeroed moves the gradients by {moved:.2e}; last row of dW_out / dW_out = {share:.2e}")
    assert moved > 1e-2 and share > 1e-2, (name, moved, share)


@pytest.mark.parametrize("name", ["L1", "L7", "L12", "L15", "S143n", "S151n"])
def test_the_oracles_own_fp32_form_leaves_the_bounds_their_margin(name):
    """train_oracle.step in fp32 against fp64 on the ReLU piece the fp32 run was on, B = 17, T = 40: every tensor under REL / 3 and
    |dy| under 2e-5 / 3 (measured 7.4e-7 .. 9.3e-7 for the worst tensor, |dy| <= 9.6e-7: the usual 10 x).  The reference's own rounding does
    not grow with depth or state width, so a GPU case over REL is a finding, not a tolerance to raise."""
    cfg = TABLE[name]
    B, T = 17, 40
    w = synth.make_weights(cfg, seed=5)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=60 + B)
    cot = cotangent(cfg, B, T, 9)
    gates = []
    y32, g32 = train_oracle.step(cfg, w, x_imu, x_s, cot, dtype=torch.float32, gates_out=gates)
    assert len(gates) == cfg["tf_layers"] and gates[0].shape == (B, T, cfg["tf_hid_size"])
    y64, g64 = train_oracle.step(cfg, w, x_imu, x_s, cot, relu_gates=gates)
    assert len(g64) == n_tensors(cfg)
    worst = ("", 0.0)
    for n, ref in g64.items():
        err = np.linalg.norm(g32[n].astype(np.float64) - ref) / (np.linalg.norm(ref) + 1e-30)
        worst = max(worst, (n, err), key=lambda p: p[1])
    dy = np.abs(y32 - y64).max()
    print(f"{name}: fp32 oracle vs fp64 oracle, |dy| {dy:.2e}, worst tensor {worst[0]} {worst[1]:.2e}")
    assert worst[1] < REL / 3, worst
    assert dy < YTOL / 3, dy
