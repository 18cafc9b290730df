#!/usr/bin/env python3
"""Golden traces of the REFERENCE streaming runners at the four model shapes the streaming engines serve (x_imu 72 / 90 columns:
without / with the acc-sum feature; state 119 / 131 columns: two / five stationary body points), and of RTRunner's IK-corrected
history feedback (real_time_runner.py:334-382, 483-495).

Runs only in the build container, like make_runner_golden.py, whose stubs (fairmotion -> scipy, a kinematic character for PyBullet,
torch.Tensor.cuda -> identity) and IMU sequence it imports; the reference's runners and model are imported as they are.  Only data
is written: tests/golden/tip_runner_shapes_golden.npz, one stream of 70 frames per tag (all four on the same raw IMU frames and
s_init, stored once):

    tag             runner                                                                     model                              x_imu / x_s
    min_noacc_5     RTRunnerMin(with_acc_sum=False)                                            synth.TRAIN_DEFAULT (8 heads)      72 / 131
    full_noacc_2    RTRunner(five_sbp=False, with_acc_sum=False)                               PAPER, size_s 119, no acc-sum      72 / 119
    full_acc_2      RTRunner(five_sbp=False, with_acc_sum=True)                                PAPER, size_s 119                  90 / 119
    full_acc_5_ik   RTRunner(five_sbp=True, with_acc_sum=True, multi_sbp_terrain_and_correction=True)   PAPER                     90 / 131

Per tag: raw IMU, s_init, the newest row of every model input, a few calls in full, the consumed output rows, qdq, ct, the history row
appended after every frame; for full_acc_5_ik also the corrected pose the runner fed back (st_hist_copy[3:57], per frame) and whether
it differs from the pose it returned (s_t[3:57]).  RTRunner(five_sbp=False, multi_sbp_terrain_and_correction=True) raises IndexError
inside the reference (real_time_runner.py:200), so it has no trace.

usage: python tests/golden/make_runner_shapes_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_runner_golden import REF, FakeChar, install_stubs, smooth_imu_sequence  # noqa: E402

N_FRAMES = 70
FULL_CALLS = (0, 1, 40)
MIN_CORRECTED_FRAMES = 5


def main():
    install_stubs(False)
    sys.path.insert(0, REF)
    import tip_amd  # noqa: F401
    from tip_amd import synth
    import amass_char_info
    import constants as cst
    from simple_transformer_with_state import TF_RNN_Past_State
    from real_time_runner import RTRunner
    from real_time_runner_minimal import RTRunnerMin

    torch.Tensor.cuda = lambda self, *a, **k: self      # harness only

    def full(five, acc, multi):
        return lambda char, model, s_init: RTRunner(char, model, 40, s_init, map_bound=cst.MAP_BOUND, grid_size=cst.GRID_SIZE,
                                                    five_sbp=five, with_acc_sum=acc, multi_sbp_terrain_and_correction=multi)

    traces = (
        ("min_noacc_5", dict(synth.TRAIN_DEFAULT), lambda char, model, s_init: RTRunnerMin(char, model, 40, s_init, with_acc_sum=False)),
        ("full_noacc_2", dict(synth.PAPER, size_s=119, with_acc_sum=False), full(False, False, False)),
        ("full_acc_2", dict(synth.PAPER, size_s=119), full(False, True, False)),
        ("full_acc_5_ik", dict(synth.PAPER), full(True, True, True)),
    )
    out = {}
    for tag, cfg, make_runner in traces:
        w = synth.make_weights(cfg, seed=0)
        model = TF_RNN_Past_State(cfg["input_size_imu"], cfg["size_s"], rnn_hid_size=cfg["rnn_hid_size"], tf_hid_size=cfg["tf_hid_size"],
                                  tf_in_dim=cfg["tf_in_dim"], n_heads=cfg["n_heads"], tf_layers=cfg["tf_layers"], dropout=0.0,
                                  in_dropout=0.0, past_state_dropout=0.0, with_acc_sum=cfg["with_acc_sum"])
        model.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
        model.eval()
        calls = []
        orig_forward = model.forward

        def tapped(x_imu, x_s, orig_forward=orig_forward, calls=calls):
            y = orig_forward(x_imu, x_s)
            calls.append((x_imu.numpy().copy(), x_s.numpy().copy(), y.detach().numpy().copy()))
            return y

        model.forward = tapped
        rng = np.random.RandomState(7)
        s_init = np.zeros(114)
        s_init[3:57] = rng.randn(54) * 0.3          # root + 17 joint axis-angles
        s_init[2] = 0.95
        runner = make_runner(FakeChar(amass_char_info), model, s_init)
        fed_back = []
        orig_record = runner.record_state_aa_and_c

        def record(cur_s, cur_c, orig_record=orig_record, fed_back=fed_back):
            fed_back.append(np.array(cur_s[3:57], dtype=np.float64))
            return orig_record(cur_s, cur_c)

        runner.record_state_aa_and_c = record       # (the constructor's own call, history row 0, is already behind us)
        raw = smooth_imu_sequence(N_FRAMES, 3)
        n_sbps = (cfg["size_s"] - 111) // 4
        qdq, ct, hist, hist_q, corrected = [], [], [], [], []
        root = np.array([0.0, 0.0, 0.95])
        for t in range(N_FRAMES):
            n_fed = len(fed_back)
            res = runner.step(raw[t], root) if isinstance(runner, RTRunnerMin) else runner.step(raw[t], root, t)
            root = res["qdq"][:3]
            qdq.append(np.array(res["qdq"], dtype=np.float64))
            ct.append(np.array(res["ct"], dtype=np.float64))
            row = np.array(runner.s_and_c_in_buffer[-1], dtype=np.float64)
            assert row.shape == (cfg["size_s"],) and np.isfinite(row).all(), (tag, t, row.shape)
            hist.append(row)
            if len(fed_back) > n_fed:               # a model frame: the pose the runner fed back, against the pose it returned
                hist_q.append(fed_back[-1])
                corrected.append(bool(np.abs(fed_back[-1] - res["qdq"][3:57]).max() > 0.0))
            else:                                   # priming frame: nothing fed back
                hist_q.append(np.array(res["qdq"][3:57], dtype=np.float64))
                corrected.append(False)
        assert len(calls) == N_FRAMES - 5 and calls[0][0].shape[2] == 72 + (18 if cfg["with_acc_sum"] else 0)
        assert calls[0][1].shape[2] == cfg["size_s"] and ct[-1].shape == (4 * n_sbps,)
        out["raw_imu"], out["s_init"] = raw, s_init            # the same 70 frames and initial state for every tag
        out[tag + "/qdq"] = np.array(qdq)
        out[tag + "/ct"] = np.array(ct)
        out[tag + "/hist_last"] = np.array(hist)
        out[tag + "/n_calls"] = np.array([len(calls)])
        out[tag + "/call_T"] = np.array([c[0].shape[1] for c in calls])
        for k in FULL_CALLS:
            out[f"{tag}/x_imu_call{k}"] = calls[k][0][0]
            out[f"{tag}/x_s_call{k}"] = calls[k][1][0]
        out[tag + "/x_imu_last_rows"] = np.array([c[0][0, -1] for c in calls])
        out[tag + "/x_s_last_rows"] = np.array([c[1][0, -1] for c in calls])
        out[tag + "/y_last_rows"] = np.array([c[2][0, -1] for c in calls])
        if tag.endswith("_ik"):
            out[tag + "/hist_q"] = np.array(hist_q)                  # st_hist_copy[3:57]: what a host passes to override_history
            out[tag + "/hist_corrected"] = np.array(corrected)
            dmax = max(np.abs(hist[t][:108] - _six(qdq[t][3:57])).max() for t in range(N_FRAMES) if corrected[t])
            print(tag, "frames whose fed-back pose was corrected:", int(np.sum(corrected)), "largest 6D difference: %.3f" % dmax)
            assert np.sum(corrected) >= MIN_CORRECTED_FRAMES, "the override trace must not be vacuous"
        else:
            assert not any(corrected), tag
        print(tag, "frames", N_FRAMES, "model calls", len(calls), "widths", calls[0][0].shape[2], calls[0][1].shape[2], ct[-1].shape[0])
    path = os.path.join(HERE, "tip_runner_shapes_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


def _six(aa):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(np.asarray(aa).reshape(-1, 3)).as_matrix()[:, :, :2].reshape(-1)


if __name__ == "__main__":
    main()
