#!/usr/bin/env python3
"""Golden traces of the REFERENCE streaming runner at other window lengths: RTRunnerMin(char, model, max_input_l = W, ...)
(real_time_runner_minimal.py:24,54,131,139) for W in {1, 7, 24, 41, 64} — one-slot rings, between the 6-tap output filter and the
11-tap smoother, an acc-sum over fewer than ACC_SUM_WIN_LEN = 40 rows, one past 40, and an acc-sum over the newest 40 rows of a longer
window.  One stream per length, F = 2 W + 16 frames: every ring wraps twice and the output filter is primed.

Runs only in the build container, with the stubs, the kinematic character and the synthetic IMU frames of make_runner_golden.py
(imported, not copied); the model is the reference TF_RNN_Past_State with the build's synthetic weights (seed 0), dropout off, .eval(),
with_acc_sum, five stationary body points.  IMU seed 3, s_init from RandomState(103) as make_runner_golden.py draws it.

Written to tests/golden/tip_runner_window_golden.npz, data only, per length under "w<W>/": the raw frames (float64), every call's
newest x_imu / x_s / y row, qdq[3:] and ct per frame (float32), and the full windows of two calls — the first sliding call (call W)
and the last one.  oracle/streaming_oracle.py:StreamOracle(max_len=W), pinned to this file by tests/test_stream_window_cpu.py, carries
every other length.

usage: python tests/golden/make_runner_window_golden.py [--real-fairmotion]
"""
import os
import sys

import numpy as np
import torch

from make_runner_golden import HERE, REF, FakeChar, install_stubs, smooth_imu_sequence

WINDOWS = (1, 7, 24, 41, 64)


def main():
    real = "--real-fairmotion" in sys.argv
    install_stubs(real)
    sys.path.insert(0, REF)
    impl = "fairmotion (installed package)" if real else "scipy stand-in (fairmotion fork absent: parity UNPINNED for A2R / R2A conventions)"
    import tip_amd  # noqa: F401
    from tip_amd import synth
    import amass_char_info
    from simple_transformer_with_state import TF_RNN_Past_State
    from real_time_runner_minimal import RTRunnerMin

    torch.Tensor.cuda = lambda self, *a, **k: self      # harness only
    w = synth.make_weights(synth.PAPER, seed=0)
    model = TF_RNN_Past_State(72, 131, rnn_hid_size=512, tf_hid_size=1024, tf_in_dim=256, n_heads=16, tf_layers=4,
                              dropout=0.0, in_dropout=0.0, past_state_dropout=0.0, with_acc_sum=True)
    model.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    model.eval()

    calls = []
    orig_forward = model.forward

    def tapped(x_imu, x_s):
        y = orig_forward(x_imu, x_s)
        calls.append((x_imu.numpy().copy(), x_s.numpy().copy(), y.detach().numpy().copy()))
        return y

    model.forward = tapped

    seed = 3
    rng = np.random.RandomState(100 + seed)
    s_init = np.zeros(114)
    s_init[3:57] = rng.randn(54) * 0.3          # root + 17 joint axis-angles
    s_init[2] = 0.95
    out = {"s_init": s_init, "windows": np.array(WINDOWS)}
    for W in WINDOWS:
        n_frames = 2 * W + 16
        runner = RTRunnerMin(FakeChar(amass_char_info), model, W, s_init.copy(), with_acc_sum=True)
        raw = smooth_imu_sequence(n_frames, seed)
        calls.clear()
        qdq, ct = [], []
        root = np.array([0.0, 0.0, 0.95])
        for t in range(n_frames):
            res = runner.step(raw[t], root)
            root = res["qdq"][:3]
            qdq.append(res["qdq"][3:].copy())
            ct.append(res["ct"].copy())
        tag = f"w{W}"
        f32 = np.float32
        out[tag + "/raw_imu"] = raw
        out[tag + "/qdq_rest"] = np.array(qdq, dtype=f32)
        out[tag + "/ct"] = np.array(ct, dtype=f32)
        out[tag + "/call_T"] = np.array([c[0].shape[1] for c in calls])
        for k in (W, len(calls) - 1):
            out[f"{tag}/x_imu_call{k}"] = calls[k][0][0].astype(f32)
            out[f"{tag}/x_s_call{k}"] = calls[k][1][0].astype(f32)
        out[tag + "/x_imu_last_rows"] = np.array([c[0][0, -1] for c in calls], dtype=f32)
        out[tag + "/x_s_last_rows"] = np.array([c[1][0, -1] for c in calls], dtype=f32)
        out[tag + "/y_last_rows"] = np.array([c[2][0, -1] for c in calls], dtype=f32)
        print(tag, "frames", n_frames, "model calls", len(calls), "T:", out[tag + "/call_T"][:8], "...")
    out["conversions_impl"] = np.frombuffer(impl.encode(), dtype=np.uint8).copy()
    path = os.path.join(HERE, "tip_runner_window_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
