"""CPU: the train-set combiner / window sampler oracle (oracle/data_oracle.py) against the output of the REAL reference
code (tests/golden/make_data_golden.py -> tip_data_golden.npz)."""
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from make_data_golden import motion_files, RATES, LENS   # noqa: E402  (synthetic motion generator: data, not reference code)
from oracle import data_oracle                             # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden", "tip_data_golden.npz")


def combined_by_oracle(z):
    """Run the oracle over the same files the reference combined; returns (IMU, SUM, S, info)."""
    IMU, SUM, S, info = [], [], [], []
    start, kept = 0, 0
    dnames = list(LENS.keys())
    for dname, i, imu, s, c in motion_files():
        m = min(len(s), len(imu))
        if m <= data_oracle.ACC_SUM_WIN_LEN:          # preprocess_and_combine_syn_amass.py:68-70
            continue
        a, b, cc = data_oracle.combine_sequence(imu, s, c, z["biases"][kept], nan_root_vel="DIP" in dname)
        kept += 1
        IMU.append(a); SUM.append(b); S.append(cc)
        info.append([start, start + len(a), RATES[dnames.index(dname)]])
        start += len(a)
    return np.concatenate(IMU), np.concatenate(SUM), np.concatenate(S), np.array(info)


def test_combiner_matches_reference():
    z = np.load(GOLD)
    IMU, SUM, S, info = combined_by_oracle(z)
    assert np.array_equal(info, z["info"])
    assert IMU.dtype == np.float32 and IMU.shape == z["IMU"].shape
    assert np.abs(IMU - z["IMU"]).max() < 2e-6          # fp64 math, fp32 storage: at most an ulp apart
    assert np.abs(SUM - z["SUM"]).max() < 2e-6
    assert np.array_equal(np.isnan(S), np.isnan(z["S"]))   # augmented-DIP root velocity is NaN (:61-62)
    assert np.nanmax(np.abs(S - z["S"])) < 2e-6


def test_window_sampler_matches_reference():
    z = np.load(GOLD)
    random.seed(99)
    ends = data_oracle.sample_ends(z["info"], 40)
    assert len(ends) == int(z["n_windows"][0])
    for k, t in enumerate(ends):
        x_imu, x_s, y = data_oracle.window(z["IMU"], z["SUM"], z["S"], t, 40)
        sums = [np.nansum(a.astype(np.float64)) for a in (x_imu, x_s, y)]
        assert np.allclose(sums, z["win/sums"][k], rtol=0, atol=1e-9), k
        if k < 3:
            assert np.array_equal(x_imu, z["win/x_imu"][k])
            assert np.array_equal(np.nan_to_num(x_s, nan=9.0), np.nan_to_num(z["win/x_s"][k], nan=9.0))
            assert np.array_equal(np.nan_to_num(y, nan=9.0), np.nan_to_num(z["win/y"][k], nan=9.0))


# ---- rotation-vector edges: a fixture shared with tests/test_data_edges_gpu.py ----------------------------------------------
# norms on both sides of scipy's small-angle threshold (1e-3: Taylor series below, sin(a/2)/a above), at and around pi (qw = 0)
# and past one turn; axes: two coordinate axes, an exactly representable-by-thirds direction and a general one
ROTVEC_NORMS = (0.0, 1e-8, 9.99e-4, 1e-3, 1.001e-3, np.pi - 1e-9, np.pi, 2 * np.pi - 0.01, 3.5 * np.pi)
ROTVEC_AXES = {0: np.array([1.0, 0.0, 0.0]), 5: np.array([0.0, 0.0, -1.0]), 11: np.array([1.0, 2.0, -2.0]) / 3.0,
               17: np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81])}


def rotvec_edge_motion():
    """(imu, s, c, frames): a 49-frame file (41 kept frames) whose kept frame frames[i] carries axis-angles of norm
    ROTVEC_NORMS[i] in the joints of ROTVEC_AXES."""
    from make_data_golden import synth_motion
    imu, s, c = synth_motion(49, 31)
    frames = [3 + 4 * i for i in range(len(ROTVEC_NORMS))]
    for f, n in zip(frames, ROTVEC_NORMS):
        for j, ax in ROTVEC_AXES.items():
            s[f + data_oracle.TRIM, 3 + 3 * j:6 + 3 * j] = n * ax
    return imu, s, c, frames


def check_rotvec_fixture(s, frames, S):
    """The oracle's rows of the edge frames are finite, and before the float32 store every 3x2 block has orthogonal unit columns."""
    assert np.isfinite(S[frames]).all()
    r = data_oracle.two_axis(s[data_oracle.TRIM:len(s) - data_oracle.TRIM, 3:57])[frames].reshape(len(frames), 18, 3, 2)
    a, b = r[..., 0], r[..., 1]
    assert np.abs((a * a).sum(-1) - 1.0).max() <= 1e-12 and np.abs((b * b).sum(-1) - 1.0).max() <= 1e-12
    assert np.abs((a * b).sum(-1)).max() <= 1e-12
    return r


def test_rotvec_edge_fixture_is_sound():
    imu, s, c, frames = rotvec_edge_motion()
    assert len(frames) == len(ROTVEC_NORMS) and max(frames) < len(s) - 2 * data_oracle.TRIM
    _, _, S = data_oracle.combine_sequence(imu, s, c, np.zeros(18))
    assert S.shape == (41, 131)
    r = check_rotvec_fixture(s, frames, S)
    eye = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])
    for j in ROTVEC_AXES:
        assert np.array_equal(r[0, j], eye)                                  # zero rotation vector: the identity, not 0/0
        assert np.abs(r[1, j] - eye).max() <= 2e-8                           # 1e-8 rad
        # Rodrigues' formula for the first two columns, written out: R = c I + s [k]x + (1 - c) k k^T
        for i, n in enumerate(ROTVEC_NORMS):
            k = ROTVEC_AXES[j]
            K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
            R = np.cos(n) * np.eye(3) + np.sin(n) * K + (1.0 - np.cos(n)) * np.outer(k, k)
            # (the angle is recomputed as |n k|: a few ulps of n = up to ~1e-14 rad at 3.5 pi, plus the arithmetic)
            assert np.abs(r[i, j] - R[:, :2]).max() <= 1e-13, (i, j)
