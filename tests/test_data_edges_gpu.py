"""GPU: the train-set combiner and the window gather (csrc/tip_data.hip) against oracle/data_oracle.py at the boundaries their
tiling creates: sequence lengths around the accepted minimum and around the 128-frame (combine_imu_kernel) and 256-frame
(acc_sum_kernel) workgroup tiles, root orientations that are not exact rotations (the hand-written 3x3 inverse), axis-angles at
zero, around the small-angle threshold, at pi and past one turn, and windows at both legal ends of the combined arrays.
Every element is compared; NaN positions are compared separately."""
import functools
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from make_data_golden import synth_motion                                    # noqa: E402
import tip_amd                                                                # noqa: E402
from oracle import data_oracle                                                # noqa: E402
from test_data_oracle import check_rotvec_fixture, rotvec_edge_motion         # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 2e-6        # as test_data_gpu.py: fp64 math on both sides, one float32 rounding
TOL_ROT = 1.2e-7  # rotation-matrix entries are at most 1 in magnitude: one float32 ulp there is at most 2^-23 = 1.19e-7
SENTINEL = -777.25


@functools.lru_cache(maxsize=None)
def _motion(L, seed):
    return synth_motion(L, seed)


def motion(m, variant, seed):
    """A synthetic file with min(L_imu, L_s) = m: "equal", or one more imu row ("imu_longer"), or one more qdq row ("s_longer")."""
    imu, s, c = (a.copy() for a in _motion(m + 1, seed))
    if variant == "equal":
        return imu[:m], s[:m], c[:m]
    if variant == "imu_longer":
        return imu, s[:m], c[:m]
    assert variant == "s_longer"
    return imu[:m], s, c


def as_file(imu, s, c):
    return {"imu": imu, "nimble_qdq": s, "constrs": c}


def check_rows(tag, IMU, SUM, S, imu, s, c, bias, nan_root_vel):
    """Rows the combiner wrote for one file against the oracle: every element, NaN positions apart."""
    a, b, cc = data_oracle.combine_sequence(imu, s, c, bias, nan_root_vel=nan_root_vel)
    assert IMU.shape == a.shape and SUM.shape == b.shape and S.shape == cc.shape, tag
    assert not np.isnan(IMU).any() and not np.isnan(SUM).any(), tag
    nan = np.zeros(S.shape, dtype=bool)
    nan[:, 108:111] = bool(nan_root_vel)                                     # columns 108..110 all NaN and nothing else is
    assert np.array_equal(np.isnan(cc), nan) and np.array_equal(np.isnan(S), nan), tag
    e_imu, e_sum = np.abs(IMU - a).max(), np.abs(SUM - b).max()
    e_rot = np.abs(S[:, :108] - cc[:, :108]).max()
    e_rest = np.nanmax(np.abs(S[:, 108:] - cc[:, 108:]))
    print(f"{tag}: frames {len(a)} max|IMU| {np.abs(a).max():.3g} err IMU {e_imu:.3g} SUM {e_sum:.3g} rot {e_rot:.3g} rest {e_rest:.3g}")
    assert e_imu < TOL, (tag, e_imu, np.unravel_index(np.abs(IMU - a).argmax(), a.shape))
    assert e_sum < TOL, (tag, e_sum, np.unravel_index(np.abs(SUM - b).argmax(), b.shape))
    assert e_rot <= TOL_ROT, (tag, e_rot, np.unravel_index(np.abs(S[:, :108] - cc[:, :108]).argmax(), (len(a), 108)))
    assert e_rest < TOL, (tag, e_rest)


def combine_and_check(tag, files, dip, rates=None):
    """combine_motions over accepted files [(imu, s, c)], each against the oracle; returns the info table."""
    rates = rates or list(range(2, 2 + len(files)))
    bias = np.linspace(-0.1, 0.1, 18 * len(files)).reshape(len(files), 18)
    cmb = tip_amd.data.combine_motions([as_file(*f) for f in files], rates, dip, biases=bias)
    IMU, SUM, S = (t.cpu().numpy() for t in (cmb.IMU, cmb.SUM, cmb.S))
    start = 0
    for k, (imu, s, c) in enumerate(files):
        n = min(len(imu), len(s)) - 8
        assert cmb.info[k].tolist() == [start, start + n, rates[k]], (tag, cmb.info)
        check_rows(f"{tag}[{k}]", IMU[start:start + n], SUM[start:start + n], S[start:start + n], imu, s, c, bias[k], dip[k])
        start += n
    assert len(cmb.info) == len(files) and len(IMU) == start
    return cmb.info


# L' = min(L) - 8 = 32 (refused) | 33 | 127 128 129 (one combine_imu_kernel tile +- 1) | 255 256 257 (one acc_sum_kernel tile
# +- 1) | 300
LENGTHS = (40, 41, 135, 136, 137, 263, 264, 265, 308)
LENGTH_CASES = [(m, "equal") for m in LENGTHS] + [(m, v) for m in (41, 137, 265) for v in ("imu_longer", "s_longer")]


@pytest.mark.parametrize("m,variant", LENGTH_CASES)
def test_lengths_around_the_minimum_and_the_workgroup_tiles(m, variant):
    """The same file twice in one call, as a plain file and as an augmented-DIP file (nan_root_vel = 1)."""
    assert torch.cuda.is_available()
    lib = tip_amd.lib.load()
    imu, s, c = motion(m, variant, 100 + m)
    assert min(len(imu), len(s)) == m
    n = lib.tip_combine_frames(len(imu), len(s))
    if m == 40:
        assert n == 0 and lib.tip_combine_frames(40, 41) == 0 and lib.tip_combine_frames(41, 40) == 0
        cmb = tip_amd.data.combine_motions([as_file(imu, s, c)] * 2, [3, 5], [False, True])
        assert cmb.IMU.shape == (0, 72) and cmb.SUM.shape == (0, 18) and cmb.S.shape == (0, 131) and cmb.info.shape == (0, 3)
        return
    assert n == m - 8
    info = combine_and_check(f"m{m}/{variant}", [(imu, s, c)] * 2, [False, True], rates=[3, 5])
    assert info.tolist() == [[0, n, 3], [n, 2 * n, 5]]


def test_refused_length_writes_nothing_through_the_c_abi():
    """min(L) = 40 is "too short": tip_combine_sequence returns 0 and leaves all three outputs (and the scratch) alone."""
    lib = tip_amd.lib.load()
    imu, s, c = _motion(41, 140)
    d_imu, d_s, d_c = (torch.tensor(a).cuda() for a in (imu, s, c))
    bias = torch.zeros(18, dtype=torch.float64, device="cuda")
    for L_imu, L_s in ((40, 40), (40, 41), (41, 40)):
        out = [torch.full((64, w), SENTINEL, dtype=torch.float32, device="cuda") for w in (72, 18, 131)]
        scratch = torch.full((64 * 18,), SENTINEL, dtype=torch.float64, device="cuda")
        rc = lib.tip_combine_sequence(d_imu.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), L_imu, L_s, bias.data_ptr(), 0,
                                      out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), scratch.data_ptr(),
                                      scratch.numel() * 8, None)
        torch.cuda.synchronize()
        assert rc == 0, (L_imu, L_s, rc)
        assert all(bool((t == SENTINEL).all()) for t in out + [scratch]), (L_imu, L_s)


def test_refused_file_between_two_accepted_ones():
    first, short, last = motion(41, "equal", 141), motion(40, "imu_longer", 142), motion(137, "s_longer", 143)
    files, rates, dip = [first, short, last], [2, 4, 6], [True, False, False]
    bias = np.linspace(-0.1, 0.1, 36).reshape(2, 18)                          # one row per KEPT file
    cmb = tip_amd.data.combine_motions([as_file(*f) for f in files], rates, dip, biases=bias)
    assert cmb.info.tolist() == [[0, 33, 2], [33, 33 + 129, 6]]               # the second kept file starts where the first ends
    IMU, SUM, S = (t.cpu().numpy() for t in (cmb.IMU, cmb.SUM, cmb.S))
    assert len(IMU) == len(SUM) == len(S) == 162
    check_rows("mixed[0]", IMU[:33], SUM[:33], S[:33], *first, bias[0], True)
    check_rows("mixed[2]", IMU[33:], SUM[33:], S[33:], *last, bias[1], False)


def test_root_orientations_that_are_not_exact_rotations():
    """Real DIP readings are not exactly orthonormal: the root-local frame needs the true inverse (1 / det, every cofactor), which
    equals the transpose only on exact rotations.  137 kept frames: two combine_imu_kernel workgroups."""
    imu, s, c = motion(145, "equal", 7)
    rng = np.random.RandomState(5)
    L = len(imu)
    for off in (0, 9 + 9 * 2):                                                # the root and one of the five other sensors
        P = np.eye(3) + 0.05 * rng.standard_normal((L, 3, 3))
        imu[:, off:off + 9] = (imu[:, off:off + 9].reshape(L, 3, 3) @ P).reshape(L, 9)
    root = imu[4:-4, :9].reshape(-1, 3, 3)
    assert np.abs(np.linalg.det(root) - 1.0).max() > 0.05 and np.linalg.cond(root).max() < 2.0   # det != 1, well conditioned
    assert np.abs(np.linalg.inv(root) - root.transpose(0, 2, 1)).max() > 0.05                    # inverse != transpose
    combine_and_check("skewed", [(imu, s, c)] * 2, [False, True])


def test_rotation_vector_edges():
    """Norms 0, 1e-8, 9.99e-4, 1e-3, 1.001e-3, pi - 1e-9, pi, 2 pi - 0.01 and 3.5 pi on four axes, against scipy through the oracle."""
    imu, s, c, frames = rotvec_edge_motion()
    _, _, S_o = data_oracle.combine_sequence(imu, s, c, np.zeros(18))
    check_rotvec_fixture(s, frames, S_o)                                      # the fixture itself is sound (CPU)
    combine_and_check("rotvec", [(imu, s, c)] * 2, [False, True])


# ---- window gather -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def combined_arrays():
    """308 combined frames by the oracle: a plain file (160) and an augmented-DIP file (148, NaN root velocity)."""
    a = data_oracle.combine_sequence(*_motion(168, 11), np.linspace(-0.1, 0.1, 18))
    b = data_oracle.combine_sequence(*_motion(156, 12), np.linspace(0.1, -0.1, 18), nan_root_vel=True)
    IMU, SUM, S = (np.concatenate([x, y]) for x, y in zip(a, b))
    assert len(IMU) == 308 and np.isnan(S[160:, 108:111]).all() and not np.isnan(S[:160]).any()
    return IMU, SUM, S


def end_frames(T, n):
    """Both legal extremes (t = T reads row 0; t = n - 1 ends y on the last row), duplicates, an unsorted run, windows that
    straddle the NaN boundary at frame 160."""
    ends = [T, n - 1, T, 200, 150, 151, 150, n - 1, T + 1, 299, 160, 161, 159 + T // 2, n - 2]
    assert all(T <= t <= n - 1 for t in ends)
    return ends


@pytest.mark.parametrize("with_sum", [True, False])
@pytest.mark.parametrize("T", [1, 7, 40, 80])
def test_gather_is_a_bit_exact_copy_at_every_window_length(T, with_sum):
    IMU, SUM, S = combined_arrays()
    n = len(IMU)
    d_imu, d_sum, d_s = (torch.tensor(a).cuda() for a in (IMU, SUM, S))
    random.seed(0)
    ds = tip_amd.data.TrainSubDataset.from_arrays(T, [[0, 160, 1], [160, n, 1]], d_imu, d_s, IMU_sum=d_sum if with_sum else None,
                                                  with_acc_sum=with_sum)
    ends = end_frames(T, n)
    ds.ends = torch.tensor(ends, dtype=torch.int64, device="cuda")           # chosen end frames in place of the sampled ones
    x_imu, x_s, y = (t.cpu().numpy() for t in ds.batch(range(len(ends))))
    assert x_imu.shape == (len(ends), T, 90 if with_sum else 72) and x_s.shape == y.shape == (len(ends), T, 131)
    for k, t in enumerate(ends):
        o_imu, o_s, o_y = data_oracle.window(IMU, SUM if with_sum else None, S, t, T)
        assert np.array_equal(x_imu[k], o_imu), (k, t)
        for got, want in ((x_s[k], o_s), (y[k], o_y)):
            assert np.array_equal(np.isnan(got), np.isnan(want)), (k, t)
            assert np.array_equal(np.nan_to_num(got, nan=9.0), np.nan_to_num(want, nan=9.0)), (k, t)


@pytest.mark.parametrize("with_sum", [True, False])
@pytest.mark.parametrize("T", [1, 7])
def test_gather_writes_nothing_outside_its_outputs(T, with_sum):
    """tip_gather_windows through the C ABI into buffers with 131 guard floats in front and behind: the windows are complete and
    the guards untouched (the (T + 1) * 131 loop over the S rows must not run past x_s or in front of y)."""
    lib = tip_amd.lib.load()
    IMU, SUM, S = combined_arrays()
    n = len(IMU)
    d_imu, d_sum, d_s = (torch.tensor(a).cuda() for a in (IMU, SUM, S))
    ends = end_frames(T, n)
    t_idx = torch.tensor(ends, dtype=torch.int64, device="cuda")
    G, wi = 131, 90 if with_sum else 72
    bufs = [torch.full((G + len(ends) * T * w + G,), SENTINEL, dtype=torch.float32, device="cuda") for w in (wi, 131, 131)]
    rc = lib.tip_gather_windows(d_imu.data_ptr(), d_sum.data_ptr() if with_sum else None, d_s.data_ptr(), n, t_idx.data_ptr(),
                                len(ends), T, *(b.data_ptr() + 4 * G for b in bufs), None)
    torch.cuda.synchronize()
    assert rc == 0
    for b, w, pick in zip(bufs, (wi, 131, 131), range(3)):
        h = b.cpu().numpy()
        assert np.all(h[:G] == SENTINEL) and np.all(h[-G:] == SENTINEL), pick
        body = h[G:-G].reshape(len(ends), T, w)
        for k, t in enumerate(ends):
            want = data_oracle.window(IMU, SUM if with_sum else None, S, t, T)[pick]
            assert np.array_equal(np.isnan(body[k]), np.isnan(want)), (pick, k)
            assert np.array_equal(np.nan_to_num(body[k], nan=9.0), np.nan_to_num(want, nan=9.0)), (pick, k)
