"""Model shapes of the streaming front / back end, the part that needs no GPU: a numpy restatement of the reference's runners at the
four shapes (x_imu 72 | 90 columns: without | with acc-sum; state 119 | 131 columns: two | five stationary body points) and of
RTRunner's corrected history feedback, pinned against traces of the REAL runners (tests/golden/make_runner_shapes_golden.py ->
tests/golden/tip_runner_shapes_golden.npz); the new C-ABI symbols; the engines' shape validation.

ShapedOracle is what tests/test_stream_shapes_gpu.py holds the device kernels to where no trace exists."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT
from oracle.streaming_oracle import (ACC_SUM_SCALE, ACC_SUM_WIN, COEFF, N_DOFS, StreamOracle, aa_to_rot6d, imu_rotate_to_local,
                                     rot6d_to_aa)
from scipy.spatial.transform import Rotation

SHAPES_GOLDEN = os.path.join(ROOT, "tests", "golden", "tip_runner_shapes_golden.npz")
# tag -> (n_sbps, with_acc_sum): tests/golden/make_runner_shapes_golden.py
TAGS = {"min_noacc_5": (5, False), "full_noacc_2": (2, False), "full_acc_2": (2, True), "full_acc_5_ik": (5, True)}


class ShapedOracle(StreamOracle):
    """StreamOracle (RTRunnerMin, five SBPs, acc-sum) restated for RTRunner / RTRunnerMin at any of the four shapes
    (real_time_runner.py:279-332, 403-449, 495), plus the host's override of the fed-back pose (:483-495)."""

    def __init__(self, s_init, n_sbps=5, with_acc_sum=True, max_len=40):
        super().__init__(s_init, max_len)
        self.n_sbps, self.with_acc_sum = int(n_sbps), bool(with_acc_sum)
        self.hist = [np.concatenate([aa_to_rot6d(self.s_init[3:N_DOFS]), self.s_init[N_DOFS:N_DOFS + 3],
                                     np.zeros(self.n_sbps * 4)])]                     # :99, :298-305

    def build_inputs(self):
        """:413-426 -> (x_imu [T, 72 | 90], x_s [T, 119 | 131]) in float64."""
        in_imu = imu_rotate_to_local(np.array(self.smoothed[-self.max_len:]))
        x_imu = in_imu
        if self.with_acc_sum:                                                          # :416-423
            self.acc_sum.append(in_imu[-ACC_SUM_WIN:, 54:72].sum(axis=0))
            x_imu = np.concatenate([in_imu, np.array(self.acc_sum[-self.max_len:]) / ACC_SUM_SCALE], axis=1)
        x_s = np.array(self.hist[-x_imu.shape[0]:])
        self._root_R = in_imu[-1, :9].reshape(3, 3)
        return x_imu, x_s

    def consume(self, y_last):
        """:431-449, :307-332, :495 (without a correction: st_hist_copy = s_t)."""
        nc = self.n_sbps * 4
        self.outs.append(np.array(y_last, dtype=np.float32))                           # float32 row, decoded in place while < 6 rows
        if len(self.outs) >= len(COEFF):
            s = (np.array(self.outs[-len(COEFF):]) * COEFF[:, None]).sum(axis=0) / COEFF.sum()
        else:
            s = self.outs[-1]
        st, c_t = s[:-nc], s[-nc:]
        c_t[0::4] = (c_t[0::4] > 0.0) * 1.0                                            # :327-330
        c_t[1::4] /= 5.0
        c_t[2::4] /= 5.0
        c_t[3::4] /= 5.0
        st_aa = rot6d_to_aa(st[:-3])
        s_t = np.zeros(2 * N_DOFS)
        s_t[N_DOFS:N_DOFS + 3] = st[-3:]
        s_t[6:N_DOFS] = st_aa[3:]
        s_t[3:6] = Rotation.from_matrix(self._root_R).as_rotvec()
        if self.last_s is not None:
            s_t[6:] = (s_t[6:] + self.last_s[6:]) / 2.0
        self.last_s = s_t.copy()
        self.hist.append(np.concatenate([aa_to_rot6d(s_t[3:N_DOFS]), s_t[N_DOFS:N_DOFS + 3], c_t]))
        return s_t[3:], np.array(c_t, dtype=np.float64)

    def override(self, q_aa):
        """:483-495: the history row just appended takes its 108 pose columns from the host's corrected pose (st_hist_copy[3:57]);
        root velocity, c_t and last_s (the pose average) keep the uncorrected frame."""
        row = self.hist[-1].copy()
        row[:108] = aa_to_rot6d(np.asarray(q_aa, dtype=np.float64).reshape(54))
        self.hist[-1] = row


def load_traces():
    z = np.load(SHAPES_GOLDEN)
    out = {}
    for k in z.files:
        if "/" in k:
            tag, name = k.split("/")
            out.setdefault(tag, {})[name] = z[k]
    for tr in out.values():
        tr["raw_imu"], tr["s_init"] = z["raw_imu"], z["s_init"]                       # (shared by the four traces)
    return out


@pytest.fixture(scope="module")
def traces():
    return load_traces()


def test_fixture_protocol(traces):
    assert set(traces) == set(TAGS)
    assert os.path.getsize(SHAPES_GOLDEN) < 1 << 20
    for tag, (n_sbps, acc) in TAGS.items():
        tr = traces[tag]
        assert int(tr["n_calls"][0]) == 65 and tr["raw_imu"].shape == (70, 72)
        assert list(tr["call_T"][:40]) == list(range(1, 41)) and set(tr["call_T"][40:]) == {40}
        assert tr["x_imu_last_rows"].shape == (65, 90 if acc else 72)
        assert tr["x_s_last_rows"].shape == tr["y_last_rows"].shape == (65, 111 + 4 * n_sbps)
        assert tr["hist_last"].shape == (70, 111 + 4 * n_sbps) and tr["ct"].shape == (70, 4 * n_sbps)
    ik = traces["full_acc_5_ik"]
    assert ik["hist_q"].shape == (70, 54) and int(ik["hist_corrected"].sum()) >= 5     # the override trace is not vacuous
    for t in np.flatnonzero(ik["hist_corrected"]):
        assert np.abs(ik["hist_q"][t] - ik["qdq"][t][3:57]).max() > 0.0


@pytest.mark.parametrize("tag", list(TAGS))
def test_restatement_matches_reference_runners_teacher_forced(traces, tag):
    """The bounds of tests/test_streaming_oracle.py: 1e-5 on the float32 model inputs, 1e-9 on history rows and poses — the
    overridden history rows of full_acc_5_ik included."""
    tr = traces[tag]
    n_sbps, acc = TAGS[tag]
    o = ShapedOracle(tr["s_init"], n_sbps, acc)
    k = 0
    for t in range(70):
        if not o.ingest(tr["raw_imu"][t]):
            assert np.array_equal(tr["qdq"][t], tr["s_init"])
            continue
        x_imu, x_s = o.build_inputs()
        assert x_imu.shape == (tr["call_T"][k], 90 if acc else 72) and x_s.shape == (tr["call_T"][k], 111 + 4 * n_sbps)
        assert np.abs(x_imu[-1] - tr["x_imu_last_rows"][k]).max() < 1e-5
        assert np.abs(x_s[-1] - tr["x_s_last_rows"][k]).max() < 1e-5
        if f"x_imu_call{k}" in tr:
            assert np.abs(x_imu - tr[f"x_imu_call{k}"]).max() < 1e-5, (tag, k)
            assert np.abs(x_s - tr[f"x_s_call{k}"]).max() < 1e-5, (tag, k)
        s_rest, c_t = o.consume(tr["y_last_rows"][k])
        if "hist_q" in tr:
            if tr["hist_corrected"][t]:
                assert np.abs(np.array(o.hist[-1]) - tr["hist_last"][t]).max() > 1e-3   # without the override the row is wrong
            o.override(tr["hist_q"][t])
        assert np.abs(np.array(o.hist[-1]) - tr["hist_last"][t]).max() < 1e-9, (tag, t)
        assert np.abs(s_rest - tr["qdq"][t][3:]).max() < 1e-9
        assert np.array_equal(c_t, tr["ct"][t])
        k += 1
    assert k == 65


def test_new_symbols_are_declared_and_exported():
    from tip_amd import lib as tlib
    hdr = open(os.path.join(ROOT, "include", "tip_hip.h")).read()
    lib = ctypes.CDLL(tlib.LIB_PATH)
    for name in ("tip_stream_reset_shaped", "tip_stream_history_override"):
        assert re.search(r"TIP_API int " + name + r"\(", hdr), name
        assert name in tlib.EXPORTS and hasattr(lib, name), name
    assert int(re.search(r"#define TIP_ABI_VERSION (\d+)", hdr).group(1)) == 5
    # argument checks that run before any launch: no device needed
    L = tlib.load()
    buf = (ctypes.c_float * 4)()
    p = ctypes.addressof(buf)
    for n_sbps in (0, 1, 3, 4, 6):
        assert L.tip_stream_reset_shaped(p, p, 1, n_sbps, 1, None) == -1, n_sbps        # TIP_ERR_INVALID_ARG
    assert L.tip_stream_reset_shaped(None, p, 1, 2, 0, None) == -1
    assert L.tip_stream_reset_shaped(p, p, 0, 2, 0, None) == 0                           # nothing to do
    assert L.tip_stream_history_override(None, 1, p, p, 1, None) == -1
    assert L.tip_stream_history_override(p, 1, None, p, 1, None) == -1
    assert L.tip_stream_history_override(p, 1, p, None, 1, None) == -1
    assert L.tip_stream_history_override(p, 1, p, p, -1, None) == -1
    assert L.tip_stream_history_override(p, 1, None, None, 0, None) == 0
    nb5, nb2 = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.tip_stream_state_bytes(3, ctypes.byref(nb5)) == 0 and nb5.value == 3 * 10496 * 4   # the same for every shape


def test_engine_shape_validation_needs_no_device():
    """stream_shape() runs first in both engines' constructors: a model outside the four shapes is refused with a ValueError that names
    them, before anything touches a device."""
    from tip_amd import streaming

    def model(n_imu, size_s, acc):
        return types.SimpleNamespace(input_size_imu=n_imu, size_s=size_s, with_acc_sum=acc, training=False)

    assert streaming.stream_shape(model(72, 131, True)) == (5, True)
    assert streaming.stream_shape(model(72, 131, False)) == (5, False)
    assert streaming.stream_shape(model(72, 119, True)) == (2, True)
    assert streaming.stream_shape(model(72, 119, False)) == (2, False)
    for bad in (model(72, 123, True), model(60, 131, True), model(72, 111, False), model(90, 131, False)):
        with pytest.raises(ValueError) as e:
            streaming.stream_shape(bad)
        for a, b in streaming.SHAPES:
            assert f"{a} / {b}" in str(e.value)
        for cls in (streaming.StreamingEngine, streaming.StaggeredStreamingEngine):
            with pytest.raises(ValueError):
                cls(bad, np.zeros((1, 114), dtype=np.float32))
