"""Window lengths other than 40 in the streaming front / back end, the part that needs no GPU: the oracle
(oracle/streaming_oracle.py: StreamOracle(max_len=W)) against traces of the REAL RTRunnerMin(char, model, max_input_l = W, ...)
(tests/golden/make_runner_window_golden.py -> tests/golden/tip_runner_window_golden.npz), the host side of the tip_stream_*_w family
and the engines' validation of `window`.  tests/test_stream_window_gpu.py holds the device kernels to the same file and oracle."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT
from oracle.streaming_oracle import StreamOracle

WINDOW_GOLDEN = os.path.join(ROOT, "tests", "golden", "tip_runner_window_golden.npz")
WINDOWS = (1, 7, 24, 41, 64)
INVALID_ARG = -1


def block_floats(W):
    """include/tip_hip.h: 11*72 + W*(72 + 18 + 131) + 6*131 + 54 + 3 floats, rounded up to 64."""
    return (11 * 72 + W * (72 + 18 + 131) + 6 * 131 + 54 + 3 + 63) // 64 * 64


def load_window_traces():
    z = np.load(WINDOW_GOLDEN)
    out = {}
    for k in z.files:
        if "/" in k:
            tag, name = k.split("/")
            out.setdefault(int(tag[1:]), {})[name] = z[k]
    for tr in out.values():
        tr["s_init"] = z["s_init"]
    return out


@pytest.fixture(scope="module")
def traces():
    return load_window_traces()


def test_fixture_protocol(traces):
    assert os.path.getsize(WINDOW_GOLDEN) <= 1000000
    assert tuple(sorted(traces)) == WINDOWS
    z = np.load(WINDOW_GOLDEN)
    assert bytes(z["conversions_impl"]) == bytes(np.load(os.path.join(ROOT, "tests", "golden", "tip_runner_golden.npz"))["conversions_impl"])
    for W, tr in traces.items():
        F = 2 * W + 16
        assert tr["raw_imu"].shape == (F, 72) and tr["raw_imu"].dtype == np.float64
        assert list(tr["call_T"]) == [min(k + 1, W) for k in range(F - 5)]
        assert tr["x_imu_last_rows"].shape == (F - 5, 90) and tr["x_s_last_rows"].shape == tr["y_last_rows"].shape == (F - 5, 131)
        assert tr["qdq_rest"].shape == (F, 111) and tr["ct"].shape == (F, 20)
        assert sorted(int(k[10:]) for k in tr if k.startswith("x_imu_call")) == [W, F - 6]
        for k in (W, F - 6):
            assert tr[f"x_imu_call{k}"].shape == (W, 90) and tr[f"x_s_call{k}"].shape == (W, 131)


@pytest.mark.parametrize("W", WINDOWS)
def test_oracle_matches_reference_runner_at_window(traces, W):
    """Teacher-forced with the reference model's own output rows.  The fixture stores float32: the model inputs are the runner's own
    float32 casts (1e-6; measured 2.4e-7), pose and c_t are float64 values rounded to float32 (1e-6 covers the rounding of |x| < 8;
    against the unrounded values the difference is 0)."""
    tr = traces[W]
    o = StreamOracle(tr["s_init"], max_len=W)
    k = 0
    for t in range(2 * W + 16):
        if not o.ingest(tr["raw_imu"][t]):
            assert np.abs(tr["qdq_rest"][t] - tr["s_init"][3:]).max() < 1e-6
            continue
        x_imu, x_s = o.build_inputs()
        assert x_imu.shape == (tr["call_T"][k], 90) and x_s.shape == (tr["call_T"][k], 131)
        assert np.abs(x_imu[-1] - tr["x_imu_last_rows"][k]).max() < 1e-6, (W, k)
        assert np.abs(x_s[-1] - tr["x_s_last_rows"][k]).max() < 1e-6, (W, k)
        if f"x_imu_call{k}" in tr:
            assert np.abs(x_imu - tr[f"x_imu_call{k}"]).max() < 1e-6, (W, k)
            assert np.abs(x_s - tr[f"x_s_call{k}"]).max() < 1e-6, (W, k)
        s_rest, c_t = o.consume(tr["y_last_rows"][k])
        assert np.abs(s_rest - tr["qdq_rest"][t]).max() < 1e-6, (W, t)
        assert np.array_equal(c_t[0::4], tr["ct"][t][0::4])
        assert np.abs(c_t - tr["ct"][t]).max() < 1e-6
        k += 1
    assert k == 2 * W + 11


def test_w_family_on_the_host():
    from tip_amd import lib as tlib
    L = tlib.load()
    assert L.tip_abi_version() == 5 == tlib.TIP_ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "tip_hip.h")).read()
    assert int(re.search(r"#define TIP_ABI_VERSION (\d+)", hdr).group(1)) == 5
    family = ["tip_stream_state_bytes_w", "tip_stream_window_len_w", "tip_stream_reset_w", "tip_stream_ingest_w", "tip_stream_consume_w",
              "tip_stream_attach_w", "tip_stream_detach_w", "tip_stream_ingest_staggered_w", "tip_stream_consume_staggered_w",
              "tip_stream_ingest_mapped_w", "tip_stream_consume_mapped_w", "tip_stream_history_override_w"]
    raw = ctypes.CDLL(tlib.LIB_PATH)
    for name in family:
        assert re.search(r"TIP_API int " + name + r"\(", hdr), name
        assert name in tlib.EXPORTS and hasattr(raw, name), name
    declared = set(re.findall(r"TIP_API\s+[\w\s\*]+?\b(tip_\w+)\s*\(", hdr))
    assert declared == set(tlib.EXPORTS), declared ^ set(tlib.EXPORTS)

    for W in (1, 2, 40, 128):
        for f in range(W + 11):
            assert L.tip_stream_window_len_w(f, W) == min(max(f - 4, 0), W), (f, W)
    for f in range(60):
        assert L.tip_stream_window_len_w(f, 40) == L.tip_stream_window_len(f)
    nb = ctypes.c_size_t()
    assert L.tip_stream_state_bytes_w(3, 40, ctypes.byref(nb)) == 0 and nb.value == 3 * 10496 * 4
    for W in (1, 41, 128):
        assert L.tip_stream_state_bytes_w(5, W, ctypes.byref(nb)) == 0 and nb.value == 5 * block_floats(W) * 4, W
    assert block_floats(40) == 10496

    # a window outside [1, 128] is refused before anything else is looked at — and before any launch: no device needed
    buf = (ctypes.c_float * 4)()
    p = ctypes.addressof(buf)
    for W in (0, -1, 129):
        assert L.tip_stream_state_bytes_w(1, W, ctypes.byref(nb)) == INVALID_ARG
        assert L.tip_stream_window_len_w(10, W) == INVALID_ARG
        assert L.tip_stream_reset_w(p, p, 1, 5, 1, W, None) == INVALID_ARG
        assert L.tip_stream_ingest_w(p, p, 1, 0, p, p, W, None) == INVALID_ARG
        assert L.tip_stream_consume_w(p, p, 1, 0, p, p, W, None) == INVALID_ARG
        assert L.tip_stream_attach_w(p, 1, p, p, 1, W, None) == INVALID_ARG
        assert L.tip_stream_detach_w(p, 1, p, 1, W, None) == INVALID_ARG
        assert L.tip_stream_ingest_staggered_w(p, p, 1, p, p, p, W, None) == INVALID_ARG
        assert L.tip_stream_consume_staggered_w(p, p, p, 1, p, p, W, None) == INVALID_ARG
        assert L.tip_stream_ingest_mapped_w(p, p, 1, p, 1, p, p, p, W, None) == INVALID_ARG
        assert L.tip_stream_consume_mapped_w(p, p, p, p, 1, 1, p, p, p, p, W, None) == INVALID_ARG
        assert L.tip_stream_history_override_w(p, 1, p, p, 1, W, None) == INVALID_ARG
    # the other argument checks are the 40-row entry points', at 40 and elsewhere
    for W in (24, 40):
        assert L.tip_stream_reset_w(p, p, 1, 3, 1, W, None) == INVALID_ARG
        assert L.tip_stream_reset_w(None, p, 1, 5, 1, W, None) == INVALID_ARG
        assert L.tip_stream_reset_w(p, p, 0, 5, 1, W, None) == 0
        assert L.tip_stream_ingest_w(None, p, 1, 0, p, p, W, None) == INVALID_ARG
        assert L.tip_stream_ingest_w(p, p, 1, 9, None, p, W, None) == INVALID_ARG
        assert L.tip_stream_ingest_w(p, p, 0, 9, p, p, W, None) == 0
        assert L.tip_stream_consume_w(p, None, 1, 0, p, p, W, None) == INVALID_ARG
        assert L.tip_stream_ingest_mapped_w(p, p, 1, p, 2, p, p, p, W, None) == INVALID_ARG      # B > n
        assert L.tip_stream_history_override_w(p, 1, None, None, 0, W, None) == 0


def test_engine_window_validation_needs_no_device():
    from tip_amd import streaming
    model = types.SimpleNamespace(input_size_imu=72, size_s=131, with_acc_sum=True, training=False)
    s_init = np.zeros((1, 114), dtype=np.float32)
    for cls in (streaming.StreamingEngine, streaming.StaggeredStreamingEngine):
        for bad in (0, 129, -1, 24.0, None):
            with pytest.raises(ValueError, match="window"):
                cls(model, s_init, window=bad)
        with pytest.raises(ValueError, match="window=24"):
            cls(model, s_init, reuse=True, window=24)
        with pytest.raises(ValueError, match=str(streaming.LIVE_WINDOW_MAX)):
            cls(model, s_init, live_dropout=True, window=streaming.LIVE_WINDOW_MAX + 1)
    assert streaming.LIVE_WINDOW_MAX == 40 and streaming.WINDOW_MAX == 128
