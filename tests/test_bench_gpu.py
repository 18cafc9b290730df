"""GPU: bench.py's plain run (`--gpus 1 --steps K --warmup W`) prints the headline line alone, times exactly K steps, and with
--dump-outputs writes what the last timed step computed: the [B, T, 131] output of the B = 256 headline forward on bench.py's seeded
inputs, held to the oracle like tests/test_hip_parity.py::test_auto_plan_at_the_bench_batch_vs_oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    from tip_amd import synth
    from oracle import oracle
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
           "--dump-outputs", str(tmp_path)]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] - 256 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert d["extra"] == {} and d["cpu_baseline"] is None and d["ranks_output_identical"] is None
    assert sorted(os.listdir(tmp_path)) == ["y.npy"]
    y = np.load(tmp_path / "y.npy")
    assert y.dtype == np.float32 and y.shape == (256, 40, 131)
    cfg = synth.PAPER
    w = synth.make_weights(cfg, seed=0)
    x_imu, x_s = synth.make_inputs(cfg, 256, 40, seed=1234)      # bench.py's inputs at rank 0
    yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float32)
    assert np.abs(y - yo).max() < 2e-5, np.abs(y - yo).max()
