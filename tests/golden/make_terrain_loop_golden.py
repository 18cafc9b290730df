#!/usr/bin/env python3
"""Golden fixture of the REFERENCE's true closed loop for tip_amd.replay.ReplayPool(terrain=...): the real RTRunner.step
(real_time_runner.py; five_sbp, with_acc_sum, multi_sbp_terrain_and_correction=True, play_back_gt=False) around the reference's own
TF_RNN_Past_State (past_state_dropout = 0, .eval()) — model -> tracker -> leg IK -> model history -> model — on one synthetic
recording.  tip_terrain_golden.npz is teacher-forced with a scripted model; here the pose the IK corrects really reaches the next
model call.

Runs only in the build container (it reads the reference checkout).  The reference's real_time_runner, data_utils and
simple_transformer_with_state are imported as they are; what is not installed is stood in exactly as the other makers do, imported
from them unchanged: make_runner_golden.install_stubs / smooth_imu_sequence (fairmotion -> scipy: parity UNPINNED),
make_kin_golden.make_char / q_diff (KinChar: real FK of data/amass.urdf through tests/kin_oracle.py, PyBullet parity UNPINNED).

The weights are tip_amd.synth.make_weights(PAPER, seed 0) — what the tests' load_synth loads — with ONE departure, stored in the
fixture: `bias_index` / `bias_shift`, added to linear.bias at the contact-logit entries (with random weights the contact flags are
coin flips and the IK never sees a held contact).  The recording is a standing character's IMU: the root sensor upright with a slow
yaw, the others smooth (make_runner_golden.smooth_imu_sequence), and s_init upright.

The maker searches recording seeds SEEDS (at most 50) and keeps the first one for which, over the stored horizon F_cmp (rows
0 .. F_cmp - 1 of the script's row convention):
  - the IK fired on at least MIN_FIRED rows, with at least MIN_CALLS_AFTER model calls after the first of them;
  - tests/terrain_oracle.py, teacher-forced in fp64 on the reference's own rows, takes the reference's fire decisions, and every decision
    margin its trace reports is at least MIN_MARGIN (as make_terrain_golden.py requires).
F_cmp is the longest horizon up to the recording's length that meets the margin bar.  If no seed qualifies the maker says so, writes
nothing and exits with status 1.

tests/golden/tip_terrain_loop_golden.npz (data only), rows by the script's convention (row 0 the start state, the step on frame t
fills row t + 1):
  table/*            the skeleton table, as in tip_terrain_golden.npz
  raw_imu [L, 72], s_init [114], qdq [L, 114], ct [L, 20], viz_locs [L, 5, 3], valid [L]
  y_last [L, 131]    the model's raw last row of the call that made the row (NaN where there was none)
  q_hist [L, 54]     the pose the runner fed back (record_state_aa_and_c's argument, columns 3 .. 56)
  fire [L]           q_hist differs from the returned pose
  hist [L, 131]      the newest history row after the step, as the model sees it on the next frame
  f32/root [F_cmp, 3], f32/viz_locs [F_cmp, 5, 3]   the same loop restated in float32 (oracle.forward and terrain_oracle in float32 on the
                     same weights and frames, tests/replay_terrain_oracle.py): it takes the reference's fire decisions on every row
  F_cmp, seed, bias_index, bias_shift, min_margins (terrain_oracle.MARGINS order), searched (per seed tried: seed, fired rows, calls
  after the first fire, F_cmp, the smallest margin), conversions_impl, fk_impl

usage: python tests/golden/make_terrain_loop_golden.py
"""
import os
import sys

import numpy as np
import torch
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
REF = "/root/reference"

import kin_oracle as ko                # noqa: E402
import make_kin_golden as mkg          # noqa: E402
import make_runner_golden as mrg       # noqa: E402
import terrain_oracle as to            # noqa: E402

MAP_BOUND, GRID_SIZE, MIN_MARGIN = 5.0, 0.1, 1e-4
N_FRAMES, SEEDS = 160, tuple(range(50))
MIN_FIRED, MIN_CALLS_AFTER = 3, 10
BIAS_INDEX = np.array([111, 115, 127])          # the contact logits of lankle, rankle and root
BIAS_SHIFT = np.array([0.5, 0.5, 0.5], dtype=np.float32)
UP = Rotation.from_rotvec([np.pi / 2, 0, 0])    # the character's zero pose has its legs along -y: y -> z (make_terrain_golden.py)


def recording(n, seed):
    imu = mrg.smooth_imu_sequence(n, seed)
    t = np.arange(n) / 60.0
    yaw = 0.3 * np.sin(2 * np.pi * 0.2 * t)
    imu[:, :9] = (Rotation.from_rotvec(np.stack([0 * yaw, 0 * yaw, yaw], axis=1)) * UP).as_matrix().reshape(n, 9)
    s_init = np.zeros(114)
    s_init[:3] = [0.2, -0.1, 0.93]
    s_init[3:6] = UP.as_rotvec()
    return imu.astype(np.float32).astype(np.float64), s_init         # (the frames as the float32 the device is fed)


def run_reference(RTRunner, char, model, imu, s_init):
    L = imu.shape[0]
    runner = RTRunner(char, model, 40, s_init, MAP_BOUND, GRID_SIZE, play_back_gt=False, five_sbp=True, with_acc_sum=True,
                      multi_sbp_terrain_and_correction=True)
    fed, rows, record, forward = [], [], runner.record_state_aa_and_c, model.forward

    def tapped_record(cur_s, cur_c):
        fed.append(np.array(cur_s[3:57]).copy())
        return record(cur_s, cur_c)

    def tapped_forward(x_imu, x_s):
        y = forward(x_imu, x_s)
        rows.append(y.detach().numpy()[0, -1].copy())
        return y

    runner.record_state_aa_and_c, model.forward = tapped_record, tapped_forward
    try:
        out = {"qdq": np.repeat(s_init[None], L, 0), "ct": np.zeros((L, 20)), "viz_locs": np.full((L, 5, 3), 100.0),
               "valid": np.zeros(L, bool), "y_last": np.full((L, 131), np.nan), "q_hist": np.repeat(s_init[None, 3:57], L, 0),
               "hist": np.zeros((L, 131))}
        out["hist"][0] = runner.s_and_c_in_buffer[-1]
        for t in range(L - 1):                                               # the script's loop (offline_testing_simple.py:123-139)
            n_calls, n_fed = len(rows), len(fed)
            res = runner.step(imu[t], out["qdq"][t, :3], t)
            out["qdq"][t + 1], out["ct"][t + 1], out["viz_locs"][t + 1] = res["qdq"], res["ct"], res["viz_locs"]
            out["hist"][t + 1] = runner.s_and_c_in_buffer[-1]
            if len(rows) > n_calls:
                out["valid"][t + 1], out["y_last"][t + 1] = True, rows[-1]
                assert len(fed) == n_fed + 1
                out["q_hist"][t + 1] = fed[-1]
            else:
                out["q_hist"][t + 1] = out["qdq"][t + 1, 3:57]
    finally:
        model.forward = forward
    out["fire"] = (out["q_hist"] != out["qdq"][:, 3:57]).any(axis=1)
    return out


def horizon(table, s_init, ref):
    """The longest F (rows 0 .. F - 1) over which the fp64 oracle, teacher-forced, takes the reference's fire decisions with every
    margin at least MIN_MARGIN; (F, fired rows, model calls after the first fire, margins over that horizon)."""
    L = ref["qdq"].shape[0]
    G, D = to.grid_num(MAP_BOUND, GRID_SIZE), to.diffuse_region(GRID_SIZE)
    st, F, margins = to.State(table, s_init, G, 64, np.float64), 1, {k: np.inf for k in to.MARGINS}
    for r in range(1, L):
        if ref["valid"][r]:
            tr = to.new_trace()
            fired = to.step(table, st, ref["qdq"][r, 3:], ref["ct"][r], G, D, GRID_SIZE, True, np.float64, tr, r)[3]
            if bool(fired) != bool(ref["fire"][r]) or min(tr["margins"].values()) < MIN_MARGIN:
                break
            margins = {k: min(margins[k], tr["margins"][k]) for k in margins}
        F = r + 1
    rows = np.nonzero(ref["fire"][:F])[0]
    after = int(ref["valid"][rows[0] + 1:F].sum()) if len(rows) else 0
    return F, len(rows), after, margins


def main():
    mrg.install_stubs(False)
    sys.modules["fairmotion.ops.quaternion"].Q_diff = mkg.q_diff
    sys.path.insert(0, REF)
    import tip_amd  # noqa: F401
    from tip_amd import synth
    import amass_char_info as info
    from real_time_runner import RTRunner
    from simple_transformer_with_state import TF_RNN_Past_State
    torch.Tensor.cuda = lambda self, *a, **k: self      # harness only
    table = ko.read_urdf(os.path.join(REF, "data", "amass.urdf"), info)
    char, fk_impl = mkg.make_char(table, info, False)
    w = synth.make_weights(synth.PAPER, seed=0)
    w["linear.bias"] = w["linear.bias"].copy()
    w["linear.bias"][BIAS_INDEX] += BIAS_SHIFT
    model = TF_RNN_Past_State(72, 131, rnn_hid_size=512, tf_hid_size=1024, tf_in_dim=256, n_heads=16, tf_layers=4, dropout=0.0,
                              in_dropout=0.0, past_state_dropout=0.0, with_acc_sum=True)
    model.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    model.eval()
    searched, found = [], None
    for seed in SEEDS:
        imu, s_init = recording(N_FRAMES, seed)
        with torch.no_grad():
            ref = run_reference(RTRunner, char, model, imu, s_init)
        F, fired, after, margins = horizon(table, s_init, ref)
        worst = min(margins.values())
        searched.append((seed, fired, after, F, worst if np.isfinite(worst) else -1.0))
        print(f"seed {seed}: fired rows {int(ref['fire'].sum())} in all; over F_cmp = {F}: fired {fired}, calls after the first fire {after}, "
              f"smallest margin {worst:.2e}")
        if fired >= MIN_FIRED and after >= MIN_CALLS_AFTER:
            found = (seed, imu, s_init, ref, F, margins)
            break
    if found is None:
        print("NO SEED QUALIFIES: nothing written.  Searched (seed, fired, calls after, F_cmp, smallest margin):", searched)
        sys.exit(1)
    seed, imu, s_init, ref, F, margins = found
    assert min(margins.values()) >= MIN_MARGIN
    # the same loop restated in float32 — the forward oracle and the tracker in float32, on the same weights and frames — for the noise
    # floor the GPU test takes its root / viz_locs bound from (the stream half stays StreamOracle's fp64: the floor is not overstated)
    from oracle import oracle
    import replay_terrain_oracle as rto
    lo = rto.run(table, imu[:F], s_init, lambda x_imu, x_s: oracle.forward(synth.PAPER, w, x_imu[None], x_s[None], dtype=np.float32)[0, -1],
                 dtype=np.float32, rows_f32=True)
    assert np.array_equal(lo["fire"], ref["fire"][:F]) and np.array_equal(lo["valid"], ref["valid"][:F])
    noise = {k: float(np.abs(lo[k].astype(np.float64) - r).max()) for k, r in (("root", ref["qdq"][:F, :3]), ("viz_locs", ref["viz_locs"][:F]),
                                                                              ("s_rest", ref["qdq"][:F, 3:]))}
    print("the float32 restatement of the loop against the reference:", {k: float(f"{v:.3g}") for k, v in noise.items()})
    out = {"table/" + k: v for k, v in table.items()}
    out.update({"raw_imu": imu.astype(np.float32), "s_init": s_init, "qdq": ref["qdq"], "ct": ref["ct"], "viz_locs": ref["viz_locs"],
                "valid": ref["valid"], "y_last": ref["y_last"].astype(np.float32), "q_hist": ref["q_hist"], "fire": ref["fire"],
                "hist": ref["hist"], "F_cmp": np.array([F]), "seed": np.array([seed]), "bias_index": BIAS_INDEX, "bias_shift": BIAS_SHIFT,
                "min_margins": np.array([margins[k] for k in to.MARGINS]), "searched": np.array(searched, dtype=np.float64),
                "f32/root": lo["root"].astype(np.float32), "f32/viz_locs": lo["viz_locs"].astype(np.float32)})
    conv = "scipy stand-in (fairmotion fork absent: parity UNPINNED)"
    out["conversions_impl"] = np.frombuffer(conv.encode(), dtype=np.uint8).copy()
    out["fk_impl"] = np.frombuffer(fk_impl.encode(), dtype=np.uint8).copy()
    path = os.path.join(HERE, "tip_terrain_loop_golden.npz")
    np.savez_compressed(path, **out)
    print(f"seed {seed}: F_cmp {F}, fired rows {np.nonzero(ref['fire'][:F])[0].tolist()}, margins",
          {k: float(f"{v:.3g}") for k, v in margins.items()})
    print("wrote", path, os.path.getsize(path), "bytes; FK:", fk_impl)
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
