"""tip_amd.terrain without a GPU: the C-ABI surface of tip_terrain_*, the map constants, and the oracle the GPU tests compare against
(tests/terrain_oracle.py) held to the reference-generated golden (tests/golden/tip_terrain_golden.npz: the real RTRunner.step, three
tracks, multi_sbp_terrain_and_correction off and on)."""
import ctypes
import os
import re

import numpy as np
import pytest

import terrain_oracle as to
from tip_amd import lib as tlib
from tip_amd import terrain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"tip_terrain_state_bytes": 4, "tip_terrain_reset": 9, "tip_terrain_track": 22}      # name: number of arguments
FP64_BOUND = 1e-12                # the issue's bound for the fp64 restatement against the reference; measured: 1.5e-14
TRACKS = (("track0", 199), ("track1", 259), ("track2", 249))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "tip_terrain_golden.npz"))


@pytest.fixture(scope="module")
def table(golden):
    return {k[len("table/"):]: golden[k] for k in golden.files if k.startswith("table/")}


def test_c_abi_surface():
    """Every tip_terrain_* name is declared in the header, exported by the library and bound in lib.py; the ABI is still 5; null
    pointers, negative counts and sizes out of range return -1 and a zero count returns 0, all before any launch."""
    hdr = open(os.path.join(ROOT, "include", "tip_hip.h")).read()
    assert set(re.findall(r"TIP_API int (tip_terrain_\w+)\(", hdr)) == set(NAMES)
    assert int(re.search(r"#define TIP_ABI_VERSION (\d+)", hdr).group(1)) == 5
    raw = ctypes.CDLL(tlib.LIB_PATH)
    lib = tlib.load()
    for name, nargs in NAMES.items():
        m = re.search(r"TIP_API int " + name + r"\((.*?)\);", hdr, re.S)
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == nargs, name
        assert name in tlib.EXPORTS and hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == nargs and getattr(lib, name).restype is lib.tip_forward.restype, name
    assert lib.tip_abi_version() == 5 and tlib.TIP_ABI_VERSION == 5
    n = ctypes.c_size_t()
    for bad in ((-1, 100, 64), (3, 1, 64), (3, 5000, 64), (3, 100, 0), (3, 100, 70000)):
        assert lib.tip_terrain_state_bytes(*bad, ctypes.byref(n)) == -1, bad
    assert lib.tip_terrain_state_bytes(3, 100, 64, None) == -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)        # a non-null pointer: every call below returns before it would launch
    ok = (p, p, 4, 100, 64, None, 1, p, None)
    for k in (0, 1, 7):
        args = list(ok)
        args[k] = None
        assert lib.tip_terrain_reset(*args) == -1, k
    for k, bad in ((2, -1), (3, 0), (4, 0), (6, -1)):
        args = list(ok)
        args[k] = bad
        assert lib.tip_terrain_reset(*args) == -1, k
    args = list(ok)
    args[6] = 0
    assert lib.tip_terrain_reset(*args) == 0
    ok = (p, p, 4, 100, 64, 5, 0.1, None, p, p, 1, 8, p, p, 20, None, 0, p, p, p, p, None)
    for k in (0, 1, 8, 9, 12, 13, 17, 18, 19, 20):     # each required pointer in turn
        args = list(ok)
        args[k] = None
        assert lib.tip_terrain_track(*args) == -1, k
    # n_slots, grid_num, max_regions, diffuse_region (0 and 17), grid_size (0, NaN), count, n_rows, a c_t width, an unknown flag
    for k, bad in ((2, -1), (3, 1), (4, 0), (5, 0), (5, 17), (6, 0.0), (6, float("nan")), (10, -1), (11, -1), (14, 12), (16, 2)):
        args = list(ok)
        args[k] = bad
        assert lib.tip_terrain_track(*args) == -1, (k, bad)
    args = list(ok)
    args[14], args[16] = 8, 1                         # two SBPs with multi_sbp_terrain_and_correction: the fifth SBP is missing
    assert lib.tip_terrain_track(*args) == -1
    args[16] = 0
    args[10] = 0
    assert lib.tip_terrain_track(*args) == 0
    src = open(os.path.join(tlib.CSRC, "tip_terrain.hip")).read()
    assert "asm" not in src and "getenv" not in src and "tip_env" not in src


def test_state_bytes_linear_and_aligned():
    lib = tlib.load()
    one, n = ctypes.c_size_t(), ctypes.c_size_t()
    for G, M in ((100, 64), (200, 64), (20, 4), (6, 1)):
        assert lib.tip_terrain_state_bytes(1, G, M, ctypes.byref(one)) == 0
        assert one.value % 8 == 0 and one.value >= 1024 + 120 + 48 + 12 + 12 + 16 * M + 4 * G * G
        assert one.value == terrain.HEAD_BYTES + 16 * M + 4 * G * G      # what TerrainState reads
        for k in (0, 3, 1024):
            assert lib.tip_terrain_state_bytes(k, G, M, ctypes.byref(n)) == 0 and n.value == k * one.value
    assert lib.tip_terrain_state_bytes(1, 200, 64, ctypes.byref(one)) == 0 and one.value < 165 * 1024      # 160 KB of map per slot


def test_map_constants_are_the_references():
    """int(map_bound / grid_size) * 2 and round(0.5 / grid_size) (real_time_runner.py:115, :128): 100 at the demo's 5 m / 0.1 m, 200 at
    the offline script's 10 m / 0.1 m, patches of 2 x 5 cells."""
    for mod in (terrain, to):
        assert mod.grid_num(5.0, 0.1) == 100 and mod.grid_num(10.0, 0.1) == 200 and mod.diffuse_region(0.1) == 5
        assert mod.grid_num(1.0, 0.1) == 20 and mod.diffuse_region(0.05) == 10
    assert to.chains(_table()) == [((0, 1, 2, 3), [3, 6, 9]), ((0, 4, 5, 6), [45, 48, 51])]      # ik_chain_map_* (:81-95)


def _table():
    g = np.load(os.path.join(ROOT, "tests", "golden", "tip_terrain_golden.npz"))
    return {k[len("table/"):]: g[k] for k in g.files if k.startswith("table/")}


def golden_track(golden, tag, multi):
    """(s_init, s_rest [n, 111], ct, valid, expected dict) of one golden track in one mode."""
    s57 = golden[tag + "/s_rest"]
    s_rest = np.concatenate([s57, np.zeros((s57.shape[0], 54))], axis=1)
    pre = f"{tag}/m{int(multi)}/"
    exp = {k[len(pre):]: golden[k] for k in golden.files if k.startswith(pre)}
    q_hist = s_rest[:, :54].copy()
    q_hist[exp["fire_rows"]] = exp["q_hist"]
    exp["q_hist"] = q_hist
    return golden[tag + "/s_init"], s_rest, golden[tag + "/ct"], golden[tag + "/valid"], exp


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("tag,n", TRACKS)
def test_oracle_matches_the_golden_teacher_forced(golden, table, tag, n, multi):
    """Inputs: the golden's qdq[3:114] and ct of every step; outputs: the real RTRunner.step's qdq[:3], viz_locs, the pose it fed
    back, and its state after every step and at the end.  Continuous values within 1e-12, every discrete value equal."""
    s_init, s_rest, ct, valid, exp = golden_track(golden, tag, multi)
    assert s_rest.shape == (n, 111) and ct.shape == (n, 20) and not valid[:5].any() and valid[5:].all()
    root, viz, q_hist, fire, st, tr = to.track(table, s_init, s_rest, ct, valid, 5.0, 0.1, multi, 64)
    errs = {"root": np.abs(root - exp["root"]).max(), "viz_locs": np.abs(viz - exp["viz_locs"]).max(),
            "q_hist": np.abs(q_hist - exp["q_hist"]).max(),
            "region_height": np.abs(np.array(st.region_height) - exp["region_height"]).max(),
            "region_weight": np.abs(np.array(st.region_weight) - exp["region_weight"]).max(),
            "ik_deltas": np.abs(st.ik_deltas - exp["ik_deltas"]).max()}
    print(f"{tag} multi={int(multi)}: oracle - golden", {k: float(f"{v:.2e}") for k, v in errs.items()})
    assert all(v <= FP64_BOUND for v in errs.values()), errs
    assert np.array_equal(fire, exp["fire"]) and np.array_equal(tr["ticks"], exp["ticks"]) and np.array_equal(tr["n_regions"], exp["n_regions"])
    assert np.array_equal(st.region_map, exp["region_map"]) and st.off_map == 0 and st.regions_full == 0
    assert (viz[~valid] == 100).all() and (root[~valid] == s_init[:3]).all() and not fire[~valid].any()
    if not multi:
        assert not fire.any() and not st.ik_deltas.any()
    assert min(tr["margins"].values()) >= 1e-4, tr["margins"]


def test_the_fixture_reaches_every_branch(golden):
    """What the generator asserted when it wrote the fixture: every branch at least 3 times, every decision margin >= 1e-4."""
    counts = dict(zip(to.BRANCHES, golden["branch_counts"]))
    margins = dict(zip(to.MARGINS, golden["min_margins"]))
    print(counts, margins)
    for k in ("merge", "new", "region0", "expiry", "ik_fire", "ik_small", "ik_reset", "pelvis_near"):
        assert counts[k] >= 3, (k, counts)
    assert min(margins.values()) >= 1e-4, margins
    assert golden["track0/m1/fire"].sum() >= 5 and golden["track2/m1/region_map"].shape == (100, 100)


def test_oracle_open_cases():
    """The decisions the reference leaves open, on the oracle: off-map and overflow write nothing and are counted; a tie goes to the
    lower index; a non-finite location is inactive."""
    table = _table()
    st = to.State(table, np.zeros(114), 20, 2, np.float64)
    tr = to.new_trace()
    st.c_prev[0] = [0.9, 0.0, 0.5]                     # centre cell 9 + 10: the patch [14, 24) leaves the 20-cell map
    st.ticks[0] = 0
    before = st.region_map.copy()
    assert to._update(st, 0, 0, 20, 5, 0.1, np.float64, tr, 0, False) == 0 and st.off_map == 1 and st.ticks[0] == -1
    assert np.array_equal(st.region_map, before) and len(st.region_height) == 1
    st.c_prev[0] = [0.0, 0.0, 0.5]
    st.ticks[0] = 0
    assert to._update(st, 0, 0, 20, 5, 0.1, np.float64, tr, 0, False) == 0 and len(st.region_height) == 2      # a new region: h - h
    st.c_prev[0] = [0.0, 0.0, 1.0]
    st.ticks[0] = 0
    before = st.region_map.copy()
    assert to._update(st, 0, 0, 20, 5, 0.1, np.float64, tr, 0, False) == 0 and st.regions_full == 1 and len(st.region_height) == 2
    assert np.array_equal(st.region_map, before) and st.ticks[0] == -1
    st.c_prev[0] = [np.nan, 0.0, 0.5]
    st.ticks[0] = 0
    assert to._update(st, 0, 0, 20, 5, 0.1, np.float64, tr, 0, False) == 0 and st.ticks[0] == 0      # inactive: nothing moves
    st2 = to.State(table, np.zeros(114), 20, 8, np.float64)
    st2.region_height, st2.region_weight = [0.0, 0.5, 0.625], [10.0, 10.0, 10.0]
    st2.region_map[8:10, 8:10], st2.region_map[10:12, 10:12] = 2, 1
    st2.c_prev[0], st2.ticks[0] = [0.0, 0.0, 0.5625], 0           # 0.0625 from both, exactly
    to._update(st2, 0, 0, 20, 5, 0.1, np.float64, tr, 0, False)
    assert st2.region_map[10, 10] == 1 and st2.region_weight == [10.0, 11.0, 10.0]
