"""No GPU: the C-ABI surface of the deployed forward (tip_forward_live, tip_seeds_next) — header, bindings, exported symbols — and the
host restatement of the seed successor against the formula the header documents."""
import inspect
import os
import re

import pytest
import torch

import tip_amd
from tip_amd import lib as tlib
from tip_amd import synth
from conftest import ROOT
from test_host_cpu import make_model

HEADER = os.path.join(ROOT, "include", "tip_hip.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_and_lib_binds_the_live_entry_points():
    hdr = _header()
    m = re.search(r"TIP_API int tip_forward_live\((.*?)\);", hdr, re.S)
    assert m, "tip_forward_live is not declared"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 18 and args[6] == "const int* rows" and args[14] == "const unsigned long long* seeds_dev"
    assert re.search(r"TIP_API int tip_seeds_next\(unsigned long long\* seeds_dev, tip_stream_t stream\);", hdr)
    assert int(re.search(r"#define TIP_ABI_VERSION (\d+)", hdr).group(1)) == 5        # additions only
    assert "tip_forward_live" in tlib.EXPORTS and "tip_seeds_next" in tlib.EXPORTS
    lib = tlib.load()
    assert len(lib.tip_forward_live.argtypes) == 18 and len(lib.tip_seeds_next.argtypes) == 2
    assert lib.tip_forward_live.restype is lib.tip_seeds_next.restype is lib.tip_forward.restype
    # argument errors need no device: null handle / null buffer / misaligned buffer
    assert lib.tip_forward_live(None, None, None, None, 1, 40, None, 0, None, 1.0, 0.8, 1, 0.1, 2, None, None, 0, None) == -1
    assert lib.tip_seeds_next(None, None) == -1 and lib.tip_seeds_next(4, None) == -1


def test_seed_successor_matches_the_header_formula():
    """The header writes the successor out as three assignments to z and a final xor; evaluate THAT text and compare."""
    hdr = _header()
    doc = hdr[hdr.index("splitmix64 successor"):hdr.index("TIP_API int tip_seeds_next")]
    add = int(re.search(r"z = s \+ (0x[0-9A-Fa-f]+);", doc).group(1), 16)
    m1 = re.search(r"z = \(z \^ \(z >> (\d+)\)\) \* (0x[0-9A-Fa-f]+);\s+z = \(z \^ \(z >> (\d+)\)\) \* (0x[0-9A-Fa-f]+);", doc)
    last = int(re.search(r"next\(s\) = z \^ \(z >> (\d+)\)", doc).group(1))
    M = (1 << 64) - 1

    def header_next(s):
        z = (s + add) & M
        z = ((z ^ (z >> int(m1.group(1)))) * int(m1.group(2), 16)) & M
        z = ((z ^ (z >> int(m1.group(3)))) * int(m1.group(4), 16)) & M
        return z ^ (z >> last)

    for s in (0, 1, 123456789, 2 ** 62 - 1, 2 ** 63, M, 0x9E3779B97F4A7C15):
        assert tlib.seed_successor(s) == header_next(s), hex(s)
    assert tlib.seed_successor(0) == 0xE220A8397B1DCDAF                      # splitmix64's first output for state 0
    # a chain never returns to its start within a few steps and the two words stay distinct
    s, seen = 42, set()
    for _ in range(1000):
        s = tlib.seed_successor(s)
        assert s not in seen
        seen.add(s)


def test_host_surface():
    m = make_model(synth.PAPER, p_state=0.8)
    sig = inspect.signature(m.forward_live)
    assert [p for p in sig.parameters] == ["x_imu", "x_s", "rows", "last_row_only", "seeds", "seeds_dev", "workspace", "out"]
    assert all(sig.parameters[p].kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters)[2:])
    assert sig.parameters["last_row_only"].default is True
    from tip_amd.streaming import StreamingEngine, StaggeredStreamingEngine
    for eng in (StreamingEngine, StaggeredStreamingEngine):
        p = inspect.signature(eng.__init__).parameters["live_dropout"]
        assert p.default is False
    # CPU tensors: refused like every inference entry point (no fallback)
    x_imu, x_s = synth.make_inputs(synth.PAPER, 1, 4, seed=0)
    with pytest.raises(RuntimeError):
        m.forward_live(torch.tensor(x_imu), torch.tensor(x_s))
