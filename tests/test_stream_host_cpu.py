"""The streaming engines' pure host pieces without a GPU or the library: the slot-list validator (streaming.slot_list) and the staging
image a compact pool uploads between two frames (streaming.stage_image), against a word-by-word restatement of its layout."""
import random
import struct

import numpy as np
import pytest

from tip_amd import streaming


def _image_restated(n, positions, attach, detach, rows):
    """include/tip_hip.h, tip_stream_ingest_mapped / tip_stream_attach: little-endian 32-bit words, one at a time."""
    words = [-1] * n
    for p, s in enumerate(positions):
        words[p] = s                                  # position -> slot; the positions past k stay -1
    o_att = len(words)
    words += list(attach)
    if len(words) % 2:
        words.append(None)                            # padding word: the int64 block starts on 8 bytes; its value is not defined
    o_det = len(words)
    for s in detach:
        words += list(struct.unpack("<ii", struct.pack("<q", s)))
    o_rows = len(words)
    for r in rows:
        words += list(struct.unpack("<114i", np.asarray(r, dtype="<f4").tobytes()))
    return words, (o_att, o_det, o_rows)


def _check(n, sp, attach, detach, s_host):
    rows = s_host[attach] if attach else np.zeros((0, 114), dtype=np.float32)
    img, off = streaming.stage_image(n, sp.slot_at, attach, detach, rows)
    want, want_off = _image_restated(n, sp.slot_at, attach, detach, rows)
    assert img.dtype == np.int32 and img.ndim == 1 and img.flags["C_CONTIGUOUS"]
    assert tuple(off) == want_off and img.size == len(want) <= n * 118 + 2         # fits the engine's staging buffer
    o_att, o_det, o_rows = off
    assert o_att == n and o_det % 2 == 0 and 0 <= o_det - (n + len(attach)) <= 1    # int64 block: 8-byte aligned, at most one pad word
    assert o_rows == o_det + 2 * len(detach) and img.size == o_rows + 114 * len(attach)
    for i, w in enumerate(want):
        if w is not None:
            assert img[i] == w, (i, off)
    assert (img[len(sp): n] == -1).all() and sorted(img[: len(sp)].tolist()) == sorted(sp.slot_at)
    assert img[o_det: o_rows].view(np.int64).tolist() == list(detach)               # what the engine's index_fill_ reads
    assert img[o_rows:].view(np.float32).tobytes() == np.asarray(rows, dtype=np.float32).tobytes()   # row bits, NaN payloads included


@pytest.mark.parametrize("n", [1, 2, 5, 64, 257])
def test_stage_image_layout_over_random_attach_detach_sequences(n):
    """60 sequences per pool size (300 in all), each a few frames of random attach / detach calls between two uploads, as
    StaggeredStreamingEngine(compact=True) records them: dict-ordered pending lists, a slot possibly in both."""
    rng = random.Random(n)
    nrng = np.random.RandomState(n)
    for seq in range(60):
        sp = streaming.SlotPositions(n, [s for s in range(n) if rng.random() < 0.7])
        s_host = nrng.randn(n, 114).astype(np.float32)
        s_host[nrng.randint(n), nrng.randint(114)] = np.float32("nan")
        s_host.view(np.int32)[nrng.randint(n), nrng.randint(114)] = rng.randrange(-2 ** 31, 2 ** 31)     # any bit pattern survives
        for frame in range(rng.randrange(1, 6)):
            att, det = {}, {}
            for _ in range(rng.choice((0, 0, 1, 3, n))):
                s = rng.randrange(n)
                if rng.random() < 0.5:
                    sp.attach(s)
                    att[s] = None
                else:
                    sp.detach(s)
                    det[s] = None
            if seq % 7 == 0 and frame == 0:
                att = {}                                                          # empty attach list with a detach list, and both empty
            _check(n, sp, list(att), list(det), s_host)


def test_stage_image_empty_pool_and_empty_lists():
    sp = streaming.SlotPositions(4)
    img, off = streaming.stage_image(4, sp.slot_at, [], [], np.zeros((0, 114), dtype=np.float32))
    assert img.tolist() == [-1] * 4 and tuple(off) == (4, 4, 4)
    img, off = streaming.stage_image(3, [2], [], [1], np.zeros((0, 114), dtype=np.float32))
    assert tuple(off) == (3, 4, 6) and img[:3].tolist() == [2, -1, -1] and img[4:6].view(np.int64).tolist() == [1]
    img, off = streaming.stage_image(3, [2, 0], [0], [], np.full((1, 114), 1.0, dtype=np.float32))
    assert tuple(off) == (3, 4, 4) and img[:4].tolist() == [2, 0, -1, 0] and (img[4:] == 0x3F800000).all() and img.size == 4 + 114


def test_slot_list_accepts_and_refuses():
    assert streaming.slot_list([], 4, "X.f") == []
    assert streaming.slot_list((3, 0, 2), 4, "X.f") == [3, 0, 2]                   # order kept
    assert streaming.slot_list(range(2, 4), 4, "X.f") == [2, 3]
    assert streaming.slot_list(np.array([1, 0], dtype=np.int64), 4, "X.f") == [1, 0]
    out = streaming.slot_list([np.int32(1)], 4, "X.f")
    assert out == [1] and type(out[0]) is int
    must, outside, dup = "slots must be a list of slot indices", "slot index outside [0, 4)", "duplicate slot index"
    for bad, text in ((3, must), (None, must), ([None], must), ([4], outside), ([-1], outside), ([0, 4, 0], outside), ([1, 1], dup),
                      ([0, 2, 0], dup)):
        with pytest.raises(ValueError) as e:
            streaming.slot_list(bad, 4, "X.f")
        assert str(e.value) == f"tip_amd.X.f: {text}"
    with pytest.raises(ValueError):
        streaming.slot_list([0], 0, "X.f")                                        # no slot fits an empty pool
