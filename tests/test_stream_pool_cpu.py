"""Compact staggered pools without a GPU: the position allocator (streaming.SlotPositions) and the batch ladder (streaming.pool_ladder)."""
import random

import pytest

from tip_amd import streaming


def _check_dense(sp, attached):
    k = len(sp)
    assert sorted(sp.slot_at) == sorted(attached)                 # every attached slot holds exactly one position ...
    assert len(set(sp.slot_at)) == k
    for p, s in enumerate(sp.slot_at):                            # ... and the positions are 0 .. k-1
        assert sp.pos[s] == p
    assert sum(1 for q in sp.pos if q >= 0) == k
    assert all(sp.pos[s] == -1 for s in range(sp.n) if s not in attached)


@pytest.mark.parametrize("n", [1, 7, 64, 300])
def test_positions_stay_dense_and_unique(n):
    rng = random.Random(n)
    sp = streaming.SlotPositions(n, range(n))
    assert sp.slot_at == list(range(n))                           # a fresh pool: positions = slots
    attached = set(range(n))
    for _ in range(2000):
        s = rng.randrange(n)
        op = rng.random()
        if op < 0.45:
            before = list(sp.slot_at)
            changed = sp.detach(s)
            assert changed == (s in attached)
            if changed:
                p = before.index(s)
                if p == len(before) - 1:
                    assert sp.slot_at == before[:-1]
                else:                                             # the slot at the last position moves into the hole
                    assert sp.slot_at == before[:p] + [before[-1]] + before[p + 1:-1]
            attached.discard(s)
        else:
            was = sp.pos[s]
            changed = sp.attach(s)
            assert changed == (was < 0)
            if was >= 0:
                assert sp.pos[s] == was                           # re-attaching keeps the position
            else:
                assert sp.pos[s] == len(sp) - 1                   # a new slot takes position k
            attached.add(s)
        _check_dense(sp, attached)
    sp.reset(attached)
    assert sp.slot_at == sorted(attached)                          # reset(): slot order again
    _check_dense(sp, attached)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 24, 40, 64, 65, 256, 257, 300, 512, 700, 1024, 1500, 4096])
def test_ladder_is_monotone_and_ends_at_n(n):
    lad = streaming.pool_ladder(n)
    assert lad[-1] == n and lad[0] == 1
    assert all(a < b for a, b in zip(lad, lad[1:]))
    assert streaming.pool_bucket(0, lad) == 0
    prev = 0
    for k in range(1, n + 1):
        b = streaming.pool_bucket(k, lad)
        assert k <= b <= n and b in lad and b >= prev
        prev = b
    assert streaming.pool_bucket(n, lad) == n


def test_ladder_follows_the_auto_staircase():
    """The buckets the pool benchmark's rows land in (profiles/pool/): the top of the step that holds k."""
    lad = streaming.pool_ladder(1024)
    want = {1: 1, 8: 8, 9: 16, 24: 24, 25: 32, 33: 64, 64: 64, 100: 128, 200: 256, 256: 256, 257: 264, 281: 320, 300: 320, 500: 512,
            513: 520, 545: 576, 700: 768, 777: 784, 793: 832, 1000: 1024, 1024: 1024}
    assert {k: streaming.pool_bucket(k, lad) for k in want} == want
