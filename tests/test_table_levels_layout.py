"""Slot layout of the 8-bit level gather (spf_table_levels_layout, host only;
include/openr_spf.h SPF_T_GATHER_LEVELS): every rank slot holds cap =
ceil(n / world) level rows of `pitch` bytes (V rounded up to 16, the query's
level-row stride) and a 16-byte trailer; the slots are equal-sized so one
in-place all-gather exchanges them.
"""

import numpy as np
import pytest

from openr_amd import abi

CASES = [(10, 3, 17), (9976, 8, 9976), (7, 8, 5), (1, 1, 1), (0, 4, 100), (23, 4, 16), (5, 2, 33)]


@pytest.mark.parametrize("n,world,V", CASES)
def test_levels_layout_rules(n, world, V):
    pitch, slot_bytes, trailer_off = abi.table_levels_layout(n, world, V)
    assert pitch == (V + 15) // 16 * 16 and pitch >= V
    cap = (n + world - 1) // world
    # the trailer sits inside the slot, right after the cap rows
    assert trailer_off == cap * pitch
    assert trailer_off + 16 <= slot_bytes
    # equal-sized slots (one value for every rank), 16-byte granular
    assert slot_bytes % 16 == 0 and trailer_off % 16 == 0
    # every block fits before its trailer (blocks of spf_table_layout)
    bf, _, _ = abi.table_layout(n, world, V)
    for r in range(world):
        assert int(bf[r + 1] - bf[r]) * pitch <= trailer_off


def test_levels_layout_fabric_bytes():
    """The fabric's exchange at world 1: one slot of 9,976 rows, about 100 MB
    (a quarter of the 398 MB of uint32 rows)."""
    pitch, slot_bytes, _ = abi.table_levels_layout(9976, 1, 9976)
    assert pitch == 9984
    assert slot_bytes == 9976 * 9984 + 16 <= 101_000_000


def test_levels_layout_refuses_bad_arguments():
    with pytest.raises(abi.SpfError):
        abi.table_levels_layout(4, 0, 9)
    assert abi.load().spf_table_levels_layout(4, 2, 9, None, None, None) == abi.SPF_E_INVALID


@pytest.mark.parametrize("n,world,V", [(23, 4, 11), (10, 3, 17), (7, 8, 5)])
def test_levels_layout_gather_simulation(n, world, V):
    """Rank r's level rows (block order, `pitch` bytes apart) and its trailer
    placed in slot r of an all-gather: source i's row is at r * slot_bytes +
    (i - block_first[r]) * pitch, the trailers at r * slot_bytes +
    trailer_off."""
    rng = np.random.default_rng(n * 31 + world)
    pitch, slot_bytes, trailer_off = abi.table_levels_layout(n, world, V)
    bf, _, _ = abi.table_layout(n, world, V)
    gathered = np.full(world * slot_bytes, 0xEE, dtype=np.uint8)
    truth = {}
    for r in range(world):
        first, count = int(bf[r]), int(bf[r + 1] - bf[r])
        # the query's level table: [count][pitch], pad bytes arbitrary
        blk = rng.integers(0, 256, size=(count, pitch), dtype=np.uint8)
        for k in range(count):
            truth[first + k] = blk[k, :V].copy()
        slot = np.full(slot_bytes, 0xEE, dtype=np.uint8)
        slot[: count * pitch] = blk.reshape(-1)  # one contiguous copy
        slot[trailer_off : trailer_off + 16] = np.array([0, 7, count, 0], dtype=np.uint32).view(np.uint8)
        gathered[r * slot_bytes : (r + 1) * slot_bytes] = slot  # ncclAllGather slot r
    assert sorted(truth) == list(range(n))
    for i, row in truth.items():
        r = int(np.searchsorted(bf, i, side="right")) - 1
        off = r * slot_bytes + (i - int(bf[r])) * pitch
        assert (gathered[off : off + V] == row).all()
    for r in range(world):
        tr = gathered[r * slot_bytes + trailer_off : r * slot_bytes + trailer_off + 16].view(np.uint32)
        assert list(tr) == [0, 7, int(bf[r + 1] - bf[r]), 0]
