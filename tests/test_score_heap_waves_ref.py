"""The key tile of score_forest_heap at either block size, checked without a
GPU.

A tile of R * 256 rows (R = rows per thread * threads / 256) keeps, per
feature slab, row j in 32-bit word j mod P, half j / P, with P = R * 128
(v4_tile_slot, forest_kernels.hip). Thread tid of a BT-thread block owns rows
tid, tid + BT, ... The 512-row tile is walked either by 256 threads with two
rows each or by 512 threads with one: the records' slab offsets, and so the
pack, are shared, which needs the two to agree on where every row lies.
Here: a numpy mirror of the map, that it fills the slab exactly, that the two
block sizes agree, and that no 32-lane group of a wave meets a bank twice,
whatever features its lanes ask for.
"""

import numpy as np
import pytest

BANKS = 64  # 4-byte LDS banks of a CU


def tile_slot(j, tile_rows):
    """Row j of the tile -> (word, half) inside one slab."""
    P = tile_rows // 2
    j = np.asarray(j)
    return j % P, j // P


def owned_rows(threads, rpt):
    """[threads, rpt]: the tile rows thread tid stages, walks and stores."""
    return np.arange(threads)[:, None] + np.arange(rpt)[None, :] * threads


# (threads, rows per thread) of the instantiations
_GEOMETRIES = [(256, 1), (256, 2), (512, 1)]


@pytest.mark.parametrize("tile_rows", [256, 512, 1024])
def test_slot_map_fills_the_slab(tile_rows):
    """1024 rows is a property of the map alone: no kernel runs that tile."""
    word, half = tile_slot(np.arange(tile_rows), tile_rows)
    assert word.min() == 0 and word.max() == tile_rows // 2 - 1
    assert set(half.tolist()) == {0, 1}
    elem = word * 2 + half  # 16-bit element offset inside the slab
    assert np.array_equal(np.sort(elem), np.arange(tile_rows))


@pytest.mark.parametrize("threads,rpt", _GEOMETRIES)
def test_threads_own_every_row_once(threads, rpt):
    rows = owned_rows(threads, rpt)
    assert np.array_equal(np.sort(rows.reshape(-1)),
                          np.arange(threads * rpt))


def test_512_row_tile_is_one_map_for_both_block_sizes():
    """Element offset of every row, reached through the owner thread."""
    maps = []
    for threads, rpt in ((256, 2), (512, 1)):
        rows = owned_rows(threads, rpt)
        tile_rows = rpt * threads
        assert tile_rows == 512
        word, half = tile_slot(rows, tile_rows)
        elem = np.empty(tile_rows, dtype=np.int64)
        elem[rows.reshape(-1)] = (word * 2 + half).reshape(-1)
        maps.append(elem)
    assert np.array_equal(maps[0], maps[1])
    # rows 256..511, which the upper four waves own, are the high halves of
    # the words whose low halves rows 0..255 hold
    assert np.array_equal(maps[1][256:], maps[1][:256] + 1)


@pytest.mark.parametrize("threads,rpt", _GEOMETRIES)
def test_half_waves_read_distinct_banks(threads, rpt):
    """ds_read_u16 of the key: byte address slab * tile_rows * 2 + element
    * 2 with a slab of the lane's own choosing. A slab is a whole number of
    bank rows, so the bank is that of the word alone."""
    tile_rows = threads * rpt
    assert (tile_rows * 2) % (BANKS * 4) == 0
    rs = np.random.RandomState(threads + rpt)
    rows = owned_rows(threads, rpt)
    for r in range(rpt):
        word, half = tile_slot(rows[:, r], tile_rows)
        for slabs in (np.zeros(threads, dtype=np.int64),
                      rs.randint(0, 33, size=threads)):
            byte = slabs * tile_rows * 2 + word * 4 + half * 2
            bank = (byte // 4) % BANKS
            groups = bank.reshape(threads // 32, 32)
            assert all(len(set(g.tolist())) == 32 for g in groups), \
                (threads, rpt, r)
