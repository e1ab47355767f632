"""Phase B's rank -> record mapping with the entry cursor (lastz_amd/csrc/lz_tile_runs.hpp: lz_tc_*), on the CPU.

A sorter wave of k_settle2 names the run of each of its 448 consecutive ranks with one wave-uniform cursor over the cursor
block's entries: the entry that holds the window's first covered rank from a count, then a step per run boundary inside each
round of 64 ranks.  tests/emul/emul_tile_cursor.cpp replays that lane by lane with the header's functions, under the
invariants of emul_tile_runs.cpp (every rank of every window covered exactly once, none past it, index in range); every rank
of every partition must come out as a plain stable partition of the array puts it.  The five cases of test_tile_runs.py run
through it as they stand there; the others are the cursor's own edges.  CPU only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import helpers as H
import test_tile_runs as R
import tile_cursor_cases as Cc

TILE, WINDOW, S2_TILE, BLOCK = R.TILE, R.WINDOW, R.S2_TILE, R.BLOCK


class Cursor:
    """libemul_tile_cursor.so behind the name test_tile_runs.check calls"""
    def __init__(self, lib):
        self.emul_tile_runs = lib.emul_tile_cursor
        self.round_steps = lib.emul_tile_cursor_round_steps


@pytest.fixture(scope="module")
def cursor():
    d = tempfile.mkdtemp(prefix="emul_tile_cursor_")
    so = os.path.join(d, "libemul_tile_cursor.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so,
                           os.path.join(H.ROOT, "tests", "emul", "emul_tile_cursor.cpp")])
    L = C.CDLL(so)
    L.emul_tile_cursor.argtypes = [R.U8P, R.U64P, C.c_uint64, C.c_uint32, C.c_uint32, R.U64P, R.U32P, R.U64P]
    L.emul_tile_cursor.restype = C.c_int
    L.emul_tile_cursor_round_steps.argtypes = []
    L.emul_tile_cursor_round_steps.restype = C.c_uint64
    return Cursor(L)


# ---- the five cases of test_tile_runs.py

@pytest.mark.parametrize("n", [1, 63, TILE - 1, TILE, TILE + 1])
def test_partial_and_whole_tiles(cursor, n):
    R.test_partial_and_whole_tiles(cursor, n)


def test_empty_partitions(cursor):
    R.test_empty_partitions(cursor)


def test_one_partition_holds_everything(cursor):
    R.test_one_partition_holds_everything(cursor)
    assert cursor.round_steps() <= 1                            # runs of a whole tile: a round meets one boundary at the most


def test_sparse_partition_moves_the_cursor_more_than_once(cursor):
    R.test_sparse_partition_moves_the_cursor_more_than_once(cursor)


def test_last_run_ends_at_a_settle_tile_boundary(cursor):
    R.test_last_run_ends_at_a_settle_tile_boundary(cursor)


# ---- the cursor's own edges

def set_partition(counts, p, want):
    """counts[t][p] = want[t] (tiles past `want`: 0), the records given to / taken from the fullest other partitions of the tile"""
    for t in range(len(counts)):
        c = want[t] if t < len(want) else 0
        while counts[t][p] != c:
            others = counts[t].copy(); others[p] = 0
            donor = int(np.argmax(others))
            k = max(int(counts[t][p]) - c, -(int(counts[t][donor]) - 1))
            assert k != 0
            counts[t][donor] += k; counts[t][p] -= k


def test_more_than_64_empty_runs_inside_one_round(cursor):
    """partition 5: ten records in tile 0, ten in tile 100, none between -- 99 empty runs between two ranks of one round"""
    rng = np.random.default_rng(11)
    ntiles = 102
    assert ntiles < BLOCK                                      # all of it inside the first cursor block
    n = ntiles * TILE - 77
    counts = np.array(R.uniform_counts(ntiles, n, rng))
    set_partition(counts, 5, [10] + [0] * 99 + [10])
    R.check(cursor, R.bins_of(counts, n, rng), 11)
    assert cursor.round_steps() >= 100


def test_runs_that_start_on_a_rounds_first_and_last_rank(cursor):
    """partition 9: runs of 64, 63, 1 and 500 records -- the second starts on rank 64 (round 1's first), the third on rank 127
    (its last), the fourth on round 2's first; and the same shifted into the window of the second sorter wave"""
    rng = np.random.default_rng(12)
    ntiles, n = 6, 6 * TILE - 1
    for lead in ([], [WINDOW]):
        counts = np.array(R.uniform_counts(ntiles, n, rng))
        set_partition(counts, 9, lead + [64, 63, 1, 500])
        R.check(cursor, R.bins_of(counts, n, rng), 12)


def test_window_that_starts_on_a_blocks_bounding_entry(cursor):
    """partition 33 has 2 x 448 records in tiles 0 .. 126, so the run of tile 127 -- the bounding entry of the first cursor
    block -- starts on the first rank of the third sorter wave's window: that block is behind the window, the next one
    starts on it"""
    rng = np.random.default_rng(13)
    ntiles = BLOCK + 4
    n = ntiles * TILE - 3000
    counts = np.array(R.uniform_counts(ntiles, n, rng))
    want = [7] * (BLOCK - 2) + [14] + [50, 0, 61, 9, 300]
    assert len(want) == ntiles and sum(want[:BLOCK - 1]) == 2 * WINDOW
    set_partition(counts, 33, want)
    stats = R.check(cursor, R.bins_of(counts, n, rng), 13)
    assert stats[0] >= 1


def test_partition_whose_last_window_is_partial(cursor):
    """partition 200: one settle tile, three windows and 100 records -- the fourth sorter wave's last window holds 100 ranks"""
    rng = np.random.default_rng(14)
    ntiles, n = 5, 5 * TILE - 9
    counts = np.array(R.uniform_counts(ntiles, n, rng))
    want = [2000, 1500, 1700, 1000, S2_TILE + 3 * WINDOW + 100 - 6200]
    assert sum(want) % WINDOW == 100 and all(c > 0 for c in want)
    set_partition(counts, 200, want)
    R.check(cursor, R.bins_of(counts, n, rng), 14)


def test_gap_pair(cursor):
    """the partition bytes of test_gpu_tile_cursor.py's A/G pair in discovery order: windows that span blocks of empty runs"""
    bins = Cc.gap_partition_bytes()
    assert len(bins) == 5_073_106 and Cc.longest_gap(bins) >= BLOCK
    stats = R.check(cursor, bins, 15)
    assert stats[0] >= 2                                       # cursor moves inside one window
