"""Phase B's gather of a partition from tiles that were sorted in place (lastz_amd/csrc/lz_tile_runs.hpp), on the CPU.

k_partition sorts every tile of 16384 hits by partition where it lies; partition p is then one run per tile, and a
sorter wave of k_settle2 finds the records of 448 consecutive ranks through a cursor over the tiles' (first rank,
address) table.  tests/emul/emul_tile_runs.cpp replays that procedure lane by lane with the header's arithmetic; for a
count matrix [ntiles][256] turned into a random tagged array, every rank of every partition must come out as a plain
stable partition of the array puts it.  CPU only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import helpers as H

TILE = 16384                                                 # lz_tile_runs.hpp: LZ_PP_TILE_HOST
WINDOW, SORTW = 448, 12                                      # settle_kernels.hip: 64 * LZ_S2_ROUNDS, LZ_S2_SORTW
S2_TILE = WINDOW * SORTW                                     # LZ_S2_TILE = 5376
BLOCK = 128                                                  # lz_tile_runs.hpp: LZ_TR_BLOCK (a block covers BLOCK - 1 tiles)
U8P = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
U32P = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
U64P = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def emul():
    d = tempfile.mkdtemp(prefix="emul_tile_runs_")
    so = os.path.join(d, "libemul_tile_runs.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so,
                           os.path.join(H.ROOT, "tests", "emul", "emul_tile_runs.cpp")])
    L = C.CDLL(so)
    L.emul_tile_runs.argtypes = [U8P, U64P, C.c_uint64, C.c_uint32, C.c_uint32, U64P, U32P, U64P]
    L.emul_tile_runs.restype = C.c_int
    return L


def bins_of(counts, n, rng):
    """a partition byte per record: tile t holds counts[t][p] records of partition p (the last tile n - (ntiles - 1) TILE
    of them), in random order inside the tile"""
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.shape[1] == 256 and (counts[:-1].sum(axis=1) == TILE).all() and counts.sum() == n
    out = np.empty(n, dtype=np.uint8)
    for t, row in enumerate(counts):
        b = np.repeat(np.arange(256, dtype=np.uint8), row)
        rng.shuffle(b)
        out[t * TILE:t * TILE + len(b)] = b
    return out


def check(emul, bins, seed):
    n = len(bins)
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, 1 << 55, n, dtype=np.uint64) | (bins.astype(np.uint64) << np.uint64(55))    # tagged, as k_scan_hits2 leaves them
    out = np.zeros(n, dtype=np.uint64)
    bin_base = np.zeros(257, dtype=np.uint32)
    stats = np.zeros(3, dtype=np.uint64)
    assert emul.emul_tile_runs(bins, vals, n, WINDOW, SORTW, out, bin_base, stats) == 0
    want = vals[np.argsort(bins, kind="stable")]
    assert (out == want).all()
    assert (bin_base == np.concatenate([[0], np.cumsum(np.bincount(bins, minlength=256))])).all()
    assert stats[1] <= stats[2] + 1                            # a wave's block loads: bounded by the tiles, however sparse
    return [int(s) for s in stats]


def uniform_counts(ntiles, n, rng, empty=()):
    """every tile's records spread over the partitions at random (none in the partitions of `empty`)"""
    p = np.ones(256); p[list(empty)] = 0; p /= p.sum()
    return [rng.multinomial(min(TILE, n - t * TILE), p) for t in range(ntiles)]


@pytest.mark.parametrize("n", [1, 63, TILE - 1, TILE, TILE + 1])
def test_partial_and_whole_tiles(emul, n):
    rng = np.random.default_rng(n)
    check(emul, bins_of(uniform_counts((n + TILE - 1) // TILE, n, rng), n, rng), n)


def test_empty_partitions(emul):
    rng = np.random.default_rng(2)
    n = 5 * TILE + 1234
    bins = bins_of(uniform_counts(6, n, rng, empty=(0, 17, 255)), n, rng)
    assert not np.isin(bins, (0, 17, 255)).any()
    check(emul, bins, 2)


def test_one_partition_holds_everything(emul):
    """a run of a whole tile is longer than a settle tile (5376) and spans several of them"""
    n = 3 * TILE + 700
    assert TILE > 3 * S2_TILE
    for p in (0, 200, 255):
        check(emul, np.full(n, p, dtype=np.uint8), p)


def test_sparse_partition_moves_the_cursor_more_than_once(emul):
    """partition 77 has one record every ~100 tiles: its few ranks are one window that spans more tiles than two cursor
    blocks, so the cursor moves several times inside the window"""
    rng = np.random.default_rng(3)
    ntiles = 3 * BLOCK + 40
    n = ntiles * TILE - 5000
    counts = uniform_counts(ntiles, n, rng, empty=(77,))
    holders = list(range(5, ntiles, 100)) + [ntiles - 1]
    for t in holders:
        donor = int(np.argmax(counts[t]))
        counts[t][donor] -= 1; counts[t][77] += 1
    stats = check(emul, bins_of(counts, n, rng), 3)
    assert stats[0] >= 3                                       # moves inside one window


def test_last_run_ends_at_a_settle_tile_boundary(emul):
    """partition 9 holds exactly two settle tiles of records, the last of them ending its last run"""
    rng = np.random.default_rng(4)
    ntiles, n = 4, 4 * TILE
    counts = np.array(uniform_counts(ntiles, n, rng, empty=(9,)))
    want = [S2_TILE, 3000, 0, S2_TILE - 3000]
    for t, c in enumerate(want):
        left = c
        while left:                                            # take the records from the fullest partitions of the tile
            others = counts[t].copy(); others[9] = 0
            donor = int(np.argmax(others)); k = min(left, int(counts[t][donor]) - 1)
            counts[t][donor] -= k; counts[t][9] += k; left -= k
    assert counts[:, 9].sum() == 2 * S2_TILE
    check(emul, bins_of(counts, n, rng), 4)
