"""The target context of the fused scan kernel (lastz_amd/csrc/lz_lut.hpp: wctx, 32 bytes of the target's 2-bit array
per table entry) and its tagged hit record, on the CPU.

For every end position pos1 of a short target -- both sequence ends, all four phases of pos1 inside a byte -- the two
16-byte windows that lz_wctx_windows takes from the entry lz_wctx_make built must be the windows lz_scan_fetch
(scan_kernels.hip) takes from the half-overlapping blocks, restated here in numpy over the same arrays.  And the tagged
record with its tag cleared must be lz_hit_record(key, summ), for SLOW and other summaries, the tag being bits 8..15
of the diagonal.  CPU only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import helpers as H

PAD2 = 128                                                   # lz_lut.hpp: LZ_PAD2
SUMM_SLOW = 0x10000                                          # lz_common.hpp: LZ_SUMM_SLOW
U8P = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
U32P = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
U64P = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def emul():
    d = tempfile.mkdtemp(prefix="emul_fused_")
    so = os.path.join(d, "libemul_fused.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so,
                           os.path.join(H.ROOT, "tests", "emul", "emul_fused.cpp")])
    L = C.CDLL(so)
    L.emul_wctx_windows.argtypes = [U8P, U32P, C.c_uint32, U8P, U8P, U8P]
    L.emul_tagged_records.argtypes = [U64P, U32P, C.c_uint32, U64P, U64P, U32P, U64P]
    return L


def two_bit_arrays(tlen, seed):
    """the plain 2-bit array of a target of tlen bases as slot_encode sizes and k_pack2 fills it (base i in bits
    2 * ((i + PAD2) & 3) of byte (i + PAD2) >> 2, Gray-coded; zero outside), and its half-overlapping 64-byte blocks
    (k_overlap32: block k = bytes [32 k, 32 k + 64))"""
    rng = np.random.default_rng(seed)
    nmask = (tlen + 2 * PAD2 + 7) // 8 + 16
    two = np.zeros(nmask * 2 + 96, dtype=np.uint8)
    codes = rng.integers(0, 4, tlen)
    gray = codes ^ (codes >> 1)
    for i in range(tlen):
        two[(i + PAD2) >> 2] |= gray[i] << (2 * ((i + PAD2) & 3))
    nb = (nmask * 2 + 31) // 32
    two_x = np.zeros(nb * 64 + 64, dtype=np.uint8)
    for k in range(nb):
        blk = two[32 * k:32 * k + 64]
        two_x[64 * k:64 * k + len(blk)] = blk
    return two, two_x


def scan_fetch_windows(two_x, pos1):
    """lz_scan_fetch's target loads: (left, right) 16-byte windows of the hit that ends at pos1"""
    stl, st_r = pos1 - 1 + PAD2, pos1 + PAD2
    bl, br = (stl >> 2) - 15, st_r >> 2
    ol = bl + (bl & ~31)
    return two_x[ol:ol + 16], two_x[ol + (br - bl):ol + (br - bl) + 16], bl, br


@pytest.mark.parametrize("tlen,seed", [(19, 1), (203, 2), (1024, 3), (4099, 4)])
def test_windows_from_wctx_are_the_windows_of_scan_fetch(emul, tlen, seed):
    two, two_x = two_bit_arrays(tlen, seed)
    pos1 = np.arange(1, tlen + 1, dtype=np.uint32)             # every end position a table entry can hold, both ends included
    n = len(pos1)
    ent, left, right = (np.zeros((n, k), dtype=np.uint8) for k in (32, 16, 16))
    emul.emul_wctx_windows(two, pos1, n, ent, left, right)
    phases = set()
    for k, p in enumerate(pos1):
        wl, wr, bl, br = scan_fetch_windows(two_x, int(p))
        assert br - bl in (15, 16)
        assert (ent[k] == two[bl:bl + 32]).all(), p
        assert (left[k] == wl).all() and (left[k] == two[bl:bl + 16]).all(), p
        assert (right[k] == wr).all() and (right[k] == two[br:br + 16]).all(), p
        phases.add(((int(p) + PAD2) & 3, br - bl))
    assert {ph for ph, _ in phases} == {0, 1, 2, 3} and {d for _, d in phases} == {15, 16}
    assert left.any() and right.any()                            # (the windows do hold sequence, not just padding)


def hit_record(key, summ):
    """lz_hit_record, restated"""
    pos2, diag = key & 0xFFFFFFFF, key >> 32
    slow = bool(summ & SUMM_SLOW)
    payload = (diag >> 16) if slow else (summ & 0xFFFF)
    return pos2 | ((diag & 0xFF) << 31) | (payload << 39) | ((1 << 63) if slow else 0)


def test_tagged_record_is_the_record_plus_its_partition(emul):
    rng = np.random.default_rng(9)
    n = 4000
    pos2 = rng.integers(1, 1 << 31, n, dtype=np.uint64)
    diag = rng.integers(0, 1 << 32, n, dtype=np.uint64)        # (pos1 - pos2 mod 2^32: negative diagonals too)
    diag[:8] = [0, 0xFFFFFFFF, 0xFF00, 0x00FF, 0xFFFF0000, 0x8000, 0x7FFFFFFF, 0x80000000]
    key = (diag << np.uint64(32)) | pos2
    summ = rng.integers(0, 1 << 16, n, dtype=np.uint32)
    summ[::3] |= SUMM_SLOW                                      # SLOW and fast summaries
    summ[5] = 0                                                 # the provisional record of a queued hit
    tagged, plain, untagged = (np.zeros(n, dtype=np.uint64) for _ in range(3))
    tag = np.zeros(n, dtype=np.uint32)
    emul.emul_tagged_records(key, summ, n, tagged, plain, tag, untagged)
    for k in range(n):
        want = hit_record(int(key[k]), int(summ[k]))
        assert int(plain[k]) == want and int(untagged[k]) == want, k
        assert int(tag[k]) == (int(diag[k]) >> 8) & 0xFF, k
        assert int(tagged[k]) == want | (int(tag[k]) << 55), k
        assert (want >> 55) & 0xFF == 0, k                     # bits 55..62 are free in the record
