"""lastz --self / --band on the device: the raw hits the reference drops (seed_hit_below_diagonal and the band test,
src/seed_search.c:841-848, 903-908, 2052-2235) are, for each query position, the hits outside an interval of target
positions (lastz_amd/csrc/lz_common.hpp, lz_self_bounds), and the kernels clip every list of the position table to
it (lz_clip_run(s)).  Checked here on the CPU against a plain restatement of the reference's rule: exhaustively for
every pair of positions of small sequences, then for whole searches' raw hits.  Also the C ABI of
lzgpu_seed_hit_search_self.  CPU only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from lastz_amd import lzgpu, seqio
import helpers as H

MODE_SAME, MODE_OPP, MODE_OPP_PARTS = 1, 2, 3
U32P = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def emul():
    d = tempfile.mkdtemp(prefix="emul_self_")
    so = os.path.join(d, "libemul_self.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so,
                           os.path.join(H.ROOT, "tests", "emul", "emul_self.cpp")])
    L = C.CDLL(so)
    L.emul_self_bounds.argtypes = [C.c_uint32] * 4 + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, U32P, C.c_uint32, U32P, U32P]
    L.emul_clip_run.argtypes = [U32P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, U32P]
    L.emul_self_hits.restype = C.c_longlong
    L.emul_self_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                 C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, U32P, U32P, C.c_void_p, C.c_void_p,
                                 C.c_uint64, C.POINTER(C.c_longlong)]
    return L


# ---- the reference's rule, restated plainly (positions are hit END positions, L the seed length)
def lookup_partition(seps, pos):
    """src/sequences.c lookup_partition: the partition ix with sepBefore[ix] < pos < sepBefore[ix + 1]"""
    for ix in range(len(seps) - 1):
        if seps[ix] < pos < seps[ix + 1]:
            return ix
    raise AssertionError("position %d is on a separator or outside the partitions" % pos)


def kept(pos1, pos2, same, L, len2, band, seps1, seps2):
    if same:                                                  # seed_hit_below_diagonal, same strand
        if pos1 >= pos2:
            return False
    else:
        p1, p2 = pos1 - L, pos2 - L
        if not seps2:
            below = p1 >= (len2 - 1) - p2
        else:
            ix1, ix2 = lookup_partition(seps1, p1), lookup_partition(seps2, p2)
            if ix1 != ix2:
                below = ix1 >= ix2
            else:
                below = p1 >= (seps2[ix2] + seps2[ix2 + 1]) - p2      # sepBefore + sepAfter of the partition
        if below:
            return False
    if same and band > 0 and pos2 - pos1 > band:              # find_table_matches, the band test
        return False
    return True


def layout(records):
    """a [multi] sequence's layout (src/sequences.c:1896-1931): NUL, record, NUL, record, ..., final separator = len"""
    if records is None:
        return None, []
    seps, at = [0], 0
    for n in records:
        at += n + 1
        seps.append(at)
    return at, seps                                           # (length: the last separator is one past the end)


def valid_ends(n, L, seps):
    """end positions whose L-base window holds no separator"""
    bad = np.zeros(n + 1, dtype=bool)
    for s in seps:
        if s < n:
            bad[s] = True
    c = np.concatenate([[0], np.cumsum(bad[:n])])
    ends = np.arange(L, n + 1)
    return ends[(c[ends] - c[ends - L]) == 0]


CONFIGS = [("none", None, 160), ("one", [150], None), ("four", [70, 9, 22, 61], None)]


@pytest.mark.parametrize("parts,records,n0", CONFIGS, ids=[c[0] for c in CONFIGS])
@pytest.mark.parametrize("L", [8, 19])
@pytest.mark.parametrize("band", [0, 1, 37])
@pytest.mark.parametrize("same", [True, False], ids=["same", "opposite"])
def test_self_bounds_exhaustive(emul, parts, records, n0, L, band, same):
    n, seps = layout(records)
    if n is None:
        n = n0
    ends = valid_ends(n, L, seps)
    assert len(ends) > 20
    mode = MODE_SAME if same else (MODE_OPP_PARTS if seps else MODE_OPP)
    sep = np.array(seps if seps else [0], dtype=np.uint32)
    pos2 = ends.astype(np.uint32)
    lo, hi = np.zeros_like(pos2), np.zeros_like(pos2)
    emul.emul_self_bounds(mode, L, n, band, sep.ctypes.data, len(seps), sep.ctypes.data, len(seps), pos2, len(pos2), lo, hi)
    n_kept = 0
    for k, p2 in enumerate(ends):
        want = np.array([kept(int(p1), int(p2), same, L, n, band, seps, seps) for p1 in ends])
        got = (ends >= lo[k]) & (ends < hi[k])
        assert (got == want).all(), (int(p2), int(lo[k]), int(hi[k]), ends[got != want][:5])
        n_kept += int(want.sum())
    assert 0 < n_kept < len(ends) ** 2


def test_clip_run_every_interval(emul):
    """lz_clip_run on descending lists (the table's order), every [lo, hi) against a plain filter"""
    rng = np.random.default_rng(1)
    for length in (0, 1, 2, 3, 7, 16, 33):
        vals = np.sort(rng.choice(np.arange(1, 200), size=length, replace=False))[::-1].astype(np.uint32)
        wpos = np.concatenate([np.array([999, 998], dtype=np.uint32), vals, np.array([5], dtype=np.uint32)])
        out = np.zeros(2, dtype=np.uint32)
        for lo in range(0, 202, 3):
            for hi in range(lo, 203, 2):
                emul.emul_clip_run(wpos, 2, 2 + length, lo, hi, out)
                keep = [i for i in range(2, 2 + length) if lo <= wpos[i] < hi]
                assert int(out[1]) == len(keep)
                if keep:
                    assert int(out[0]) == keep[0] and keep == list(range(keep[0], keep[0] + len(keep)))


def _codes(raw):
    """code bytes as the device has them: bits 5-6 the base, bit 7 set for a byte that cannot be in a word"""
    bits = np.full(256, 0x80, dtype=np.uint8)
    for ch, b in ((b"A", 0), (b"C", 1), (b"G", 2), (b"T", 3)):
        bits[ch[0]] = b << 5
        bits[ch[0] | 0x20] = b << 5
    return bits[raw]


def _repetitive(n, seed):
    """random bases with copies (direct and inverted) and a low-complexity run: long lists in the table"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    s = acgt[rng.integers(0, 4, n)]
    for _ in range(6):
        a, b, ln = int(rng.integers(0, n - 300)), int(rng.integers(0, n - 300)), int(rng.integers(40, 300))
        blk = s[a:a + ln].copy()
        s[b:b + ln] = seqio.revcomp(blk) if rng.random() < 0.5 else blk
    s[n // 3:n // 3 + 120] = np.frombuffer(b"ACA" * 40, dtype=np.uint8)
    s[n // 2:n // 2 + 90] = np.frombuffer(b"TGT" * 30, dtype=np.uint8)        # (its reverse complement is the run above)
    s[2 * n // 3:2 * n // 3 + 7] = ord("N")
    return s


@pytest.mark.parametrize("case", ["same", "same-band", "opposite", "opposite-multi"])
def test_count_and_fill_keep_what_the_reference_keeps(emul, case):
    """the emulated count and fill with the clip = the unclipped raw hits, filtered by the restatement, in order"""
    L, band = 8, (150 if case == "same-band" else 0)
    base = _repetitive(2400, seed=7)
    if case == "opposite-multi":
        records = [900, 14, 30, 1450]
        n, seps = layout(records)
        t = np.zeros(n, dtype=np.uint8)
        q = np.zeros(n, dtype=np.uint8)
        at = 0
        for k, ln in enumerate(records):
            t[seps[k] + 1:seps[k + 1]] = base[at:at + ln]
            q[seps[k] + 1:seps[k + 1]] = seqio.revcomp(base[at:at + ln])       # partitions reverse-complemented one by one
            at += ln
    else:
        n, seps, t = len(base), [], base
        q = base if case.startswith("same") else seqio.revcomp(base)
    same = case.startswith("same")
    mode = MODE_SAME if same else (MODE_OPP_PARTS if seps else MODE_OPP)
    tc, qc = np.ascontiguousarray(_codes(t)), np.ascontiguousarray(_codes(q))
    sep = np.array(seps if seps else [0], dtype=np.uint32)
    cap = 4_000_000
    cnt, grp = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
    keys, allk = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
    n_all = C.c_longlong()
    nk = emul.emul_self_hits(tc.ctypes.data, qc.ctypes.data, n, L, mode, band, sep.ctypes.data, len(seps),
                             sep.ctypes.data, len(seps), cnt, grp, keys.ctypes.data, allk.ctypes.data, cap, C.byref(n_all))
    assert nk <= cap and n_all.value <= cap
    assert (cnt == grp).all()
    assert int(cnt.sum()) == nk
    allk = allk[:n_all.value]
    p2 = (allk & 0xFFFFFFFF).astype(np.int64)
    p1 = (p2 + (allk >> 32).astype(np.int64)) & 0xFFFFFFFF
    keep = np.array([kept(int(a), int(b), same, L, n, band, seps, seps) for a, b in zip(p1, p2)], dtype=bool)
    assert (keys[:nk] == allk[keep]).all()
    assert 0 < nk < n_all.value
    # several hits per list: the clip did cut runs, not only whole lists
    assert cnt.max() > 20


def test_self_entry_point_exported_and_args_layout():
    import __graft_entry__ as g
    if not os.path.exists(lzgpu.LIB_PATH):
        g.build()
    lib = lzgpu.Lib()
    assert hasattr(lib.L, "lzgpu_seed_hit_search_self")
    assert "lzgpu_seed_hit_search_self" in lzgpu.EXPORTS
    src = '#include "lzgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n",' \
          'sizeof(lz_self_args),offsetof(lz_self_args,same_strand),offsetof(lz_self_args,band_width),offsetof(lz_self_args,sep1),' \
          'offsetof(lz_self_args,n_sep1),offsetof(lz_self_args,sep2),offsetof(lz_self_args,n_sep2));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(H.ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    S = lzgpu.SelfArgs
    assert got == [C.sizeof(S), S.same_strand.offset, S.band_width.offset, S.sep1.offset, S.n_sep1.offset,
                   S.sep2.offset, S.n_sep2.offset]
