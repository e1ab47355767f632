"""lastz --chores on the device, the target half of the position filter: filter_seed_hit_by_pos (src/seed_search.c:2269-2310)
drops a raw hit unless its window lies inside the chore's target interval, and the kernels do that by clipping every list
of the position table to a constant window of hit end positions (lastz_amd/csrc/lz_common.hpp: lz_window_self,
lz_self_bounds in LZ_SELF_WINDOW mode, lz_clip_run(s)).  Checked here on the CPU: tests/emul/emul_pos_filter.cpp runs the
shared count and fill functions over a whole query, with and without the window, and the clipped counts and hit lists must
be the unclipped ones filtered by the reference's predicate, in content and in order.  The table comes from the oracle.
CPU only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import lzo
import helpers as H

U32P = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
U8P = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
U64P = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
I32P = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
#          pattern         transitions  step
SEEDS = [("1111111",       0,           1),
         ("111101101111",  1,           3)]


@pytest.fixture(scope="module")
def emul():
    d = tempfile.mkdtemp(prefix="emul_pos_filter_")
    so = os.path.join(d, "libemul_pos_filter.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so,
                           os.path.join(H.ROOT, "tests", "emul", "emul_pos_filter.cpp")])
    L = C.CDLL(so)
    L.emul_pos_filter_hits.restype = C.c_longlong
    L.emul_pos_filter_hits.argtypes = [U8P, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, I32P, U32P, C.c_int32, U32P,
                                       U32P, U32P, C.c_int, C.c_uint32, C.c_uint32, U32P, U32P, U64P, C.c_uint64, C.POINTER(C.c_int)]
    return L


def sequences():
    """target: 2,010 bases, a 20-base unit 60 times over in the middle (every word of the unit has a list of ~60 entries,
    ~20 on a table of step 3); query: three stretches of the unit in random sequence, an N among them"""
    rng = np.random.default_rng(11)
    unit = ACGT[rng.integers(0, 4, 20)]
    t = np.concatenate([ACGT[rng.integers(0, 4, 310)], np.tile(unit, 60), ACGT[rng.integers(0, 4, 500)]])
    q = ACGT[rng.integers(0, 4, 260)].copy()
    q[30:90] = np.tile(unit, 3)
    q[140:175] = np.tile(unit, 3)[7:42]
    q[200:240] = np.tile(unit, 2)
    q[215] = ord("N")
    return t, q


def codes(raw):
    """code bytes as the device has them: bits 5-6 the base, bit 7 set for a byte that cannot be in a word"""
    bits = np.full(256, 0x80, dtype=np.uint8)
    for ch, b in ((b"A", 0), (b"C", 1), (b"G", 2), (b"T", 3)):
        bits[ch[0]] = b << 5
    return np.ascontiguousarray(bits[raw])


def padded(code):
    """the count and fill functions read the window [pos - L, pos) only, but never before the array: a margin all the same"""
    return np.ascontiguousarray(np.concatenate([np.full(64, 0x80, np.uint8), code, np.full(64, 0x80, np.uint8)]))


class Search:
    def __init__(self, emul, pattern, trans, step):
        self.emul = emul
        t, q = sequences()
        self.tlen, self.qlen = len(t), len(q)
        sd = lzo.seed(pattern, trans)
        self.L = sd.length
        self.ws, self.wp = lzo.Table(t, sd, step=step).csr()
        self.ws, self.wp = np.ascontiguousarray(self.ws), np.ascontiguousarray(np.concatenate([self.wp, [0]]).astype(np.uint32))
        self.seed = (sd.length, sd.weight, sd.num_parts, np.array(sd.shift[:], dtype=np.int32), np.array(sd.mask[:], dtype=np.uint32),
                     sd.num_probes, np.array(sd.probe_xor[:], dtype=np.uint32))
        self.qbuf = padded(codes(q))
        self.cap = 400_000

    def hits(self, window=None):
        cnt, grp = np.zeros(self.qlen + 1, np.uint32), np.zeros(self.qlen + 1, np.uint32)
        keys = np.zeros(self.cap, np.uint64)
        ok = C.c_int()
        lo, hi = window if window is not None else (0, 0)
        qcode = self.qbuf[64:]                                    # (base 0 of the query; numpy keeps the margin in front of it)
        n = self.emul.emul_pos_filter_hits(qcode, self.qlen, self.tlen, *self.seed, self.ws, self.wp, int(window is not None), lo, hi,
                                           cnt, grp, keys, self.cap, C.byref(ok))
        assert 0 <= n <= self.cap
        return cnt, grp, keys[:n], bool(ok.value)


def grid(s, all_keys):
    """window edges: 0, around the seed length, around the first and last entry of the longest list (as window starts and
    as window ends of that entry), the target's length and one past it"""
    lens = np.diff(s.ws.astype(np.int64))
    w = int(np.argmax(lens))
    lst = s.wp[s.ws[w]:s.ws[w + 1]].astype(np.int64)              # descending end positions
    assert len(lst) >= (50 if s.L == 7 else 15)
    edges = {0, s.L - 1, s.L, s.L + 1, s.tlen - 1, s.tlen, s.tlen + 1}
    for e in (int(lst[0]), int(lst[-1]), int(lst[len(lst) // 2])):
        for d in (-1, 0, 1):
            edges.add(e + d)                                      # a window END on the entry's last base, one short, one past
            edges.add(e - s.L + d)                                # a window START on the entry's first base, one before, one after
    return sorted(x for x in edges if x >= 0)


@pytest.mark.parametrize("pattern,trans,step", SEEDS, ids=[p for p, _, _ in SEEDS])
def test_clipped_counts_and_hits_are_the_filtered_unclipped_ones(emul, pattern, trans, step):
    s = Search(emul, pattern, trans, step)
    cnt0, grp0, all_keys, _ = s.hits()
    assert (cnt0 == grp0).all() and int(cnt0.sum()) == len(all_keys) > 1000
    L = s.L
    pos2 = (all_keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    pos1 = (pos2 + (all_keys >> np.uint64(32)).astype(np.int64)) & 0xFFFFFFFF
    assert cnt0.max() >= (50 if L == 7 else 15)                   # lists long enough to be cut inside
    edges = grid(s, all_keys)
    cut_inside = empty = whole = 0
    for lo in edges:
        for hi in edges:
            if hi < lo:
                continue                                          # (the entry point refuses such an interval)
            cnt, grp, keys, ok = s.hits((lo, hi))
            # filter_seed_hit_by_pos, src/seed_search.c:2280-2309, on the target: pos1 -= length; discard if
            # (pos1 < tStart) || (pos1 + length > tEnd)
            p1 = pos1 - L
            discard = (p1 < lo) | (p1 + L > hi)
            want = all_keys[~discard]
            assert len(keys) == len(want) and (keys == want).all(), (pattern, lo, hi)
            want_cnt = np.bincount(pos2[~discard], minlength=s.qlen + 1).astype(np.uint32)
            assert (cnt == want_cnt).all() and (grp == want_cnt).all(), (pattern, lo, hi)
            assert ok or len(want) == 0
            if lo == hi or hi - lo < L:
                assert len(keys) == 0
            empty += len(want) == 0
            whole += len(want) == len(all_keys)
            per = np.bincount(pos2[~discard], minlength=s.qlen + 1)
            cut_inside += bool(((per > 0) & (per < cnt0)).any())
    assert empty > 10 and whole >= 4 and cut_inside > 50
