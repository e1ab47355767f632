"""Dynamic masking of the position table (lastz --masking=<count>), stated for the tests of every tier.

lastz masks a run of target bases [s, e) (origin 0, end-exclusive: the CORE) in two steps (src/masking.c:303-358): it reports
the run to mask_seed_position_table, widened by L - 1 on both sides and clamped to the sequence (src/lastz.c:3797-3801, widen()
below), and then writes 'x' over the core.  mask_seed_positions (src/pos_table.c:814-887) removes the entries p -- a word's END
position -- with start + L <= p <= end of the widened interval that are in the table, order kept.

The expected value is independent of that routine: 'x' maps to -1 under upperCharToBits, every window inside the widened
interval overlaps the core, and every window that overlaps the core lies inside the widened interval -- so the masked table is
the table BUILT from the masked bytes (oracle.lzo.Table), list order included.

A case is a target, a seed, a table geometry and one or more EVENTS.  An event is what one (query, strand) produces: a list of
cores, or of widened intervals given directly (no byte changes then).  All targets carry a run of N and a lower-case run."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


DEFAULT = "1110100110010101111"           # 12of19
L12 = "111101101111"


def widen(s, e, L, tlen):
    """the core [s, e), origin 0 -> the interval remove_interval_seeds hands to mask_seed_position_table (origin 0, end-exclusive)"""
    b, e1 = s + 1, e                       # origin 1, inclusive
    b = 1 if b < L else b - (L - 1)
    e1 = tlen if e1 >= tlen - (L - 1) else e1 + (L - 1)
    return (b - 1, e1)


def _target(tlen, seed):
    rng = np.random.default_rng(seed)
    t = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, tlen)].copy()
    t[tlen // 3: tlen // 3 + 37] = ord("N")
    t[tlen // 2: tlen // 2 + 100] |= 0x20
    return t


def _many(tlen, L):
    """3000 cores whose widened intervals are 23 to 60 bases long, every 66 bases: more ranges than a workgroup has lanes"""
    rng = np.random.default_rng(5)
    out = []
    for k in range(3000):
        s = 40 + 66 * k + int(rng.integers(0, 6))
        out.append((s, s + int(rng.integers(1, 39))))
    assert out[-1][1] + L < tlen
    return out


# name: tlen, seed, pattern, with_trans, step, table start, table end (0: tlen), events.  An event: ("core", [(s, e)]) or ("direct", [(start, end)])
CASES = {
    "clamps":      (40000, 11, DEFAULT, 1, 1, 0, 0, [("core", [(0, 30), (5, 9), (39975, 40000)])]),
    "core_of_one": (40000, 12, DEFAULT, 1, 1, 0, 0, [("core", [(25000, 25001)])]),
    "short":       (40000, 13, DEFAULT, 1, 1, 0, 0, [("direct", [(1000, 1010), (0, 18), (39990, 40000)]), ("core", [(700, 701)])]),
    "overlap":     (40000, 14, DEFAULT, 1, 1, 0, 0, [("core", [(5000, 5100), (5050, 5200), (9000, 9050), (9000, 9050)])]),
    "list_ends":   (40000, 15, "1111", 0, 1, 0, 0, [("list", "ends")]),
    "list_empty":  (40000, 16, DEFAULT, 1, 1, 0, 0, [("list", "single")]),
    "whole":       (40000, 17, DEFAULT, 1, 1, 0, 0, [("core", [(0, 40000)])]),
    "many":        (200000, 18, L12, 1, 1, 0, 0, [("many", None)]),
    "long":        (120000, 19, DEFAULT, 1, 1, 0, 0, [("core", [(10000, 110000)])]),
    # the N run is [13333, 13370), the lower-case run [20000, 20100): cores inside them, across their edges and around them
    "bytes":       (40000, 20, DEFAULT, 1, 1, 0, 0, [("core", [(13340, 13350), (13365, 13380), (13300, 13334), (19990, 20010), (20050, 20060), (20095, 20130)])]),
    "step3":       (40000, 21, L12, 1, 3, 0, 0, [("core", [(0, 7), (3000, 3040), (9001, 9002), (39990, 40000)])]),
    "step20":      (40000, 22, DEFAULT, 1, 20, 0, 0, [("core", [(0, 7), (3000, 3040), (9001, 9002), (12000, 12500), (39990, 40000)])]),
    "inside":      (40000, 23, DEFAULT, 1, 1, 5000, 30000, [("core", [(4990, 5010), (29990, 30020), (100, 200), (35000, 35100), (12000, 12050), (4970, 4982)])]),
    "two_events":  (40000, 24, DEFAULT, 1, 1, 0, 0, [("core", [(8000, 8100), (30000, 30001)]), ("core", [(8050, 8200), (7990, 8010), (30000, 30001)])]),
}
SEARCHED = ("clamps", "list_ends", "two_events")          # sparse lists, long lists, two events


def geometry(name):
    tlen, _, pattern, trans, step, start, end, _ = CASES[name]
    return dict(tlen=tlen, pattern=pattern, trans=trans, step=step, start=start, end=end or tlen, L=len(pattern))


def target(name):
    return _target(CASES[name][0], CASES[name][1])


def table(lzo, name, t):
    g = geometry(name)
    return lzo.Table(t, lzo.seed(g["pattern"], g["trans"]), step=g["step"], start=g["start"], end=g["end"])


def _list_cores(lzo, name, which):
    """cores of one base that take single entries out of one list of the unmasked table"""
    g = geometry(name)
    ws, wp = table(lzo, name, target(name)).csr()
    n = np.diff(ws.astype(np.int64))
    if which == "ends":                                   # the first, the last and a middle entry of the longest list
        w = int(np.argmax(n))
        lst = wp[ws[w]: ws[w + 1]]
        assert len(lst) >= 50
        ps = [int(lst[0]), int(lst[-1]), int(lst[len(lst) // 2])]
    else:                                                 # the only entry of a list, three times: the lists become empty
        ps = [int(wp[ws[w]]) for w in np.flatnonzero(n == 1)[[0, 100, 1000]]]
    return [(p - 1, p) for p in ps], ps


def events(lzo, name):
    """[(widened intervals [(start, end)], cores [(s, e)])] per event"""
    return _once(("events", name), lambda: _events(lzo, name))


def _events(lzo, name):
    g = geometry(name)
    out = []
    for kind, arg in CASES[name][7]:
        if kind == "direct":
            out.append((list(arg), []))
            continue
        cores = arg if kind == "core" else _many(g["tlen"], g["L"]) if kind == "many" else _list_cores(lzo, name, arg)[0]
        out.append(([widen(s, e, g["L"], g["tlen"]) for s, e in cores], list(cores)))
    return out


def expected(lzo, name):
    """per event: the masked bytes and the table built from them, (masked target, oracle Table) -- computed once, not to be changed"""
    return _once(("expected", name), lambda: [(t, table(lzo, name, t)) for t in masked_targets(lzo, name)])


def masked_targets(lzo, name):
    """the target after each event: the cores of the events so far are 'x'"""
    t = target(name)
    out = []
    for _, cores in events(lzo, name):
        t = t.copy()
        for s, e in cores:
            t[s:e] = ord("x")
        out.append(t)
    return out


def query(name, rev=False):
    """5 kbp of the target around the first core, every 13th base changed (HSPs on both sides of a masked run)"""
    from lastz_amd import seqio
    t = target(name)
    at = {"clamps": 0, "list_ends": 17000, "two_events": 6000}[name]
    q = t[at: at + 5000].copy()
    q[::13] = np.frombuffer(b"ACGT", dtype=np.uint8)[(np.arange(len(q[::13])) + 1) % 4]
    return seqio.revcomp(q) if rev else q


def emul():
    """tests/emul/emul_mask.cpp compiled into a temporary directory"""
    def make():
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        so = os.path.join(tempfile.mkdtemp(prefix="emul_mask_"), "libemul_mask.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(root, "tests", "emul", "emul_mask.cpp")])
        lib = C.CDLL(so)
        lib.emul_table_mask.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
        return lib
    return _once("emul", make)


def emul_mask(ws, wp, intervals, L, tlen):
    """the pass on copies of a CSR table -> (return code, wstart, wpos)"""
    ws = np.ascontiguousarray(ws, dtype=np.uint32).copy()
    wp = np.ascontiguousarray(wp, dtype=np.uint32).copy()
    n = len(wp)
    if n == 0:
        wp = np.zeros(1, dtype=np.uint32)
    iv = np.ascontiguousarray(np.array(intervals, dtype=np.uint32).reshape(-1, 2))
    kept = C.c_uint32()
    rc = emul().emul_table_mask(ws.ctypes.data, len(ws) - 1, wp.ctypes.data, n, iv.ctypes.data, len(iv), L, tlen, C.byref(kept))
    return rc, ws, wp[:kept.value]
