"""Exact-match extension of seed hits (lastz --exact=<length>): one table of cases for the three tiers -- the serial
statement and the GPU's decomposition on the CPU (tests/test_exact_cases.py, tests/emul/emul_exact.cpp), the goldens from
the pristine binary (tests/golden/make_exact_golden.py), and lzgpu_seed_hit_search_exact with the command line on the GPU
(tests/test_gpu_exact.py, tests/test_gpu_exact_cli.py).

Sequences come from seeded generators; nothing large is committed.  Every case names a seed, a threshold and, where given,
a hit capacity, and `reach`: the branch counters of the serial routine that must not be zero (emul_exact.cpp's order:
windows not matching, left ends clipped by diagEnd, hits dropped, dropped or clipped by another diagonal's extent, runs
past the cap) -- what keeps the case from testing nothing."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from lastz_amd import seqio
import self_cases as S

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
DEFAULT_SEED = "1110100110010101111"                       # 12of19
CAP = 128                                                  # lz_exact.hpp: LZ_EX_CAP
COUNTERS = ("not_matching", "clipped", "dropped", "other_diagonal", "past_cap")
WHOLE = 1 << 28                                            # the hit capacity that chunks nothing here
GOLDEN_FORMAT = "--format=general-:name1,start1,end1,name2,start2,end2,strand2,score"


def match_bits():
    """hp->charToBits of a DNA search (nuc_to_bits, src/dna_utilities.c): upper and lower case, everything else -1"""
    t = np.full(256, -1, dtype=np.int8)
    for k, c in enumerate("ACGT"):
        t[ord(c)] = t[ord(c.lower())] = k
    return t


def _case(seq, pattern, trans, thr, option, reach, capacity=None, multi=None, extra=()):
    """option: the seed on lastz's command line; reach: the counters that must be non-zero; multi: the lengths of the
    target's records but the last (a t.fa[multi] target), None for one record; extra: further options the files need"""
    return dict(seq=seq, pattern=pattern, trans=trans, thr=thr, option=option, reach=reach, capacity=capacity, multi=multi, extra=list(extra))


CASES = {
    "edges_m11": _case("edges", "1" * 11, 0, 30, ["--seed=match11", "--notransition"], ("dropped",)),
    "edges":     _case("edges", DEFAULT_SEED, 1, 30, ["--seed=12of19"], ("not_matching", "dropped")),
    # (on ONE diagonal diagEnd always sits on a mismatch or an end of a sequence: a later hit's left run stops there by itself,
    # one base short of being clipped.  A left end is clipped only by an extent written from another diagonal: collide)
    "spaced":    _case("spaced", DEFAULT_SEED, 1, 25, ["--seed=12of19"], ("not_matching", "dropped")),
    "collide":   _case("collide", DEFAULT_SEED, 1, 40, ["--seed=12of19"], ("clipped", "dropped", "other_diagonal")),
    "long":      _case("long", DEFAULT_SEED, 1, 50, ["--seed=12of19"], ("dropped", "past_cap")),
    "bytes":     _case("bytes", DEFAULT_SEED, 1, 30, ["--seed=12of19"], ("not_matching", "dropped"), multi=(1500,),
                       extra=["--ambiguous=iupac"]),            # (lastz reads an R only when told to; it matches nothing all the same)
    "chunks":    _case("spaced", DEFAULT_SEED, 1, 25, ["--seed=12of19"], ("not_matching", "dropped"), capacity=2048),
}
GOLDEN_CASES = [n for n in CASES if n != "chunks"]         # (chunks is spaced: the same command line)

_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _rand(rng, n):
    return ACGT[rng.integers(0, 4, n)]


def _other(rng, b):
    """every base replaced by a different one"""
    return ACGT[(np.searchsorted(ACGT, b) + rng.integers(1, 4, len(b))) % 4]


def _edges():
    """3 kbp target; the query is the target with single substitutions whose distances make exact runs of thr - 1, thr and
    thr + 1 bases, over and over (thr = 30)"""
    rng = np.random.default_rng(101)
    t = _rand(rng, 3000)
    q = t.copy()
    at, k = 17, 0
    while at < len(q):
        q[at:at + 1] = _other(rng, q[at:at + 1])
        at += (29, 30, 31)[k % 3] + 1
        k += 1
    return t, q


def _spaced():
    """20 kbp pair at about 90 % identity: substitutions only, so that the hits of a homologous stretch share a diagonal;
    3 kbp of the query are of the other strand (the command-line tier searches both)"""
    rng = np.random.default_rng(102)
    t = _rand(rng, 20000)
    q = t.copy()
    sub = rng.random(len(q)) < 0.10
    q[sub] = _other(rng, q[sub])
    rev = t[15000:18000].copy()                                # a stretch of the other strand
    sub = rng.random(len(rev)) < 0.10
    rev[sub] = _other(rng, rev[sub])
    q[6000:9000] = seqio.revcomp(rev)
    q = np.concatenate([q[:12000], q[12500:]])                 # and a second diagonal
    return t, q


def _collide():
    """70 kbp target with two different copies of a 300-base query block 65,536 bases apart: two diagonals in one bucket.  The
    copy at the higher target position is found first; its exact runs decide what happens to the other copy's hits"""
    rng = np.random.default_rng(103)
    t = _rand(rng, 70000)
    q = _rand(rng, 2000)
    block = q[800:1100]
    lo, hi = block.copy(), block.copy()
    for at in (60, 150, 240):                                  # the lower copy: runs of 60, 89, 89, 59
        lo[at:at + 1] = _other(rng, lo[at:at + 1])
    for at in (100, 200):                                      # the higher copy: runs of 100, 99, 99
        hi[at:at + 1] = _other(rng, hi[at:at + 1])
    t[1500:1800] = lo
    t[1500 + 65536:1800 + 65536] = hi
    return t, q


def _long():
    """a 6 kbp identical block (more than 4 x the cap on both sides of most of its hits), a run that starts on base 0 of both
    sequences and one that ends on the last base of both, on diagonals 0, +500 and -100; and twenty-four 60-base blocks
    between spacers that differ, so that the search has more HSPs than the smallest HSP capacity (16)"""
    rng = np.random.default_rng(104)
    s0, s1, s2 = _rand(rng, 400), _rand(rng, 6000), _rand(rng, 400)
    blocks = [_rand(rng, 60) for _ in range(24)]
    mid_t = np.concatenate([np.concatenate([b, _rand(rng, 30)]) for b in blocks])
    mid_q = np.concatenate([np.concatenate([b, _rand(rng, 30)]) for b in blocks])
    t = np.concatenate([s0, _rand(rng, 700), s1, _rand(rng, 300), mid_t, s2])
    q = np.concatenate([s0, _rand(rng, 200), s1, _rand(rng, 900), mid_q, s2])
    return t, q


def _bytes():
    """match_bits semantics: a run that crosses a lower-case stretch (it goes on), an N at the same place in both sequences
    (it stops there), an IUPAC code in one sequence, and a target of two records, the NUL between them inside a stretch
    the query has whole"""
    rng = np.random.default_rng(105)
    t = _rand(rng, 3000)
    q = _rand(rng, 2600)
    q[200:500] = t[300:600]                                    # lower case in the middle of a shared run, in the query only
    q[320:360] |= 0x20
    q[700:1000] = t[900:1200]                                  # ... in both
    t[1000:1040] |= 0x20
    q[800:840] |= 0x20
    q[1200:1400] = t[2000:2200]                                # an N at the same place in both
    t[2100] = q[1300] = ord("N")
    q[1500:1700] = t[2300:2500]                                # an IUPAC code in the target
    t[2400] = ord("R")
    q[1900:2300] = t[1300:1700]                                # across the records' boundary at 1500
    return t, q


SEQS = {"edges": _edges, "spaced": _spaced, "collide": _collide, "long": _long, "bytes": _bytes}


def records(name):
    """(target, query) as the FASTA files hold them"""
    return _once(("seq", CASES[name]["seq"]), SEQS[CASES[name]["seq"]])


def sequences(name):
    """(target bytes as the search sees them, its separators or [], query): a [multi] target is NUL, record, NUL, record, NUL"""
    t, q = records(name)
    v, seps = S.lay_out(t, CASES[name]["multi"])
    return v, seps, q


def target_records(name):
    t, _ = records(name)
    m = CASES[name]["multi"]
    if m is None:
        return [("target", t)]
    cuts = np.cumsum([0] + list(m) + [len(t) - sum(m)])
    return [("t%d" % k, t[cuts[k]:cuts[k + 1]]) for k in range(len(cuts) - 1)]


def lastz_options(name):
    """the case on lastz's command line (after the two files)"""
    c = CASES[name]
    return ["--exact=%d" % c["thr"]] + c["option"] + c["extra"] + ["--strand=plus"]


# ---------------------------------------------------------------------------------------- raw hits, the two CPU routines

def raw_hits(lzo, name):
    """the raw seed hits of the plus strand in discovery order, from the oracle: (pos1, pos2 arrays, its counters)"""
    def make():
        import helpers as H
        c = CASES[name]
        v, _, q = sequences(name)
        tab = lzo.Table(v, lzo.seed(c["pattern"], c["trans"]))
        h, st = lzo.seed_hit_search(tab, q, H.scoring()[1], mode=1)
        return np.ascontiguousarray(h["pos1"]), np.ascontiguousarray(h["pos2"]), st
    return _once(("raw", CASES[name]["seq"], CASES[name]["pattern"], CASES[name]["trans"]), make)


U8P = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
I8P = np.ctypeslib.ndpointer(dtype=np.int8, flags="C_CONTIGUOUS")
U32P = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
U64P = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
HSP_DTYPE = np.dtype([("pos1", "<u4"), ("pos2", "<u4"), ("length", "<u4"), ("score", "<i4")])


def emul():
    """tests/emul/emul_exact.cpp, compiled into a temporary directory"""
    def make():
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        so = os.path.join(tempfile.mkdtemp(prefix="emul_exact_"), "libemul_exact.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(root, "tests", "emul", "emul_exact.cpp")])
        L = C.CDLL(so)
        head = [U8P, C.c_uint32, U8P, C.c_uint32, I8P, C.c_uint32, C.c_int32, U32P, U32P, C.c_uint64, U32P, U64P, U64P]
        L.emul_exact_serial.argtypes = head
        L.emul_exact_decomposed.argtypes = head
        return L
    return _once("emul", make)


def run_on(fn, v, q, p1, p2, L, thr, n_extra):
    """one of the two routines over any sequences and any hit list in discovery order (a seed of length L, threshold thr):
    (HSPs in discovery order, the routine's extra words)"""
    p1, p2 = np.ascontiguousarray(p1, dtype=np.uint32), np.ascontiguousarray(p2, dtype=np.uint32)
    rows = np.zeros(4 * max(len(p1), 1), dtype=np.uint32)
    n, extra = np.zeros(1, dtype=np.uint64), np.zeros(n_extra, dtype=np.uint64)
    rc = fn(np.ascontiguousarray(v), len(v), np.ascontiguousarray(q), len(q), match_bits(), L, thr, p1, p2, len(p1), rows, n, extra)
    assert rc == 0
    return rows[:4 * int(n[0])].reshape(-1, 4).copy().view(HSP_DTYPE).reshape(-1), extra


def _run(fn, lzo, name, n_extra):
    c = CASES[name]
    v, _, q = sequences(name)
    p1, p2, _ = raw_hits(lzo, name)
    return run_on(fn, v, q, p1, p2, len(c["pattern"]), c["thr"], n_extra)


def serial(lzo, name):
    """the serial routine: (HSPs in discovery order, {counter: value})"""
    def make():
        hs, cn = _run(emul().emul_exact_serial, lzo, name, 5)
        return hs, dict(zip(COUNTERS, (int(x) for x in cn)))
    return _once(("serial", name), make)


def decomposed(lzo, name):
    """the decomposition: (HSPs in discovery order, SLOW hits)"""
    hs, extra = _run(emul().emul_exact_decomposed, lzo, name, 1)
    return hs, int(extra[0])


def rows_of(name, hsps):
    """HSPs of the plus strand -> the golden's rows (name1, start1, end1, name2, start2, end2, strand2, score), positions
    relative to the target record the HSP lies in"""
    _, seps, _ = sequences(name)
    recs = target_records(name)
    out = []
    for h in hsps:
        s1, e1 = int(h["pos1"] - h["length"]), int(h["pos1"])
        k, off = 0, 0
        if seps:
            k = max(j for j in range(len(seps) - 1) if seps[j] < e1)
            off = seps[k] + 1
        out.append((recs[k][0], s1 - off + 1, e1 - off, "query", int(h["pos2"] - h["length"]) + 1, int(h["pos2"]), "+", int(h["score"])))
    return out


def parse_rows(text):
    out = []
    for line in text.splitlines():
        f = line.split("\t")
        if len(f) == 8:
            out.append((f[0].strip(), int(f[1]), int(f[2]), f[3].strip(), int(f[4]), int(f[5]), f[6], int(f[7])))
    return out
