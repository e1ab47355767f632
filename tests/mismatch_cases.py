"""N-mismatch extension of seed hits (lastz --mismatch=<count>,<length>): one table of cases for the three tiers -- the serial
transcription and the GPU's decomposition on the CPU (tests/test_mismatch_cases.py, tests/emul/emul_mismatch.cpp), the goldens
from the pristine binary (tests/golden/make_mismatch_golden.py), and lzgpu_seed_hit_search_mismatch with the command line on
the GPU (tests/test_gpu_mismatch.py, tests/test_gpu_mismatch_cli.py).

The sequences are those of tests/exact_cases.py (its generators, imported), a `collide` pair of its own (under exact_cases'
one no left scan is clipped by the other diagonal's extent: there every hit of the lower copy is dropped) and one pair more,
`background`.  Every case names a seed, M, a threshold and, where given, a hit capacity, and `reach`: the branch counters of
the serial routine (emul_mismatch.cpp's order, COUNTERS below) that must not be zero -- what keeps the case from testing
nothing.  `other_diagonal` counts left scans that ended at a diagEnd another diagonal of the bucket wrote, not drops."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import exact_cases as EC
import self_cases as S

COUNTERS = ("too_many", "seed_mm", "clipped", "nul_left", "start", "shortfall", "right_stop", "dropped", "other_diagonal",
            "past_cap", "past_step")
FORMS = ("fast_too_many", "fast_no_hsp", "slow")            # emul_mismatch_decomposed's form[]: 0, 1, 2
WHOLE = EC.WHOLE
GOLDEN_FORMAT = EC.GOLDEN_FORMAT
DIAG_SIZE = 1 << 16
match_bits = EC.match_bits


def _case(seq, pattern, trans, M, thr, option, reach, capacity=None, multi=None, extra=()):
    return dict(seq=seq, pattern=pattern, trans=trans, M=M, thr=thr, option=option, reach=reach, capacity=capacity, multi=multi, extra=list(extra))


D = EC.DEFAULT_SEED
CASES = {
    "edges":      _case("edges", D, 1, 1, 61, ["--seed=12of19"], ("clipped", "shortfall")),
    "edges_m11":  _case("edges", "1" * 11, 0, 2, 92, ["--seed=match11", "--notransition"], ("shortfall",)),
    "low":        _case("edges", D, 1, 3, 20, ["--seed=12of19"], ("right_stop",)),
    "spaced":     _case("spaced", D, 1, 2, 40, ["--seed=12of19"], ("seed_mm", "too_many", "clipped", "shortfall", "dropped")),
    "many":       _case("spaced", D, 1, 50, 400, ["--seed=12of19"], ("start", "right_stop")),
    "collide":    _case("collide_mm", D, 1, 1, 40, ["--seed=12of19"], ("clipped", "other_diagonal", "dropped")),
    "long":       _case("long", D, 1, 3, 60, ["--seed=12of19"], ("past_cap", "past_step", "start", "right_stop")),
    "bytes":      _case("bytes", D, 1, 1, 120, ["--seed=12of19"], ("nul_left", "right_stop"), multi=(1500,), extra=["--ambiguous=iupac"]),
    "chunks":     _case("spaced", D, 1, 2, 40, ["--seed=12of19"], ("seed_mm", "too_many", "clipped", "shortfall", "dropped"), capacity=2048),
    "background": _case("background", D, 1, 2, 40, ["--seed=12of19"], ("too_many", "seed_mm", "dropped")),
}
GOLDEN_CASES = [n for n in CASES if n != "chunks"]         # (chunks is spaced: the same command line)

# background: where the three blocks lie, (target position, query position), and how long they are
PLANTED = ((30000, 2000), (110000, 9000), (170000, 16000))
PLANTED_LEN = 300


def _background():
    """a 200 kbp random target and an unrelated 20 kbp random query into which three 300-base blocks of the target are planted
    at about 95 % identity: nearly every hit is chance, and phase A has to say so by itself"""
    rng = np.random.default_rng(106)
    t = EC._rand(rng, 200000)
    q = EC._rand(rng, 20000)
    for tp, qp in PLANTED:
        b = t[tp:tp + PLANTED_LEN].copy()
        sub = rng.random(PLANTED_LEN) < 0.05
        b[sub] = EC._other(rng, b[sub])
        q[qp:qp + PLANTED_LEN] = b
    return t, q


def _collide_mm():
    """70 kbp target with two copies of a 300-base query block 65,536 bases apart: two diagonals in one bucket.  The copy at the
    higher target position is found first at every query position, but it holds the block's first 100 bases only: its one HSP
    writes an extent into the middle of the block, the lower copy's hits in front of that extent are dropped, and the first one
    behind it has its left scan clipped there -- by the other diagonal's extent -- while its own bases go on matching"""
    rng = np.random.default_rng(107)
    t = EC._rand(rng, 70000)
    q = EC._rand(rng, 2000)
    block = q[800:1100]
    lo = block.copy()
    for at in (60, 150, 240):                                  # the lower copy: runs of 60, 89, 89, 59
        lo[at:at + 1] = EC._other(rng, lo[at:at + 1])
    t[1500:1800] = lo
    t[1500 + 65536:1600 + 65536] = block[:100]
    return t, q


SEQS = dict(EC.SEQS, background=_background, collide_mm=_collide_mm)


def records(name):
    """(target, query) as the FASTA files hold them"""
    return EC._once(("seq", CASES[name]["seq"]), SEQS[CASES[name]["seq"]])


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


def lastz_options(name, spelling=0):
    """the case on lastz's command line (after the two files); spelling 1: --<count>mismatch=<length>"""
    c = CASES[name]
    opt = "--mismatch=%d,%d" % (c["M"], c["thr"]) if spelling == 0 else "--%dmismatch=%d" % (c["M"], c["thr"])
    return [opt] + c["option"] + c["extra"] + ["--strand=plus"]


# ---------------------------------------------------------------------------------------- raw hits, the two CPU routines

def raw_hits(lzo, name, interval=(0, 0)):
    """the raw seed hits of the plus strand in discovery order, from the oracle: (pos1, pos2 arrays, its counters); interval:
    the (start, end) of the query the search is limited to, (0, 0) for all of it"""
    def make():
        import helpers as H
        c = CASES[name]
        v, _, q = sequences(name)
        tab = lzo.Table(v, lzo.seed(c["pattern"], c["trans"]))
        h, st = lzo.seed_hit_search(tab, q, H.scoring()[1], mode=1, start=interval[0], end=interval[1])
        return np.ascontiguousarray(h["pos1"]), np.ascontiguousarray(h["pos2"]), st
    return EC._once(("raw", CASES[name]["seq"], CASES[name]["pattern"], CASES[name]["trans"], CASES[name]["multi"], interval), make)


def emul_source():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return os.path.join(root, "tests", "emul", "emul_mismatch.cpp")


def emul():
    """tests/emul/emul_mismatch.cpp, compiled into a temporary directory"""
    def make():
        so = os.path.join(tempfile.mkdtemp(prefix="emul_mismatch_"), "libemul_mismatch.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, emul_source()])
        L = C.CDLL(so)
        head = [EC.U8P, C.c_uint32, EC.U8P, C.c_uint32, EC.I8P, C.c_uint32, C.c_uint32, C.c_int32, EC.U32P, EC.U32P, C.c_uint64, EC.U32P, EC.U64P]
        L.emul_mismatch_serial.argtypes = head + [EC.U64P, EC.U32P]
        L.emul_mismatch_decomposed.argtypes = head + [EC.U8P, EC.U32P]
        return L
    return EC._once("emul_mismatch", make)


def run_on(fn, v, q, p1, p2, L, M, thr, extra):
    """one of the two routines over any sequences and any hit list in discovery order (a seed of length L, M mismatches,
    threshold thr): (HSPs in discovery order, diagEnd as the routine leaves it); extra: its counters[] or form[]"""
    p1, p2 = np.ascontiguousarray(p1, dtype=np.uint32), np.ascontiguousarray(p2, dtype=np.uint32)
    rows = np.zeros(4 * max(len(p1), 1), dtype=np.uint32)
    n, dend = np.zeros(1, dtype=np.uint64), np.zeros(DIAG_SIZE, dtype=np.uint32)
    rc = fn(np.ascontiguousarray(v), len(v), np.ascontiguousarray(q), len(q), match_bits(), L, M, thr, p1, p2, len(p1), rows, n, extra, dend)
    assert rc == 0, rc
    return rows[:4 * int(n[0])].reshape(-1, 4).copy().view(EC.HSP_DTYPE).reshape(-1), dend


def _run(fn, lzo, name, extra, interval=(0, 0)):
    c = CASES[name]
    v, _, q = sequences(name)
    p1, p2, _ = raw_hits(lzo, name, interval)
    return run_on(fn, v, q, p1, p2, len(c["pattern"]), c["M"], c["thr"], extra)


def serial(lzo, name, interval=(0, 0)):
    """the serial routine, on all of the query or on an interval of it: (HSPs in discovery order, {counter: value}, diagEnd as it
    leaves it)"""
    def make():
        cn = np.zeros(len(COUNTERS), dtype=np.uint64)
        hs, dend = _run(emul().emul_mismatch_serial, lzo, name, cn, interval)
        return hs, dict(zip(COUNTERS, (int(x) for x in cn))), dend
    return EC._once(("mm_serial", name, interval), make)


def decomposed(lzo, name):
    """the decomposition: (HSPs in discovery order, every hit's form (an index into FORMS), diagEnd as it leaves it)"""
    def make():
        form = np.zeros(max(len(raw_hits(lzo, name)[0]), 1), dtype=np.uint8)
        hs, dend = _run(emul().emul_mismatch_decomposed, lzo, name, form)
        return hs, form[:len(raw_hits(lzo, name)[0])], dend
    return EC._once(("mm_decomposed", name), make)


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


parse_rows = EC.parse_rows
