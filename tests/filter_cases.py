"""The seed-hit filter (lastz --filter=[<T>,]<M>, --filter=cares:[<T>,]<M>: lzgpu_set_hit_filter): one table of cases for the
three tiers -- the reference's predicate and the library's on the CPU, with the serial statement of a search over the hits the
filter keeps (tests/test_filter_cases.py, tests/emul/emul_filter.cpp), the goldens from the pristine binary
(tests/golden/make_filter_golden.py), and the library with the command line on the GPU (tests/test_gpu_filter.py,
tests/test_gpu_filter_cli.py).

The statement.  filter_seed_hit_by_subs runs after the diagEnd test and before any extension, a hit it rejects writes nothing,
and its verdict depends on the bases under the window alone: a filtered search is the same search over the raw hits in
discovery order with the rejected ones taken out.  So for every case: the raw hits from the oracle (its plain-hit processor),
the verdicts from the byte-wise transcription of the reference's routine, and over the kept hits the serial X-drop pass of
emul_filter.cpp, or emul_exact.cpp's / emul_mismatch.cpp's serial routine, or the hits themselves (`plain`).

Sequences come from seeded generators, at most 20 kbp a side, but for the `within` and `self` cases, which take theirs from
pos_filter_cases / self_cases.  Every case names `reach`: counts the CPU tier asserts are not zero (REACH below)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from lastz_amd import seqio
import exact_cases as EC
import mismatch_cases as MC
import pos_filter_cases as PF
import self_cases as S

SEED_12OF19 = EC.DEFAULT_SEED
SEED_8OF15 = "110100110010101"
WHOLE = EC.WHOLE
GOLDEN_FORMAT = EC.GOLDEN_FORMAT
match_bits = EC.match_bits
# reach: few_matches / many_transversions / kept = hits with that verdict; special_only = hits rejected only because a byte
# outside ACGTacgt counted as a transversion; lower_kept = kept hits with a counted position where the two bases match in
# different case; hsps = HSPs of the search
REACH = ("few_matches", "many_transversions", "kept", "special_only", "lower_kept", "hsps")


def _case(seq, M, T=None, cares=False, kind="xdrop", pattern=SEED_12OF19, trans=1, option=("--seed=12of19",), reach=("kept", "hsps"),
          capacity=None, golden=False, thr=None, mm=None, extra=(), strands=("+",), sub=None, seeding=False):
    """M, T: --filter=[T,]M (T None: no transversion limit); cares: --filter=cares:; kind: the search (xdrop, exact, mismatch,
    plain, within, self); option / extra: the seed and what else the files need on lastz's command line; thr, mm: the length of an
    --exact / --mismatch search and its mismatches; sub: the case of pos_filter_cases / self_cases a within / self search is;
    seeding: the table is built under seeding_bits() instead of upperCharToBits"""
    return dict(seq=seq, M=M, T=T, cares=cares, kind=kind, pattern=pattern, trans=trans, option=list(option), reach=reach,
                capacity=capacity, golden=golden, thr=thr, mm=mm, extra=list(extra), strands=strands if not golden else ("+", "-"), sub=sub,
                seeding=seeding)


ALL3 = ("few_matches", "many_transversions", "kept", "hsps")
CASES = {
    "whole_2_15":   _case("spaced", 15, 2, reach=ALL3, golden=True),
    "whole_1_15":   _case("spaced", 15, 1, reach=ALL3, golden=True),
    "matches_only": _case("spaced", 17, reach=("few_matches", "kept", "hsps"), golden=True),
    "cares_12":     _case("spaced", 12, cares=True, reach=("few_matches", "kept", "hsps"), golden=True),
    "noop":         _case("spaced", 0),
    # lastz makes its words under upperCharToBits, in the table and in the query (src/lastz.c:354, :3082-3125), and a word's window
    # holds no byte that table rejects (src/seed_search.c:499-510, src/pos_table.c:436-447): on lastz's command line NO raw hit has
    # a lower-case letter, an N, an IUPAC letter or a NUL anywhere in its window, so `bytes` -- the golden and the command-line
    # case -- cannot reach "rejected by a special byte" or "kept with a lower-case match" (its extensions run through such bytes,
    # its windows lie beside them).  The library takes any char_to_bits for its table: bytes_seeding is the same pair under a
    # table in which lower case, N and R are seed bytes, and reaches both through real raw hits; the NUL, which no table
    # takes, is under the windows of the predicates' sweep (tests/test_filter_cases.py).
    "bytes":        _case("bytes", 15, 0, reach=("few_matches", "kept", "hsps"), golden=True, extra=["--ambiguous=iupac"]),
    "bytes_seeding": _case("bytes", 15, 0, reach=("special_only", "lower_kept", "kept", "hsps"), seeding=True, extra=["--ambiguous=iupac"]),
    "exact":        _case("spaced", 15, 2, kind="exact", thr=25, reach=ALL3, golden=True),
    "mismatch":     _case("spaced", 15, 2, kind="mismatch", thr=30, mm=2, reach=ALL3, golden=True),
    "within":       _case("within", 17, 1, kind="within", sub="inside", reach=("many_transversions", "kept", "hsps")),
    "self":         _case("self", 17, 1, kind="self", sub="seed_t2", trans=2, reach=("few_matches", "kept", "hsps")),
    "plain":        _case("spaced", 15, 2, kind="plain", reach=("few_matches", "many_transversions", "kept")),
    "chunks":       _case("spaced", 15, 2, reach=ALL3, capacity=2048),
    "empty_chunks": _case("empty", 15, pattern=SEED_8OF15, option=("--seed=" + SEED_8OF15,), reach=("few_matches", "kept", "hsps"), capacity=2048),
}
GOLDEN_CASES = [n for n in CASES if CASES[n]["golden"]]
EMPTY_CHUNKS = 3                                           # empty_chunks: the first 3 x capacity raw hits are all rejected


def seeding_bits():
    """a char_to_bits for the table under which lower case, N and R make words: nuc_to_bits with N as A and R as G"""
    t = match_bits().copy()
    t[ord("N")], t[ord("R")] = 0, 2
    return t


def table_bits(lzo, name):
    """the char_to_bits the case's table is built under"""
    return seeding_bits() if CASES[name]["seeding"] else lzo.upper_nuc_to_bits()


def scoring(name):
    """the masked matrix of the case's X-drop search: HOXD70, and under --ambiguous=iupac every score against N or an IUPAC letter
    0 (ambiguate_iupac with lastz's default rewards, src/dna_utilities.c:1588-1640)"""
    def make():
        import helpers as H
        m = H.scoring()[1].copy()
        if "--ambiguous=iupac" in CASES[name]["extra"]:
            amb = [ord(x) for x in "NnBDHKMRSVWYbdhkmrsvwy"]
            for a in amb:
                for b in amb + [ord(x) for x in "ACGTacgt"]:
                    m[a, b] = m[b, a] = 0
        return np.ascontiguousarray(m)
    return EC._once(("fscoring", "--ambiguous=iupac" in CASES[name]["extra"]), make)


def case_of(name):
    """a case of CASES by its name, or a dict with the fields the predicates read (pattern, cares, M, T) as it is"""
    return CASES[name] if isinstance(name, str) else name


def positions(name):
    """lz_hit_filter.positions of the case"""
    c = case_of(name)
    L = len(c["pattern"])
    if not c["cares"]:
        return (1 << L) - 1
    return sum(1 << k for k in range(L) if c["pattern"][k] != "0")


def filter_option(name):
    c = CASES[name]
    return "--filter=%s%s%d" % ("cares:" if c["cares"] else "", "" if c["T"] is None else "%d," % c["T"], c["M"])


def lastz_options(name):
    """the case on lastz's command line (after the two files): both strands, lastz's default"""
    c = CASES[name]
    ext = {"xdrop": [], "exact": ["--exact=%d" % (c["thr"] or 0)], "mismatch": ["--mismatch=%d,%d" % (c["mm"] or 0, c["thr"] or 0)]}[c["kind"]]
    return [filter_option(name)] + ext + c["option"] + c["extra"]


# ---------------------------------------------------------------------------------------- sequences

def _light():
    """random 20 kbp target, random 8 kbp query: every raw hit of the 8of15 seed is chance"""
    rng = np.random.default_rng(301)
    return EC._rand(rng, 20000), EC._rand(rng, 8000)


def _empty():
    """light's query with 2 kbp of the target at about 90 % identity appended (substitutions only): the chance hits of the
    first 8 kbp fill whole chunks that a whole-window filter empties; the appended stretch still gives an HSP"""
    t, q = _light()
    rng = np.random.default_rng(302)
    tail = t[11000:13000].copy()
    sub = rng.random(len(tail)) < 0.10
    tail[sub] = EC._other(rng, tail[sub])
    return t, np.concatenate([q, tail])


def sequences(name):
    """(target bytes as the search sees them, its separators or [], the query of the plus strand)"""
    c = CASES[name]
    if c["seq"] in ("spaced", "bytes"):
        return EC.sequences(c["seq"])
    if c["seq"] == "empty":
        t, q = EC._once(("fseq", "empty"), _empty)
        return t, [], q
    if c["seq"] == "within":
        t, qs = PF.queries(c["sub"])
        return t, [], qs[0]
    v, seps, _ = S.sequence(c["sub"])
    assert not seps
    return v, [], v


def records(name):
    c = CASES[name]
    assert c["seq"] in ("spaced", "bytes")
    return EC.records(c["seq"])


def target_records(name):
    return EC.target_records(CASES[name]["seq"])


def query_of(name, strand):
    q = sequences(name)[2]
    return q if strand == "+" else seqio.revcomp(q)


# ---------------------------------------------------------------------------------------- raw hits, verdicts, the statement

def raw_hits(lzo, name, strand="+"):
    """the raw seed hits the case's search sees, in discovery order, from the oracle: (pos1, pos2, its counters)"""
    c = CASES[name]

    def make():
        import helpers as H
        v, _, _ = sequences(name)
        q = query_of(name, strand)
        masked = H.scoring()[1]
        if c["kind"] == "within":
            p = PF.CASES[c["sub"]]
            sd = lzo.seed(p["pattern"], p["trans"])
            (ts, te), (qs, qe) = PF.intersect(p, len(v), len(q), sd.length)
            h, st = lzo.seed_hit_search(lzo.Table(v, sd, step=p["step"], start=ts, end=te), q, masked, mode=1, start=qs, end=qe)
        elif c["kind"] == "self":
            h, st = lzo.seed_hit_search(lzo.Table(v, lzo.seed(c["pattern"], c["trans"])), q, masked, mode=1, self_strand="same")
        else:
            tab = EC._once(("ftab", c["seq"], c["pattern"], c["trans"], c["seeding"]),
                           lambda: lzo.Table(v, lzo.seed(c["pattern"], c["trans"]), ctb=table_bits(lzo, name)))
            h, st = lzo.seed_hit_search(tab, q, masked, mode=1)
        return np.ascontiguousarray(h["pos1"]), np.ascontiguousarray(h["pos2"]), st
    return EC._once(("fraw", c["seq"], c["sub"], c["kind"] in ("within", "self"), c["pattern"], c["trans"], c["seeding"], strand), make)


U8P, I8P, U32P, U64P = EC.U8P, EC.I8P, EC.U32P, EC.U64P
I32P = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")


def emul_sources():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return [os.path.join(root, "tests", "emul", "emul_filter.cpp"), os.path.join(root, "lastz_amd", "csrc", "lz_host.cpp")]


def emul():
    """tests/emul/emul_filter.cpp (with the library's host pieces), compiled into a temporary directory"""
    def make():
        so = os.path.join(tempfile.mkdtemp(prefix="emul_filter_"), "libemul_filter.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", so] + emul_sources())
        L = C.CDLL(so)
        L.emul_filter_bytes.argtypes = [U8P, U8P, I8P, C.c_uint32, C.c_uint32, C.c_int, C.c_int32, C.c_int32, U32P, U32P, C.c_uint64, U8P, U8P]
        L.emul_filter_codes.argtypes = [U8P, C.c_uint32, U8P, C.c_uint32, I8P, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, U32P, U32P, C.c_uint64, U8P, U8P]
        L.emul_filter_xdrop.argtypes = [U8P, C.c_uint32, U8P, C.c_uint32, I8P, I32P, C.c_int32, C.c_int32, C.c_int, C.c_char_p, C.c_int,
                                        U32P, U32P, C.c_uint64, U32P, U64P, U64P]
        return L
    return EC._once("emul_filter", make)


def _T(c):
    return -1 if c["T"] is None else c["T"]


def by_bytes(name, t, q, p1, p2):
    """filter_seed_hit_by_subs over the windows ending at (p1, p2): (verdict per hit: 0 kept, 1 few matches, 2 many transversions;
    (matches, transversions) per hit)"""
    c = case_of(name)
    p1, p2 = np.ascontiguousarray(p1, dtype=np.uint32), np.ascontiguousarray(p2, dtype=np.uint32)
    verdict, counts = np.zeros(max(len(p1), 1), dtype=np.uint8), np.zeros(2 * max(len(p1), 1), dtype=np.uint8)
    rc = emul().emul_filter_bytes(np.ascontiguousarray(t), np.ascontiguousarray(q), match_bits(), len(c["pattern"]), positions(name),
                                  int(c["cares"]), c["M"], _T(c), p1, p2, len(p1), verdict, counts)
    assert rc == 0
    return verdict[:len(p1)], counts[:2 * len(p1)].reshape(-1, 2)


def by_codes(name, t, q, p1, p2):
    """lz_filter.hpp's predicate on match codes: (keeps per hit: 1 / 0; (matches, transversions) per hit)"""
    c = case_of(name)
    p1, p2 = np.ascontiguousarray(p1, dtype=np.uint32), np.ascontiguousarray(p2, dtype=np.uint32)
    keeps, counts = np.zeros(max(len(p1), 1), dtype=np.uint8), np.zeros(2 * max(len(p1), 1), dtype=np.uint8)
    rc = emul().emul_filter_codes(np.ascontiguousarray(t), len(t), np.ascontiguousarray(q), len(q), match_bits(), len(c["pattern"]),
                                  positions(name), c["M"], _T(c), p1, p2, len(p1), keeps, counts)
    assert rc == 0
    return keeps[:len(p1)], counts[:2 * len(p1)].reshape(-1, 2)


def verdicts(lzo, name, strand="+"):
    """the reference's verdict on every raw hit of the case"""
    def make():
        p1, p2, _ = raw_hits(lzo, name, strand)
        return by_bytes(name, sequences(name)[0], query_of(name, strand), p1, p2)
    return EC._once(("fverdict", name, strand), make)


def _rows(rows, n):
    return rows[:4 * int(n)].reshape(-1, 4).copy().view(EC.HSP_DTYPE).reshape(-1)


def expected(lzo, name, strand="+"):
    """the case's search as the reference runs it: dict(hsps in the reporter's order, raw, dropped, and where the search
    counts them extensions, bp_extended)"""
    def make():
        p1, p2, st = raw_hits(lzo, name, strand)
        return search_over(CASES[name], sequences(name)[0], query_of(name, strand), p1, p2, verdicts(lzo, name, strand)[0] == 0,
                           st["words"], table_bits(lzo, name), scoring(name))
    return EC._once(("fexpected", name, strand), make)


def search_over(c, v, q, p1, p2, keep, words, ctb, masked):
    """the statement over any sequences and any raw hits in discovery order: the search of kind c["kind"] (with c's pattern,
    trans, thr, mm) over the hits `keep` marks -> dict(hsps, raw, dropped, words and, where the search counts them, extensions,
    bp_extended); ctb, masked: the table's char_to_bits and the masked matrix of an X-drop search"""
    k1, k2 = np.ascontiguousarray(p1[keep], dtype=np.uint32), np.ascontiguousarray(p2[keep], dtype=np.uint32)
    out = dict(raw=len(p1), dropped=int(len(p1) - keep.sum()), words=words)
    L = len(c["pattern"])
    rows, n = np.zeros(4 * max(len(k1), 1), dtype=np.uint32), np.zeros(1, dtype=np.uint64)
    vv, qq = np.ascontiguousarray(v), np.ascontiguousarray(q)
    if c["kind"] == "plain":
        hs = np.zeros(len(k1), dtype=EC.HSP_DTYPE)
        hs["pos1"], hs["pos2"], hs["length"] = k1, k2, L
        out.update(hsps=hs)
    elif c["kind"] == "exact":
        rc = EC.emul().emul_exact_serial(vv, len(vv), qq, len(qq), match_bits(), L, c["thr"], k1, k2, len(k1), rows, n, np.zeros(5, dtype=np.uint64))
        assert rc == 0
        out.update(hsps=_rows(rows, n[0]), extensions=0, bp_extended=0)
    elif c["kind"] == "mismatch":
        rc = MC.emul().emul_mismatch_serial(vv, len(vv), qq, len(qq), match_bits(), L, c["mm"], c["thr"], k1, k2, len(k1), rows, n,
                                            np.zeros(len(MC.COUNTERS), dtype=np.uint64), np.zeros(MC.DIAG_SIZE, dtype=np.uint32))
        assert rc == 0
        out.update(hsps=_rows(rows, n[0]), extensions=0, bp_extended=0)
    else:
        cn = np.zeros(2, dtype=np.uint64)
        rc = emul().emul_filter_xdrop(vv, len(vv), qq, len(qq), ctb, np.ascontiguousarray(masked), 910, 3000, 1,
                                      c["pattern"].encode(), c["trans"], k1, k2, len(k1), rows, n, cn)
        assert rc == 0
        out.update(hsps=_rows(rows, n[0]), extensions=int(cn[0]), bp_extended=int(cn[1]))
    return out


def reach(lzo, name):
    """{REACH name: count} of the plus strand"""
    v, _, q = sequences(name)
    p1, p2, _ = raw_hits(lzo, name)
    verdict, counts = verdicts(lzo, name)
    c = CASES[name]
    L = len(c["pattern"])
    mb = match_bits()
    cols = np.flatnonzero([(positions(name) >> k) & 1 for k in range(L)])
    wt = v[(p1.astype(np.int64) - L)[:, None] + cols[None, :]]
    wq = q[(p2.astype(np.int64) - L)[:, None] + cols[None, :]]
    special = ((mb[wt] < 0) | (mb[wq] < 0)).sum(axis=1)
    lower = ((mb[wt] >= 0) & (mb[wt] == mb[wq]) & (wt != wq)).any(axis=1)
    T = 1 << 30 if c["T"] is None else c["T"]
    special_only = (verdict == 2) & (special > 0) & (counts[:, 1].astype(np.int64) - special <= T)
    return dict(few_matches=int((verdict == 1).sum()), many_transversions=int((verdict == 2).sum()), kept=int((verdict == 0).sum()),
                special_only=int(special_only.sum()), lower_kept=int(((verdict == 0) & lower).sum()), hsps=len(expected(lzo, name)["hsps"]))


def rows_of(name, strand, hsps):
    """HSPs of one strand -> the golden's rows (name1, start1, end1, name2, start2, end2, strand2, score), positions relative to
    the target record the HSP lies in, and in the query along the strand"""
    _, seps, _ = sequences(name)
    recs = target_records(name)
    out = []
    for h in hsps:
        s1, e1 = int(h["pos1"] - h["length"]), int(h["pos1"])
        k, off = 0, 0
        if seps:
            k = max(j for j in range(len(seps) - 1) if seps[j] < e1)
            off = seps[k] + 1
        out.append((recs[k][0], s1 - off + 1, e1 - off, "query", int(h["pos2"] - h["length"]) + 1, int(h["pos2"]), strand, int(h["score"])))
    return out


parse_rows = EC.parse_rows


def sweep(name, n=400, seed=7):
    """window ends for the predicates beyond the raw hits: at both ends of both sequences (pos = L and pos = len), at random, on
    the main diagonal and -- a [multi] target -- across every NUL; (pos1, pos2)"""
    v, seps, q = sequences(name)
    return sweep_over(v, seps, q, len(CASES[name]["pattern"]), n, seed)


def sweep_over(v, seps, q, L, n=400, seed=7):
    """sweep() over any sequences and any window length"""
    rng = np.random.default_rng(seed)
    ends1 = [L, L + 1, len(v) - 1, len(v)] + [s + d for s in seps for d in range(1, L + 2) if L <= s + d <= len(v)]
    ends2 = [L, L + 1, len(q) - 1, len(q)]
    same = rng.integers(L, min(len(v), len(q)) + 1, n)           # (the main diagonal: where a pair is homologous, windows of many matches)
    p1 = np.concatenate([np.repeat(ends1, len(ends2)), rng.integers(L, len(v) + 1, n), np.repeat(ends1, 8), rng.integers(L, len(v) + 1, 8 * len(ends2)), same])
    p2 = np.concatenate([np.tile(ends2, len(ends1)), rng.integers(L, len(q) + 1, n), rng.integers(L, len(q) + 1, 8 * len(ends1)), np.repeat(ends2, 8), same])
    return p1.astype(np.uint32), p2.astype(np.uint32)
