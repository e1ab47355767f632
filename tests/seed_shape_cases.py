"""Seed shapes beyond the five the other tests use: one table of cases for four tiers -- the oracle against the pristine
binary (tests/test_seed_shapes_oracle.py), the device decomposition on the CPU (tests/test_emul_seed_shapes.py), the
library on the GPU (tests/test_gpu_seed_shapes.py) and the bound command line (tests/test_gpu_seed_shapes_cli.py).

What depends on a seed's shape sits in the kernels: the "no word" key 1 << weight and the weight + 1 bits of the table's
radix sort, the 2^weight + 1 bounds (k_table_words, k_key_bounds_u32, k_table_export), the block bits that fit beside
the word in k_pack_words' 32-bit key, its LDS window of length + 255 codes, the probe loops in rounds of 16
(k_fill_hits2, k_scan_hits2, k_count_sorted_self) and the pieces of LZ_F2_CAP hits a wave's lists are taken in.

A case names its pattern, transitions, step, pair of sequences, threshold and hit capacity, the options that say the same
on lastz's command line, and in `reach` the numbers that make it worth running.  `reaches(name)` checks them on the
ORACLE's results alone; test_seed_shapes_oracle.py asserts it for every case, so that a case which no longer meets what it
was built for fails on the CPU.

The pairs (none committed):
  pair    seqio.synth_pair(120000, 90000, seed=31, block_min=500, block_max=4000)
  ends31  pair with the query's first and last 31 bases copied from the target's: a seed hit whose window starts at
          position 0 and one whose window ends on the last base of both
  cut     the first 3000 x 2500 bases of pair.  These share no homology (the query's blocks are copied from anywhere in
          the target), so two diverged copies are planted: 600 target bases on the plus strand, 400 on the minus strand;
          without them the light seeds have no HSP at all to compare.  With 16 to 256 words every list of the table has
          tens to hundreds of entries and a search at hit capacity 50,000 takes 3 to 40 chunks.
  big     seqio.synth_pair(300000, 300000, seed=6)
The CPU emulator tier runs the cases of `pair` and `ends31` on their first 60,000 x 50,000 bases (emul_sequences).

Looked for and not found: a pattern of more than 6 parts (lzgpu_seed_from_pattern's shift / mask pairs) among 330,000 random
patterns of length 31 and 4 to 14 ones; parts6 is one of those with 6.

(test infrastructure: data and helpers, no test in this file)"""
import ctypes as C

import numpy as np

from lastz_amd import seqio

COUNTERS = ("words", "raw_hits", "extensions", "bp_extended", "hsps")
WHOLE = 1 << 28                                     # the hit capacity that chunks nothing here
LZ_F2_CAP = 2560                                    # lastz_amd/csrc/enum_kernels.hip: hits per piece of a wave's concatenation
S14OF22 = "1110101100110010101111"
GOLDEN_FORMAT = "--format=general-:name2,start1,end1,start2,end2,strand2,score"
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _case(pattern, trans, seq="pair", step=1, thr=3000, capacity=None, option=None, plain=False, export=True, twin=None, **reach):
    """option: how lastz's command line names the seed (None: --seed=<pattern> and the transition flag); plain: the raw
    hits (extend=False) are compared too; export: the GPU tier exports last[] / prev[]; twin: a pattern that must give
    the same descriptor and results; reach: length, bits, parts, probes of the descriptor, then per strand `hsps` and
    `raw` (raw seed hits); waves: "all" -- any 64 query positions have more than LZ_F2_CAP hits between
    them -- or "some" -- 64 average ones have"""
    return dict(pattern=pattern, trans=trans, seq=seq, step=step, thr=thr, capacity=capacity, option=option, plain=plain,
                export=export, twin=twin, reach=reach)


_LIGHT = dict(seq="cut", thr=1500, capacity=50_000)

CASES = {
    # 28 bits: the 29-bit table sort, 2^28 + 1 bounds, a 1 GiB last[]
    "s14of22":     _case(S14OF22, 1, option=["--seed=14of22"], length=22, bits=28, parts=3, probes=15, hsps=(86, 124), raw=(3723, 4598)),
    # 106 probes: seven rounds of 16 with a partial last one
    "s14of22_t2":  _case(S14OF22, 2, option=["--seed=14of22", "--transition=2"], plain=True, export=False,
                         length=22, bits=28, parts=3, probes=106, hsps=(86, 124), raw=(7764, 8593)),
    "match14":     _case("1" * 14, 0, option=["--seed=match14", "--notransition"], length=14, bits=28, parts=1, probes=1, hsps=(80, 120), raw=(2061, 2819)),
    "match13_t2":  _case("1" * 13, 2, option=["--seed=match13", "--transition=2"], length=13, bits=26, parts=1, probes=92, hsps=(85, 123), raw=(18603, 19788)),
    # length 31: k_pack_words' window of the block's first position starts 30 bases in front of the query
    "long31":      _case("1100100100100100100100100100111", 1, seq="ends31", thr=1500, plain=True,
                         length=31, bits=26, parts=4, probes=14, hsps=(98, 143), raw=(5496, 6105)),
    "parts6_t1":   _case("1010001010000100000011001000001", 1, length=31, bits=18, parts=6, probes=10, hsps=(86, 124), raw=(417199, 417386)),
    "parts6_t2":   _case("1010001010000100000011001000001", 2, length=31, bits=18, parts=6, probes=46, hsps=(86, 124), raw=(1897539, 1901955)),
    "sparse31_t2": _case("1001001001001001001001001001001", 2, length=31, bits=22, parts=3, probes=67, hsps=(86, 123), raw=(177677, 177703)),
    # 4 to 8 bits: every list is long (a 3000-base target has no list of LZ_F2_CAP entries; the longest has 235), so that
    # the 64 positions of one wave concatenate to more than LZ_F2_CAP hits -- any 64 for the 4-bit seeds, 64 average ones
    # for the 8-bit seeds -- and a search takes 3 to 38 chunks
    "light2":      _case("11", 0, length=2, bits=4, parts=1, probes=1, waves="all", raw=(470041, 467518), **_LIGHT),
    "light2_t2":   _case("11", 2, plain=True, length=2, bits=4, parts=1, probes=4, waves="all", raw=(1872800, 1874258), **_LIGHT),
    "light4_t1":   _case("1111", 1, length=4, bits=8, parts=1, probes=5, waves="some", raw=(147588, 145675), **_LIGHT),
    "gap101_t1":   _case("101", 1, length=3, bits=4, parts=2, probes=3, waves="all", raw=(1405630, 1404708), **_LIGHT),
    "ends29_t1":   _case("1" + "0" * 27 + "1", 1, length=29, bits=4, parts=2, probes=3, waves="all", raw=(1378498, 1376774), **_LIGHT),
    # leading and trailing zeros are trimmed: the descriptor and the results of 11x11
    "trimmed":     _case("0011x1100", 1, twin="11x11", length=5, bits=8, parts=2, probes=5, waves="some", raw=(147595, 146633), **_LIGHT),
}
# (pattern, transitions) the library declines with LZGPU_NH_SEED when the pattern is compiled ...
DECLINED_SEEDS = [("1" * 15, 1),                                         # match15: 30 bits
                  ("1010101010101010101010101010101", 1),                # 16 ones in 31: 32 bits
                  ("1T1T1T1T11", 0)]                                     # half-weight positions
# ... and the one it compiles and lzgpu_table_prepare declines (NotHandled(1)): a word of one base
DECLINED_TABLES = [("1", 0)]

# heavy_blocks: s14of22_t2 on `big` at hit capacity 2048.  lzk_count_hits (enum_kernels.hip) restated: it wants twice as
# many blocks of query positions as it expects chunks, at most 32, and the key has 32 - (weight + 1) bits for them.
HEAVY = dict(case="s14of22_t2", seq="big", capacity=2048)


def want_block_bits(n, num_words, probes, weight, capacity):
    """-> (est_hits, want_bits, block bits the key has room for) of a search over n query positions"""
    est = float(n) * float(num_words) * float(probes) / float(1 << weight)
    want = 0
    while want < 5 and est > float(capacity) * float(1 << want) * 0.5:
        want += 1
    if est <= float(capacity):
        want = 0
    return est, want, min(want, 32 - (weight + 1))


# ---------------------------------------------------------------------------------------- sequences

_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _pair():
    return seqio.synth_pair(120_000, 90_000, seed=31, block_min=500, block_max=4000)


def _ends31():
    t, q = sequences("pair")
    q = q.copy()
    q[:31] = t[:31]
    q[-31:] = t[-31:]
    return t, q


def _diverged(block, every):
    b = block.copy()
    at = np.arange(every // 2, len(b), every)
    b[at] = ACGT[(np.searchsorted(ACGT, b[at]) + 1) % 4]
    return b


def _cut():
    t, q = sequences("pair")
    t, q = t[:3000].copy(), q[:2500].copy()
    q[1200:1800] = _diverged(t[700:1300], 29)
    q[300:700] = seqio.revcomp(_diverged(t[2000:2400], 23))
    return t, q


SEQS = {"pair": _pair, "ends31": _ends31, "cut": _cut, "big": lambda: seqio.synth_pair(300_000, 300_000, seed=6)}


def sequences(name):
    return _once(("seq", name), SEQS[name])


def emul_sequences(name):
    """what the CPU emulator tier runs a case on: the first 60,000 x 50,000 bases (ends31: with its ends copied again)"""
    t, q = sequences(CASES[name]["seq"])
    if len(t) <= 60_000:
        return t, q
    t, q = t[:60_000], q[:50_000].copy()
    if CASES[name]["seq"] == "ends31":
        q[-31:] = t[-31:]
    return t, q


def queries(name):
    q = sequences(CASES[name]["seq"])[1]
    return q, seqio.revcomp(q)


def lastz_options(name):
    """the case on lastz's command line (after the two files)"""
    c = CASES[name]
    opt = c["option"] or ["--seed=" + c["pattern"], ("--notransition", "--transition", "--transition=2")[c["trans"]]]
    return opt + (["--step=%d" % c["step"]] if c["step"] != 1 else []) + (["--hspthresh=%d" % c["thr"]] if c["thr"] != 3000 else [])


# ---------------------------------------------------------------------------------------- the oracle's statement

def table(lzo, name):
    c = CASES[name]
    return _once(("table", name), lambda: lzo.Table(sequences(c["seq"])[0], lzo.seed(c["pattern"], c["trans"]), step=c["step"]))


def oracle_search(lzo, name, masked, extend=True):
    """-> ([HSP array per strand], [counters per strand]), computed once"""
    def make():
        hs, sts = [], []
        for q in queries(name):
            h, st = lzo.seed_hit_search(table(lzo, name), q, masked, hsp_threshold=CASES[name]["thr"], mode=0 if extend else 1)
            hs.append(h)
            sts.append(st)
        return hs, sts
    return _once(("search", name, extend), make)


def summed(sts):
    return {k: sum(st[k] for st in sts) for k in COUNTERS}


def heavy_search(lzo, masked):
    """the oracle's search of heavy_blocks -> (table, [HSP array per strand], [counters per strand])"""
    def make():
        c = CASES[HEAVY["case"]]
        t, q = sequences(HEAVY["seq"])
        tab = lzo.Table(t, lzo.seed(c["pattern"], c["trans"]))
        res = [lzo.seed_hit_search(tab, qq, masked) for qq in (q, seqio.revcomp(q))]
        return tab, [r[0] for r in res], [r[1] for r in res]
    return _once("heavy", make)


def hits_per_position(lzo, name, strand):
    """the raw hits of every query position that holds a word (all probes; the light seeds have at most 5, one probe group)"""
    c = CASES[name]
    sd = lzo.seed(c["pattern"], c["trans"])
    ws, _ = table(lzo, name).csr()
    n = np.diff(ws.astype(np.int64))
    q = queries(name)[strand]
    code = np.full(256, -1, dtype=np.int64)
    code[ACGT] = np.arange(4)
    bits = code[q]
    words = []
    for e in range(sd.length, len(q) + 1):
        w = bits[e - sd.length:e]
        if (w >= 0).all():
            packed = 0
            for b in w:
                packed = (packed << 2) | int(b)
            words.append(int(lzo.lib().lzo_apply_seed(C.byref(sd), C.c_uint64(packed))))
    xors = np.array([sd.probe_xor[k] for k in range(sd.num_probes)], dtype=np.int64)
    return n[np.array(words, dtype=np.int64)[:, None] ^ xors[None, :]].sum(axis=1)


def reaches(lzo, name, masked):
    """None if the case meets what it was built for, else what is missing"""
    c, r = CASES[name], CASES[name]["reach"]
    sd = lzo.seed(c["pattern"], c["trans"])
    have = dict(length=sd.length, bits=sd.weight, parts=sd.num_parts, probes=sd.num_probes)
    want = {k: r[k] for k in have}
    if have != want:
        return "descriptor %s, stated %s" % (have, want)
    hs, sts = oracle_search(lzo, name, masked)
    if sum(len(h) for h in hs) == 0:
        return "no HSP at all"
    if "hsps" in r and tuple(len(h) for h in hs) != r["hsps"]:
        return "HSPs per strand %s, stated %s" % ([len(h) for h in hs], r["hsps"])
    if "raw" in r and tuple(st["raw_hits"] for st in sts) != r["raw"]:
        return "raw hits per strand %s, stated %s" % ([st["raw_hits"] for st in sts], r["raw"])
    if c["capacity"]:
        if any(st["raw_hits"] <= 2 * c["capacity"] for st in sts):
            return "fewer than three chunks of raw hits"
        for strand in (0, 1):                        # a wave of k_fill_hits2 / k_scan_hits2 lays the lists of 64 positions end to end
            n = hits_per_position(lzo, name, strand)
            if n.sum() != sts[strand]["raw_hits"]:
                return "strand %d: %d hits counted per position, %d raw hits" % (strand, n.sum(), sts[strand]["raw_hits"])
            least = 64 * int(n.min()) if r["waves"] == "all" else 64 * int(n.mean())
            if least <= LZ_F2_CAP:
                return "strand %d: %s 64 positions have %d hits, LZ_F2_CAP is %d" % (strand, "the lightest" if r["waves"] == "all" else "average", least, LZ_F2_CAP)
    if c["seq"] == "ends31":                         # the plus strand has a seed hit at either end of both sequences
        t, q = sequences("ends31")
        raw = oracle_search(lzo, name, masked, extend=False)[0][0]
        ends = {(int(h["pos1"]), int(h["pos2"])) for h in raw[(raw["pos2"] == 31) | (raw["pos2"] == len(q))]}
        if (31, 31) not in ends or (len(t), len(q)) not in ends:
            return "no seed hit on the first or on the last 31 bases of both sequences"
    if c["twin"]:
        tw = lzo.seed(c["twin"], c["trans"])
        if bytes(tw) != bytes(sd):
            return "the descriptor differs from that of " + c["twin"]
    return None


def heavy_reaches(lzo, masked):
    """heavy_blocks: the key has room for fewer block bits than the search wants, and there are more chunks than blocks"""
    c = CASES[HEAVY["case"]]
    tab, hs, sts = heavy_search(lzo, masked)
    nq = len(sequences(HEAVY["seq"])[1])
    weight = lzo.seed(c["pattern"], c["trans"]).weight
    for st in sts:
        est, want, have = want_block_bits(nq, int(tab.pt.contents.words_in_table), c["reach"]["probes"], weight, HEAVY["capacity"])
        if not (want > 32 - (weight + 1) and have == 3):
            return "est_hits %.0f: want_bits %d, room for %d" % (est, want, 32 - (weight + 1))
        if st["raw_hits"] <= (1 << have) * HEAVY["capacity"]:
            return "%d raw hits fit %d chunks of %d" % (st["raw_hits"], 1 << have, HEAVY["capacity"])
    if sum(len(h) for h in hs) == 0:
        return "no HSP at all"
    return None


# ---------------------------------------------------------------------------------------- the GPU child

def run(g, name):
    """tests/gpu_child.py: both strands of the case; a second run with extend=False where the case compares raw hits"""
    import helpers as H
    from oracle import lzo
    c = CASES[name]
    _, masked = H.scoring()
    g.set_hit_capacity(c["capacity"] or WHOLE)
    try:
        g.table_prepare(sequences(c["seq"])[0], g.seed(c["pattern"], c["trans"]), lzo.upper_nuc_to_bits(), step=c["step"])
        n = g.table_num_words()
        for extend in (True, False) if c["plain"] else (True,):
            r = H.search_strands(g, lambda q: g.seed_hit_search(masked, q=q, hsp_threshold=c["thr"], extend=extend), queries(name))
            yield dict(r, extend=extend, num_words=n)
    finally:
        g.set_hit_capacity(WHOLE)
