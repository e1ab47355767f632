"""Score matrices other than HOXD70, shared by tests/test_scorings.py (CPU) and tests/test_gpu_scorings.py (GPU).

The library promises the reference's output under any matrix of at most 32 x 32 classes, any xDrop and any gap penalties
(DESIGN.md 1).  HOXD70 is symmetric, so it cannot tell which of the two sequences supplies the low bit `w` of the look-up
tables' index F[x][w] (lz_host.cpp: lut_classes), and it stays far from every limit of the fast-path predicate.  The family
here is strand-symmetric (M[a][b] == M[comp a][comp b], what the tables need) but not symmetric, and sits on the limits:
score bytes of +-127, -3 * min(M) == xDrop, xDrop == 15000, and the DP's 16-bit-row rule at its last admitted y-drop.

(test infrastructure: data and two helpers, no test in this file)"""
import re

import numpy as np

from oracle import lzo
from lastz_amd import seqio

NUC = "ACGT"
COMP = {0: 3, 1: 2, 2: 1, 3: 0}


def orbit(aa, cc, ac, ca, ag, ga, at, cg):
    """4 x 4 matrix over A, C, G, T (row: target base, column: query base) that is invariant under complementing both
    bases; one argument per orbit: AA/TT, CC/GG, A->C/T->G, C->A/G->T, A->G/T->C, G->A/C->T, AT/TA, CG/GC"""
    A, Cc, G, T = 0, 1, 2, 3
    m = np.zeros((4, 4), dtype=np.int32)
    for v, cells in ((aa, ((A, A), (T, T))), (cc, ((Cc, Cc), (G, G))), (ac, ((A, Cc), (T, G))), (ca, ((Cc, A), (G, T))),
                     (ag, ((A, G), (T, Cc))), (ga, ((G, A), (Cc, T))), (at, ((A, T), (T, A))), (cg, ((Cc, G), (G, Cc)))):
        for r, c in cells:
            m[r, c] = v
    assert all(m[a, b] == m[COMP[a], COMP[b]] for a in range(4) for b in range(4))
    return m


def m4_scoring(M4, bad=-1000, fill=-100):
    """(scoring, maskedScoring) as int32[256, 256] for a 4 x 4 matrix, the way lzo.hoxd70_scoring builds them"""
    import ctypes as C
    t = (C.c_int32 * 16)(*[int(v) for v in np.asarray(M4).reshape(16)])
    sub = np.zeros((256, 256), dtype=np.int32)
    lzo.lib().lzo_dna_score_set(t, bad, fill, lzo._ptr(sub))
    masked = np.zeros((256, 256), dtype=np.int32)
    lzo.lib().lzo_masked_score_set(lzo._ptr(sub), lzo._ptr(masked))
    return sub, masked


def score_file_text(M4, bad=-1000, fill=-100):
    """the matrix as a --scores=<file> of the reference (settings only: scores and the two default scores)"""
    M4 = np.asarray(M4)
    lines = ["bad_score          = X:%d" % bad, "fill_score         = %d" % fill, "",
             "  " + "".join("%6s" % c for c in NUC)]
    for r in range(4):
        lines.append(NUC[r] + " " + "".join("%6d" % int(M4[r, c]) for c in range(4)))
    return "\n".join(lines) + "\n"


def parse_score_file(text):
    """-> (M4, bad, fill) of a file score_file_text wrote (or any --scores file over A, C, G, T)"""
    bad, fill, cols, rows = -1000, -100, None, {}
    for line in text.split("\n"):
        line = line.split("#")[0].strip()
        if not line:
            continue
        m = re.match(r"(\w+)\s*=\s*(?:\w:)?(-?\d+)$", line)
        if m:
            if m.group(1) == "bad_score": bad = int(m.group(2))
            if m.group(1) == "fill_score": fill = int(m.group(2))
            continue
        f = line.split()
        if cols is None:
            cols = f
        else:
            rows[f[0]] = [int(x) for x in f[1:]]
    M4 = np.array([[rows[r][cols.index(c)] for c in NUC] for r in NUC], dtype=np.int32)
    return M4, bad, fill


HOXD70 = orbit(91, 100, -114, -114, -31, -31, -123, -125)


def _hox_tt80():
    m = HOXD70.copy(); m[3, 3] = 80
    return m


MATRICES = {
    "eight": orbit(91, 100, -114, -60, -31, -75, -123, -125),          # all eight F[x][w] distinct, M != M^T
    "unit": orbit(1, 1, -1, -1, -1, -1, -1, -1),
    "ext": orbit(127, 127, -127, -127, -127, -127, -127, -127),
    "hoxd70": HOXD70,
    "s128": orbit(128, 100, -114, -114, -31, -31, -123, -125),         # one score outside the signed byte
    "nonsym": _hox_tt80(),                                             # not invariant under complementing both bases
    "mis0": orbit(10, 10, 0, 0, 0, 0, 0, 0),
}

PAIRS = {            # key -> (CPU pair, GPU pair) as arguments of seqio.synth_pair
    "main": (dict(tlen=60_000, qlen=50_000, seed=5, block_min=300, block_max=3000),
             dict(tlen=300_000, qlen=250_000, seed=5, block_min=300, block_max=3000)),
    "x15000": (dict(tlen=100_000, qlen=100_000, seed=9, block_min=300, block_max=3000),) * 2,
    "mis0": (dict(tlen=20_000, qlen=20_000, seed=9, block_min=300, block_max=3000),) * 2,
}

#  name        matrix     xdrop  hsp_threshold  expected scan mode  pair
SEED_CASES = {
    "eight":    ("eight",  910,   3000, 0, "main"),
    "unit":     ("unit",   3,     22,   0, "main"),      # -3 * min == xDrop
    "unit_x2":  ("unit",   2,     22,   2, "main"),      # one below the rule
    "ext":      ("ext",    381,   4000, 0, "main"),
    "ext_x380": ("ext",    380,   4000, 2, "main"),
    "x15000":   ("hoxd70", 15000, 3000, 0, "x15000"),    # B' at the top of its s16 range; three windows, k_scan_tasks, SLOW
    "x15001":   ("hoxd70", 15001, 3000, 2, "x15000"),
    "s128":     ("s128",   910,   3000, 2, "main"),
    "nonsym":   ("nonsym", 910,   3000, 2, "main"),
    "mis0":     ("mis0",   5,     300,  0, "mis0"),      # no scan stops on its own: sequence ends and diagEnd only
}
ELIGIBLE = [k for k, v in SEED_CASES.items() if v[3] == 0]
GOLDEN_MATRICES = ("eight", "unit", "ext")


def seed_case(name, gpu=False, specials=False):
    """-> (t, q, masked, kw of seed_hit_search, expected scan mode) of one seed-stage row"""
    mname, xdrop, thr, mode, pair = SEED_CASES[name]
    t, q = seqio.synth_pair(**PAIRS[pair][1 if gpu else 0])
    if specials:
        t, q = with_specials(t, q)
        mode = max(mode, 1)
    _, masked = m4_scoring(MATRICES[mname])
    return t, q, masked, dict(xdrop=xdrop, hsp_threshold=thr), mode


CHUNK_CAPACITY = 20_000


def split_case(case):
    """a case of tests/gpu_child.py: a row's name, with `.s` for its variant with special bytes or `.c` for the run in chunks of
    at most CHUNK_CAPACITY hits -> (name, specials, chunks)"""
    name, _, variant = case.partition(".")
    return name, variant == "s", variant == "c"


def run(g, case):
    import helpers as H
    name, specials, chunks = split_case(case)
    t, q, masked, kw, _ = seed_case(name, gpu=True, specials=specials)
    g.table_prepare(t, g.seed(H.DEFAULT_SEED, 1), lzo.upper_nuc_to_bits())
    if chunks:
        g.set_hit_capacity(CHUNK_CAPACITY)
    try:
        yield H.search_strands(g, lambda qq: g.seed_hit_search(masked, q=qq, **kw), [qq for _, _, qq in H.strands(q)])
    finally:
        if chunks:
            g.set_hit_capacity(1 << 28)


def with_specials(t, q, seed=4):
    """N runs, lower case, IUPAC bytes single and in runs sprinkled into both sequences (as
    test_emul_vs_oracle.test_lut_scans_through_special_bytes_that_do_not_end_a_scan does, thinner: the cases still need HSPs)"""
    rng = np.random.default_rng(seed)
    t = t.copy(); q = q.copy()
    iupac = np.frombuffer(b"RYKMSWBDHV", dtype=np.uint8)
    for arr in (t, q):
        n = len(arr)
        idx = rng.integers(0, n, n // 150)
        arr[idx] = iupac[rng.integers(0, len(iupac), len(idx))]          # single IUPAC bytes
        for s in rng.integers(0, n - 20, max(4, n // 3000)):
            k = int(rng.integers(2, 12))
            arr[s:s + k] = iupac[rng.integers(0, len(iupac), k)]         # IUPAC runs
        arr[rng.integers(0, n, n // 300)] |= 0x20                        # lower case
        for s in rng.integers(0, n - 50, max(3, n // 10000)):
            arr[s:s + int(rng.integers(1, 40))] = ord("N")               # N runs
    return t, q


# ---- DP cases.  HSPs come from the oracle's search under `hsp` (matrix of the masked scoring, xdrop, threshold).
DP_PAIR = dict(tlen=30_000, qlen=26_000, seed=5, block_min=300, block_max=3000)
SPECIAL_MAX = 2000
#  name               sub          hsp search               gap / drop parameters                                         expectation
DP_CASES = {
    "eight":          ("eight",    ("eight", 910, 3000),  dict(gap_open=400, gap_extend=30, ydrop=9400, thresh=3000),     None),
    "unit":           ("unit",     ("unit", 3, 22),       dict(gap_open=4, gap_extend=1, ydrop=20, thresh=25),            None),
    "unit_wide":      ("unit",     ("unit", 3, 22),       dict(gap_open=2, gap_extend=1, ydrop=600, thresh=25),           "wide"),
    "ext":            ("ext",      ("ext", 381, 4000),    dict(gap_open=500, gap_extend=40, ydrop=12000, thresh=4000),    None),
    # 61383 + (2500 + 500) + 1025 + 127 == 65535: the last y-drop the 16-bit row admits, and the first it does not
    "ext_row16_last": ("ext",      ("ext", 381, 4000),    dict(gap_open=2500, gap_extend=500, ydrop=61383, thresh=4000),  "row16"),
    "ext_row16_over": ("ext",      ("ext", 381, 4000),    dict(gap_open=2500, gap_extend=500, ydrop=61384, thresh=4000),  "row32"),
    "many_class":     ("many",     ("hoxd70", 910, 3000), dict(gap_open=400, gap_extend=30, ydrop=9400, thresh=3000),     None),
    # the rule's max(score) is a special class's score (R against R: 2000), not a nucleotide's
    "special_max_last": ("special", ("hoxd70", 910, 3000),
                         dict(gap_open=2500, gap_extend=500, ydrop=65535 - 1025 - SPECIAL_MAX - 3000, thresh=3000),       "row16"),
    "special_max_over": ("special", ("hoxd70", 910, 3000),
                         dict(gap_open=2500, gap_extend=500, ydrop=65535 - 1025 - SPECIAL_MAX - 3000 + 1, thresh=3000),   "row32"),
}


def dp_case(name):
    """-> (t, q, sub, masked of the HSP search, (xdrop, hsp_threshold), kw, expectation)"""
    import helpers as H
    sname, (hm, xdrop, thr), kw, expect = DP_CASES[name]
    t, q = seqio.synth_pair(**DP_PAIR)
    _, masked = m4_scoring(MATRICES[hm])
    if sname == "many":
        q = q.copy(); q[::53] = ord("R"); q[7::61] = ord("Y"); q[3000:3500] |= 0x20; q[11::97] = ord("N")
        sub = H.many_class_scoring()
    elif sname == "special":
        # R runs in both sequences: at random places, and facing each other in the middle of the plain pair's first HSPs
        # of the forward strand, so that alignments run through R against R cells
        hs, _ = lzo.seed_hit_search(lzo.Table(t, lzo.seed()), q, masked, xdrop=xdrop, hsp_threshold=thr)
        t = t.copy(); q = q.copy()
        rng = np.random.default_rng(6)
        for arr in (t, q):
            for s in rng.integers(0, len(arr) - 40, 30):
                arr[s:s + int(rng.integers(1, 12))] = ord("R")
        for h in hs[:12]:
            back = int(h["length"]) // 2
            t[int(h["pos1"]) - back:int(h["pos1"]) - back + 2] = ord("R")
            q[int(h["pos2"]) - back:int(h["pos2"]) - back + 2] = ord("R")
        sub, _ = m4_scoring(HOXD70)
        sub = sub.copy(); sub[ord("R"), ord("R")] = SPECIAL_MAX
    else:
        sub, _ = m4_scoring(MATRICES[sname])
    return t, q, sub, masked, (xdrop, thr), dict(kw), expect
