"""The cases of lzgpu_window_search (lastz_amd/csrc/window_kernels.hip) past one window per workgroup, and of the declines
the library takes after a search has begun: one table of inputs for tests/test_window_cases.py (CPU: the oracle alone, and
what every case is built to reach), tests/test_gpu_windows.py, tests/test_gpu_declines.py and the command-line test
tests/test_gpu_declines_cli.py.

The window kernel walks `for (wi = blockIdx.x; wi < n_wins; wi += gridDim.x)` with grid = min(n_windows, CUs): a block that
begins a second window finds what the first one left -- the cnt / dend union and pos[] in LDS, its start[] row in device
memory, the part[] words the short-batch path borrows.  The kernel is not shared with tests/emul, so the expected value is
always the oracle run on the cut-out pieces (want()), window by window, order included.

  many         1536 windows in one call, kinds drawn from a fixed RNG seed:
                 heavy       the target piece holds a run of 4300 A (more positions of one word than LZ_WIN_HITCAP: one
                             query position's list alone overflows the hit buffer, `take == 0`), the query piece 200-300 A
                 heavy_part  the same on a run of 2500 A: two query positions' lists overflow together (a partial `take`)
                 big         15,000-20,480 bases a side
                 small       50-2000 a side around an HSP of the whole pair, so that most hold homology
                 tiny        a side of 0, 3 or L - 1 bases
                 dup         an exact copy of an earlier window
  retry_small  8 windows, one of them 20,000 x 20,000: at threshold 600 more HSPs than the launcher's first room
               max(64 n, 4096); the same windows at 3000 right after
  edges        a 20480 x 20480 window on identical pieces (one HSP of length 20480: diagonal index q_len, diagEnd 20480 in
               16 bits), strictly inside an identical stretch of 27,000 bases: the HSP stops at all four edges of the
               window, not at the end of the homology; two oblong windows inside the same stretch, off its diagonal (the
               HSP runs from one edge to another); 60-base and 7-base copies in opposite corners of a window (the lowest
               and the highest diagonal index there is); the square, one oblong and the 60-base window again with both
               offsets shifted by 1, 2 and 3
  light        inner seeds of 4 to 12 bits and a spaced 14-bit one on windows around HSPs of the pair, sides capped per seed

The pair is tests/golden/synth200k.npz with plantings (pair()).  Its homologous blocks lie anywhere, so the small windows
are placed on the HSPs of the whole pair, not on the main diagonal.

The declines: seqio.synth_pair(30000, 30000, seed=9) with a run of 2000 A in the target and of 60 A in the query, default
seed.  decline_reach() recomputes on the oracle what the boundaries are: M, the most raw hits of one query position (hit
capacity M is searched, M - 1 declined with LZGPU_NH_HITS_OVERFLOW), and C, the candidates before entropy (HSP capacity C is
searched, C - 1 declined with LZGPU_NH_HSP_OVERFLOW).

(test infrastructure: data and helpers, no test in this file)"""
import numpy as np

from oracle import lzo
from lastz_amd import seqio
import helpers as H
import scorings as S
import chores_golden as CG
import word_limit_cases as W

LZ_WIN_TPB, LZ_WIN_MAXLEN, LZ_WIN_HITCAP = 256, 20480, 4096          # lastz_amd/csrc/window_kernels.hip
INNER = "1111111"
L = 7
A = ord("A")
EMPTY = np.zeros(0, dtype=lzo.HSP_DTYPE)
COUNTERS = ("words", "raw_hits", "extensions", "bp_extended", "hsps")

_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def masked():
    return H.scoring()[1]


# ---------------------------------------------------------------------------------------- the pair

RUN_LONG, RUN_SHORT = (30000, 4300), (70000, 2500)      # runs of A in the target: (start, length)
RUN_Q = (40000, 300)                                    # ... and in the query
SAME = (98000, 148000, 27000)                           # q[148000:175000] = t[98000:125000]
CORNERS60 = (60000, 5000, 10000, 3000)                  # a window with 60-base copies in opposite corners
CORNERS7 = (66000, 4000, 16000, 2500)                   # ... with 7-base copies, 700 points each: HSPs at threshold 600
WORD_LOW, WORD_HIGH = b"GCGCGCC", b"CGGCCGC"


def pair():
    def make():
        t, q = H.load_case("synth200k")
        t, q = t.copy(), q.copy()
        for s, n in (RUN_LONG, RUN_SHORT):
            t[s:s + n] = A
        q[RUN_Q[0]:RUN_Q[0] + RUN_Q[1]] = A
        ts, qs, n = SAME
        q[qs:qs + n] = t[ts:ts + n]
        t0, tl, q0, ql = CORNERS60
        q[q0 + ql - 60:q0 + ql] = t[t0:t0 + 60]                 # target-piece start / query-piece end
        q[q0:q0 + 60] = t[t0 + tl - 60:t0 + tl]                 # target-piece end / query-piece start
        t0, tl, q0, ql = CORNERS7
        t[t0:t0 + L] = np.frombuffer(WORD_LOW, dtype=np.uint8); q[q0 + ql - L:q0 + ql] = t[t0:t0 + L]
        t[t0 + tl - L:t0 + tl] = np.frombuffer(WORD_HIGH, dtype=np.uint8); q[q0:q0 + L] = t[t0 + tl - L:t0 + tl]
        return t, q
    return _once("pair", make)


def pair_hsps():
    """the HSPs of the whole pair under the default seed, without those of the runs of A: where the homology lies"""
    def make():
        hs = lzo.seed_hit_search(lzo.Table(pair()[0], lzo.seed()), pair()[1], masked())[0]
        b2 = hs["pos2"].astype(np.int64) - hs["length"]
        return hs[(hs["pos2"] <= RUN_Q[0]) | (b2 >= RUN_Q[0] + RUN_Q[1])]
    return _once("pair_hsps", make)


def want(win, thr, pattern=INNER, m=None, seqs=None):
    """the oracle on the cut-out pieces of one window; a piece shorter than the seed: nothing"""
    t, q = seqs or pair()
    osd = lzo.seed(pattern, 0)
    t0, tl, q0, ql = win
    if tl < osd.length or ql < osd.length:
        return EMPTY
    return lzo.seed_hit_search(lzo.Table(t[t0:t0 + tl], osd), q[q0:q0 + ql], masked() if m is None else m,
                               hsp_threshold=thr, entropic=False)[0]


def expected(case, thr):
    """[HSP array per window] of a case at a threshold, computed once and shared by the tests"""
    c = CASES[case]
    return _once(("want", case, thr), lambda: [want(w, thr, c.get("pattern", INNER)) for w in c["windows"]()])


def differs(got, wanted):
    """None if the lists of HSP arrays are equal window by window, order included; else the first window that differs"""
    if len(got) != len(wanted):
        return -1
    for k, (g, w) in enumerate(zip(got, wanted)):
        if len(g) != len(w) or not bool((g == w).all()):
            return k
    return None


# ---------------------------------------------------------------------------------------- many

N_MANY, MANY_SEED, N_BIG, N_DUP = 1536, 7, 14, 12
TRANSITIONS = (("heavy", "small"), ("small", "heavy"), ("big", "small"))


def _clip(x, lo, hi):
    return int(min(max(int(x), lo), hi))


def _small(rng, hs, t, q):
    h = hs[int(rng.integers(0, len(hs)))]
    tl, ql = int(rng.integers(50, 2001)), int(rng.integers(50, 2001))
    c1, c2 = int(h["pos1"]) - int(h["length"]) // 2, int(h["pos2"]) - int(h["length"]) // 2
    j = rng.integers(-30, 31, 2)
    return (_clip(c1 - tl // 2 + j[0], 0, len(t) - tl), tl, _clip(c2 - ql // 2 + j[1], 0, len(q) - ql), ql)


def _heavy(rng, run):
    s, n = run
    a, b = int(rng.integers(20, 400)), int(rng.integers(20, 400))
    lead, k = int(rng.integers(20, 300)), int(rng.integers(200, 301))
    return (s - a, a + n + b, RUN_Q[0] - lead, lead + k)


def many():
    """-> (windows, kinds)"""
    def make():
        t, q = pair()
        hs = pair_hsps()
        rng = np.random.default_rng(MANY_SEED)
        u = rng.random(N_MANY)
        kinds = np.where(u < 0.05, "heavy", np.where(u < 0.065, "heavy_part", np.where(u < 0.085, "tiny", "small"))).astype(object)
        kinds[rng.choice(N_MANY, N_BIG, replace=False)] = "big"
        kinds[rng.choice(np.arange(N_MANY // 2, N_MANY), N_DUP, replace=False)] = "dup"
        wins, n_tiny = [], 0
        for k in range(N_MANY):
            kind = kinds[k]
            if kind == "heavy":
                w = _heavy(rng, RUN_LONG)
            elif kind == "heavy_part":
                w = _heavy(rng, RUN_SHORT)
            elif kind == "big":
                tl, ql = (int(x) for x in rng.integers(15000, LZ_WIN_MAXLEN + 1, 2))
                w = (int(rng.integers(126000, len(t) - tl)), tl, int(rng.integers(45000, 125000)), ql)
            elif kind == "tiny":
                w = list(_small(rng, hs, t, q))
                w[1 if n_tiny % 2 == 0 else 3] = (0, 3, L - 1)[(n_tiny // 2) % 3]
                w, n_tiny = tuple(w), n_tiny + 1
            elif kind == "dup":
                w = wins[int(rng.integers(0, k))]
            else:
                w = _small(rng, hs, t, q)
            wins.append(w)
        return wins, [str(k) for k in kinds]
    return _once("many", make)


def transitions_missing(kinds, gmax):
    """With a grid of g blocks, block b runs the windows b, b + g, b + 2g, ... in that order: window i + g follows window i
    in the same block.  -> the (g, first kind, next kind) of TRANSITIONS that no block runs, for any g of 1 .. gmax"""
    k = np.array(kinds, dtype=object)
    out = []
    for g in range(1, gmax + 1):
        a, b = k[:-g], k[g:]
        out += [(g, x, y) for x, y in TRANSITIONS if not bool(((a == x) & (b == y)).any())]
    return out


def longest_word_list(piece, pattern=INNER):
    """entries of the longest list of the piece's table"""
    return int(W.list_lengths(lzo.Table(piece, lzo.seed(pattern, 0))).max())


# ---------------------------------------------------------------------------------------- retry_small, edges, light

BIG_UNRELATED = (130000, 20000, 60000, 20000)


def retry_small():
    wins, kinds = many()
    small = [w for w, k in zip(wins, kinds) if k == "small"]
    return small[:3] + [BIG_UNRELATED] + small[3:7]


def _shift(w, s):
    return (w[0] + s, w[1], w[2] + s, w[3])


IDENTICAL = (100000, LZ_WIN_MAXLEN, 150000, LZ_WIN_MAXLEN)
IDENTICAL_SCORE = 1955354                               # the oracle's score of t[100000:120480] against itself
INSIDE = [(102000, LZ_WIN_MAXLEN, 152037, 15000), (103000, 12000, 152950, LZ_WIN_MAXLEN)]


def edges():
    wins = [IDENTICAL] + INSIDE + [CORNERS60, CORNERS7]
    for s in (1, 2, 3):
        wins += [_shift(IDENTICAL, s), _shift(INSIDE[0], s), _shift(CORNERS60, s)]
    return wins


#        pattern       longest side (a window's raw hits stay under about 400,000)
LIGHT = {"11":         600,
         "111":        1500,
         "1111":       3000,
         "11111":      20000,
         "111111":     LZ_WIN_MAXLEN,
         "1110010111": LZ_WIN_MAXLEN}          # 14 bits, spaced
LIGHT_THR = 1500                               # unrelated pieces have no HSP at 1500 or above: what is found is homology


def light_windows(pattern):
    """six rectangles around HSPs of the pair, sides of half the cap to the cap; the sequences' far ends; a target piece
    shorter than the seed"""
    def make():
        t, q = pair()
        hs, cap = pair_hsps(), LIGHT[pattern]
        rng = np.random.default_rng(len(pattern))
        wins = [(len(t) - cap, cap, len(q) - cap, cap), (40000, 1, 40000, cap)]
        for h in hs[np.linspace(0, len(hs) - 1, 6).astype(int)]:
            tl, ql = (int(x) for x in rng.integers(cap // 2, cap + 1, 2))
            c1, c2 = int(h["pos1"]) - int(h["length"]) // 2, int(h["pos2"]) - int(h["length"]) // 2
            wins.append((_clip(c1 - tl // 2, 0, len(t) - tl), tl, _clip(c2 - ql // 2, 0, len(q) - ql), ql))
        return wins
    return _once(("light", pattern), make)


CASES = {"many": dict(windows=lambda: many()[0], thresholds=(600, 2200)),
         "retry_small": dict(windows=retry_small, thresholds=(600, 3000)),
         "edges": dict(windows=edges, thresholds=(600, 2200))}
for _p in LIGHT:
    CASES["light_" + _p] = dict(windows=(lambda p=_p: light_windows(p)), thresholds=(LIGHT_THR,), pattern=_p)


# ---------------------------------------------------------------------------------------- declines after work has begun

HIT_CAPACITY_DEFAULT, HSP_CAPACITY_DEFAULT = 1 << 28, 1 << 24
T_IV, Q_IV = (9000, 13000), (4000, 7000)                # the position filter of the `within` searches: both runs of A inside
FENCES = (9000, 13000)                                  # the scripted sequence fences this target interval


def decline_pair():
    def make():
        t, q = seqio.synth_pair(30000, 30000, seed=9)
        t, q = t.copy(), q.copy()
        t[10000:12000] = A
        q[5000:5060] = A
        return t, q
    return _once("decline_pair", make)


def decline_table():
    return _once("decline_table", lambda: lzo.Table(decline_pair()[0], lzo.seed()))


def oracle_of(kind, **kw):
    """the oracle's (HSPs, counters) of the decline pair: kind "plain", "self" (the target against itself, same strand) or
    "within" (T_IV x Q_IV); kw as lzo.seed_hit_search takes them"""
    def make():
        t, q = decline_pair()
        if kind == "plain":
            return lzo.seed_hit_search(decline_table(), q, masked(), **kw)
        if kind == "self":
            return lzo.seed_hit_search(decline_table(), t, masked(), self_strand="same", **kw)
        return CG.oracle_hsps(t, q, T_IV, Q_IV, masked(), **kw)
    return _once(("oracle_of", kind, tuple(sorted(kw.items()))), make)


def decline_reach(kind="plain"):
    """-> dict(raw, M, over_1024, C, hsps): raw hits, the most of one query position and the positions with more than 1024
    (from the plain-hit mode, grouped by pos2), candidates before entropy, HSPs with it"""
    raw, st = oracle_of(kind, mode=1)
    per = np.bincount(raw["pos2"])
    return dict(raw=st["raw_hits"], M=int(per.max()), over_1024=int((per > 1024).sum()),
                C=len(oracle_of(kind, entropic=False)[0]), hsps=len(oracle_of(kind)[0]))


# the scripted sequence of tests/test_gpu_declines.py: searches, window searches under another matrix, a limited table and a
# fenced target in one process
SCRIPT_LIMIT = 7
SCRIPT_WINDOWS = [(9000, 5000, 4000, 3000), (0, 20000, 0, 20000), (20000, 10000, 15000, 8000)]
SCRIPT_THR = 2200


def limited_table(tab, limit):
    """tab as the searches see it under lzgpu_table_limit(limit): the limit goes by the whole target's lists"""
    by = W.list_lengths(decline_table())
    return W.limited(tab, limit, by=by)[0]


def script_oracle():
    """-> dict: `plain` and `limited` (HSPs, counters) of the whole search, `windows` [HSP array per window] under `eight`,
    `t_iv` / `q_iv` / `fenced` / `within`: a position filter around an HSP of the limited search, the target with that
    interval fenced, and the filtered search of it under the limit"""
    def make():
        t, q = decline_pair()
        sd = lzo.seed()
        out = dict(plain=oracle_of("plain"))
        out["limited"] = lzo.seed_hit_search(limited_table(lzo.Table(t, sd), SCRIPT_LIMIT), q, masked())
        out["windows"] = [want(w, SCRIPT_THR, m=eight(), seqs=(t, q)) for w in SCRIPT_WINDOWS]
        h = out["limited"][0][len(out["limited"][0]) // 2]
        t_iv = (_clip(int(h["pos1"]) - int(h["length"]) - 700, 1, len(t)), _clip(int(h["pos1"]) + 700, 1, len(t) - 1))
        q_iv = (_clip(int(h["pos2"]) - int(h["length"]) - 400, 0, len(q)), _clip(int(h["pos2"]) + 900, 0, len(q)))
        tf = CG.fenced(t, *t_iv)
        tab = limited_table(lzo.Table(tf, sd, start=t_iv[0], end=t_iv[1]), SCRIPT_LIMIT)
        out.update(t_iv=t_iv, q_iv=q_iv, fenced=tf, within=lzo.seed_hit_search(tab, q, masked(), start=q_iv[0], end=q_iv[1]))
        return out
    return _once("script", make)


def many_classes():
    """HOXD70's masked matrix with 40 more bytes that each score on their own: more than 32 row classes"""
    m = masked().copy()
    for k in range(40):
        m[128 + k, :] = -1000 - k
    return m


def row_classes(m):
    return len(np.unique(np.asarray(m), axis=0))


def eight():
    return S.m4_scoring(S.MATRICES["eight"])[1]
