"""The position-filter cases of tests/test_gpu_pos_filter.py (lzgpu_seed_hit_search_within; lastz --chores): for every case the
search it names, as library calls (run, for tests/gpu_child.py) and as the oracle states it (oracle_search): the search of
a table that holds only the words inside the target interval, over the search interval intersected with the query
interval, on the whole sequences.

The pair: target = self_cases.rep (40,000 bases; 150 copies of a 61-base unit at 8,000, of its reverse complement at
24,000, a palindromic stretch, poly-A, (AC)n), query = the target's two halves swapped with 3 % of the bases substituted
(22,000 bases of it in the cases that need no more) -- the lists of the unit's words hold 150 entries, and every query
position inside a copy meets all of them.  pairx: the same with self_cases.repx's N runs, lower case and IUPAC letters in the
target and N / lower case in the query; multi: the target laid out as a [multi] sequence of 36 records (NULs between them).

With L = 19 the first word of the unit ends at 8,019 + 61 k, k = 0 .. 149: the list's first entry (it is sorted by
descending position) is 17,108, its last 8,019.
"""
import numpy as np

from lastz_amd import seqio
import self_cases as S

DEFAULT_SEED = S.DEFAULT_SEED
COUNTERS = S.COUNTERS
WHOLE = S.WHOLE
L = 19
P_LAST, P_FIRST = 8_019, 8_000 + 61 * 149 + 19      # the end positions of the unit's first word: lowest and highest


def _query(t, n, seed, specials=False):
    rng = np.random.default_rng(seed)
    q = np.concatenate([t[len(t) // 2:], t[:len(t) // 2]])[:n].copy()
    q &= 0xDF                                                       # (upper case: the target's specials are not copied ...)
    q[~np.isin(q, S.ACGT)] = ord("A")                               # (... nor its IUPAC letters)
    sub = np.flatnonzero(rng.random(n) < 0.03)
    q[sub] = S.ACGT[rng.integers(0, 4, len(sub))]
    if specials:
        for at in rng.integers(0, n - 40, 12):
            q[int(at):int(at) + int(rng.integers(1, 30))] = ord("N")
        low = rng.random(n) < 0.01
        q[low] |= 0x20
    return q


_built = {}


def pair(name):
    """-> target bytes (as lastz holds them), query bytes"""
    if name not in _built:
        if name == "pair":
            t = S.rep(); _built[name] = (t, _query(t, 22_000, 201))
        elif name == "pairx":
            t = S.repx(); _built[name] = (t, _query(t, 22_000, 202, specials=True))
        elif name == "multi":
            t = S.rep(); _built[name] = (S.lay_out(t, S.RAGGED)[0], _query(t, 22_000, 203))
        elif name == "pair20":
            t = S.rep20(); _built[name] = (t, _query(t, 12_000, 204))
    return _built[name]


def _case(seq="pair", t_iv=(0, 1 << 30), q_iv=(0, 1 << 30), start=0, end=0, pattern=DEFAULT_SEED, trans=1, step=1, extend=True,
          capacity=None, force_mode=0, mode=0, empty=False, min_chunks=1):
    return dict(seq=seq, t_iv=t_iv, q_iv=q_iv, start=start, end=end, pattern=pattern, trans=trans, step=step, extend=extend,
                capacity=capacity, force_mode=force_mode, mode=mode, empty=empty, min_chunks=min_chunks, strands=("+", "-"))


INSIDE = (8_000 + 61 * 40 + 7, 8_000 + 61 * 110 + 30)               # cuts the 150-entry lists inside on both ends
# mode: the scan mode the library is to report (0 clean sequences, 1 special bytes or forced, 2 forced or nothing extended);
# empty: no window fits -- the entry point returns before any search, and the scan mode is not looked at
CASES = {
    "inside":        _case(t_iv=INSIDE),
    "inside_q":      _case(t_iv=INSIDE, q_iv=(3_000, 15_000)),
    "whole":         _case(t_iv=(0, 40_000), q_iv=(0, 22_000)),
    "whole_clamped": _case(t_iv=(0, 0xFFFFFFFF), q_iv=(0, 0xFFFFFFFF)),
    "one_seed":      _case(t_iv=(P_LAST + 61 * 70 - L, P_LAST + 61 * 70)),
    "l_minus_1":     _case(t_iv=(P_LAST + 61 * 70 - L, P_LAST + 61 * 70 - 1), empty=True),
    "q_one_seed":    _case(t_iv=INSIDE, q_iv=(9_000, 9_000 + L)),
    "q_l_minus_1":   _case(t_iv=INSIDE, q_iv=(9_000, 9_000 + L - 1), empty=True),
    "t_empty":       _case(t_iv=(12_000, 12_000), empty=True),
    "q_outside":     _case(t_iv=INSIDE, q_iv=(10_000, 12_000), start=14_000, empty=True),
    "first_m1":      _case(t_iv=(2_000, P_FIRST - 1)),              # the window's end on the list's first (highest) entry, +- 1
    "first_0":       _case(t_iv=(2_000, P_FIRST)),
    "first_p1":      _case(t_iv=(2_000, P_FIRST + 1)),
    "last_m1":       _case(t_iv=(P_LAST - L - 1, 30_000)),          # the window's start on the list's last (lowest) entry, +- 1
    "last_0":        _case(t_iv=(P_LAST - L, 30_000)),
    "last_p1":       _case(t_iv=(P_LAST - L + 1, 30_000)),
    # three or more chunks of surviving hits (a chunk holds at most `capacity` of them; positions without any make no
    # chunk); the query interval begins and ends inside the copies of the unit, where every position has survivors, so
    # that it ends inside a chunk and an unfiltered search is past its first chunk where the interval begins
    "chunks":        _case(t_iv=INSIDE, q_iv=(6_000, 13_333), capacity=4096, min_chunks=3),
    "chunks_start":  _case(t_iv=INSIDE, q_iv=(0, 13_333), start=2_500, end=20_000, capacity=50_000, min_chunks=3),
    "m1":            _case(t_iv=INSIDE, force_mode=1, mode=1),
    "m2":            _case(t_iv=INSIDE, force_mode=2, mode=2),
    "specials":      _case(seq="pairx", t_iv=INSIDE, q_iv=(1_000, 21_000), mode=1),
    "specials_m2":   _case(seq="pairx", t_iv=INSIDE, force_mode=2, mode=2),
    "multi":         _case(seq="multi", t_iv=(8_000, 15_000), mode=1),
    "probes_1":      _case(seq="pair20", t_iv=(4_000 + 61 * 10 + 5, 4_000 + 61 * 30 + 40), trans=0),
    "probes_79":     _case(seq="pair20", t_iv=(4_000 + 61 * 10 + 5, 4_000 + 61 * 30 + 40), trans=2),
    "stepped":       _case(seq="pair20", t_iv=(4_000 + 61 * 10 + 5, 4_000 + 61 * 30 + 40), pattern="111101101111", step=3),
    "plainhits":     _case(seq="pair20", t_iv=(4_000 + 61 * 10 + 5, 4_000 + 61 * 30 + 40), q_iv=(500, 9_000), extend=False, mode=2),
}
SPLIT_CASES = ["inside", "inside_q", "first_0", "last_0", "chunks", "probes_79", "stepped"]
UNFILTERED_TWINS = ["whole", "whole_clamped"]


def queries(name):
    t, q = pair(CASES[name]["seq"])
    return t, (q, seqio.revcomp(q))


def run(g, name):
    """tests/gpu_child.py: the case's two strands, one run"""
    import helpers as H
    from oracle import lzo
    c = CASES[name]
    t, qs = queries(name)
    _, masked = H.scoring()
    g.set_scan_mode(c["force_mode"])
    g.set_hit_capacity(c["capacity"] or WHOLE)
    try:
        g.table_prepare(t, g.seed(c["pattern"], c["trans"]), lzo.upper_nuc_to_bits(), step=c["step"])
        run = H.search_strands(g, lambda q: g.seed_hit_search_within(masked, c["t_iv"], c["q_iv"], q=q, start=c["start"], end=c["end"],
                                                                     extend=c["extend"]), qs)
    finally:
        g.set_hit_capacity(WHOLE)
        g.set_scan_mode(0)
    yield dict(run, capacity=c["capacity"])


def intersect(c, tlen, qlen, seed_len):
    """-> the table's interval and the search interval of the restricted search, or None where no window fits"""
    ts, te = c["t_iv"][0], min(c["t_iv"][1], tlen)
    lo, hi = c["start"], c["end"] or qlen
    qs, qe = max(lo, c["q_iv"][0]), min(hi, c["q_iv"][1])
    if te < ts + seed_len or qe < qs + seed_len:
        return None
    return (ts, te), (qs, qe)


def oracle_search(lzo, name, masked, filtered=True):
    """the oracle's statement of a case: ([HSP array per strand], counters summed over the strands).  filtered=False: the
    plain search of the same pair over the case's search interval."""
    c = CASES[name]
    t, qs = queries(name)
    sd = lzo.seed(c["pattern"], c["trans"])
    hs, tot = [], dict.fromkeys(COUNTERS, 0)
    iv = intersect(c, len(t), len(qs[0]), sd.length) if filtered else ((0, 0), (c["start"], c["end"]))
    if iv is None:
        return [np.zeros(0, dtype=lzo.HSP_DTYPE) for _ in qs], tot
    tab = lzo.Table(t, sd, step=c["step"], start=iv[0][0], end=iv[0][1])
    for q in qs:
        h, st = lzo.seed_hit_search(tab, q, masked, mode=0 if c["extend"] else 1, start=iv[1][0], end=iv[1][1])
        hs.append(h)
        for k in COUNTERS:
            tot[k] += st[k]
    return hs, tot
