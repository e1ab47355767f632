"""The self-comparison cases of tests/test_self_oracle.py (CPU) and tests/test_gpu_self_matrix.py (GPU): small repetitive
sequences built from fixed seeds, and for every case the search it names -- as oracle keywords, as library calls and,
where lastz's command line can say it, as arguments of the pristine binary (tools/make_self_golden.py records those).

  rep     40,000 random A/C/G/T; at 8,000 150 copies of a random 61-base unit, at 24,000 150 copies of its reverse
          complement, at 34,000 14 copies of the unit followed by its reverse complement, at 36,000 300 x A, at
          37,000 200 x AC.  The table's lists of the repeats' words hold ~150 entries, so a self-comparison cuts
          INSIDE lists, and the hits of a wave's 64 positions run to several pieces of the fill kernels' LDS buffer.
          (The palindromic copies are what cuts lists on the OPPOSITE strand of an unpartitioned sequence: there a
          list is cut at the mirror image of the query position, so a word and its reverse complement must lie in one
          stretch.  The direct and the inverted copies alone are kept or dropped whole on that strand.)
  rep20   the same recipe at half the length with 40 and 7 copies (at 4,000 / 12,000 / 17,000 / 18,000 / 18,500), for
          heavy seeds
  repx    rep with 40 runs of 1-40 N, 1 % lower case and 0.5 % IUPAC letters, some of them inside the repeats
"""
import numpy as np

from lastz_amd import seqio

DEFAULT_SEED = "1110100110010101111"
COUNTERS = ("words", "raw_hits", "extensions", "bp_extended", "hsps")
RAGGED = [5, 19, 7000, 1, 12000] + [300] * 30          # + the rest of rep: 36 records, some no longer than the seed
CHUNK_CAPACITIES = (4096, 50_000)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rep(n, copies, pal, seed):
    rng = np.random.default_rng(seed)
    s = ACGT[rng.integers(0, 4, n)].copy()
    unit = ACGT[rng.integers(0, 4, 61)]
    at = n // 5
    s[at:at + 61 * copies] = np.tile(unit, copies)
    at = 3 * n // 5
    s[at:at + 61 * copies] = np.tile(seqio.revcomp(unit), copies)
    at = 17 * n // 20
    s[at:at + 122 * pal] = np.tile(np.concatenate([unit, seqio.revcomp(unit)]), pal)
    at = 9 * n // 10
    s[at:at + 300] = ord("A")
    at = 37 * n // 40
    s[at:at + 400] = np.frombuffer(b"AC" * 200, dtype=np.uint8)
    return s


def rep():
    return _rep(40_000, 150, 14, seed=101)


def rep20():
    return _rep(20_000, 40, 7, seed=102)


def repx():
    s = rep()
    rng = np.random.default_rng(103)
    n = len(s)
    starts = list(rng.integers(0, n - 40, 36)) + [8_000 + 61 * 20 + 7, 8_000 + 61 * 90, 24_000 + 61 * 75 + 30, 36_100]
    for at in starts:                                                  # 40 N runs, four of them inside the repeats
        s[int(at):int(at) + int(rng.integers(1, 41))] = ord("N")
    low = rng.random(n) < 0.01
    s[low] |= 0x20
    iupac = np.frombuffer(b"RYKMSWBDHV", dtype=np.uint8)
    amb = np.flatnonzero(rng.random(n) < 0.005)
    s[amb] = iupac[rng.integers(0, len(iupac), len(amb))]
    for at, ch in ((8_000 + 61 * 50 + 11, "R"), (24_000 + 61 * 10 + 3, "y"), (36_200, "a"), (37_100, "M")):
        s[at] = ord(ch)
    return s


SEQS = {"rep": rep, "rep20": rep20, "repx": repx}


def lay_out(seq, records):
    """a [multi] sequence as lastz holds it (src/sequences.c:1896-1931): NUL, record, NUL, record, ...; -> (bytes,
    separators = the partitions' sepBefore values + the final NUL, one past the end).  records: the lengths of all
    records but the last, which takes the rest; None: one sequence, no partitions."""
    if records is None:
        return seq, []
    lens = list(records) + [len(seq) - sum(records)]
    assert lens[-1] > 0
    seps, at = [0], 0
    for n in lens:
        at += n + 1
        seps.append(at)
    v = np.zeros(at, dtype=np.uint8)
    cuts = np.cumsum([0] + lens)
    for k in range(len(lens)):
        v[seps[k] + 1:seps[k + 1]] = seq[cuts[k]:cuts[k + 1]]
    return v, seps


def minus(v, seps):
    """the reverse strand as lastz makes it: the whole sequence, or every partition on its own"""
    if not seps:
        return seqio.revcomp(v)
    q = v.copy()
    for k in range(len(seps) - 1):
        q[seps[k] + 1:seps[k + 1]] = seqio.revcomp(v[seps[k] + 1:seps[k + 1]])
    return q


def _case(seq="rep", records=None, band=0, pattern=DEFAULT_SEED, trans=1, step=1, extend=True, xdrop=910,
          hsp_threshold=3000, entropic=True, capacities=(None,), force_mode=0, mode=0, cli=None, twin=None):
    return dict(seq=seq, records=records, band=band, pattern=pattern, trans=trans, step=step, extend=extend, xdrop=xdrop,
                hsp_threshold=hsp_threshold, entropic=entropic, capacities=capacities, force_mode=force_mode, mode=mode,
                cli=cli, twin=twin, strands=("+",) if band else ("+", "-"))


def _band(b):
    return _case(band=b, cli=["--strand=plus", "--band=%d" % b])


# mode: the scan mode the library is to report (0 clean sequence, 1 special bytes -- a [multi] layout's NULs are such --
# or the forced one; a search that extends nothing scans nothing and reports 2).  cli: what the case adds to
# `lastz <file> --self --nogapped --nomirror`, None where the command line cannot say it (library settings, specials
# lastz would not read from FASTA).  twin: the case whose rows a chunked case must reproduce with more launches.
CASES = {
    "rep":             _case(cli=[]),
    "rep_b1":          _band(1),
    "rep_b61":         _band(61),
    "rep_b500":        _band(500),
    "rep_b40000":      _band(40_000),
    "rep_chunks":      _case(capacities=CHUNK_CAPACITIES, twin="rep"),
    "rep_b500_chunks": _case(band=500, capacities=CHUNK_CAPACITIES, twin="rep_b500"),
    "rep_m1":          _case(force_mode=1, mode=1),
    "rep_m2":          _case(force_mode=2, mode=2),
    "repx":            _case(seq="repx", mode=1),
    "repx_m2":         _case(seq="repx", force_mode=2, mode=2),
    "seed_t0":         _case(seq="rep20", trans=0, cli=["--notransition"]),
    "seed_t2":         _case(seq="rep20", trans=2, cli=["--transition=2"]),
    "seed_7":          _case(seq="rep20", pattern="1111111", trans=0, cli=["--seed=1111111", "--notransition"]),
    "seed_12s3":       _case(seq="rep20", pattern="111101101111", trans=1, step=3, cli=["--seed=111101101111", "--step=3"]),
    "plainhits":       _case(seq="rep20", extend=False, mode=2),
    "scoring":         _case(xdrop=500, hsp_threshold=2000, cli=["--xdrop=500", "--hspthresh=2000"]),
    "scoring_noent":   _case(xdrop=500, hsp_threshold=2000, entropic=False, cli=["--xdrop=500", "--hspthresh=2000", "--noentropy"]),
    "multi_ragged":    _case(records=RAGGED, mode=1, cli=[]),
    "multi_one":       _case(seq="rep20", records=[], mode=1, cli=[]),
    "multi_chunks":    _case(records=RAGGED, mode=1, capacities=(4096,), twin="multi_ragged"),
}
SPLIT_CASES = ["rep", "rep_b500", "rep_b500_chunks", "seed_t2", "multi_ragged"]
CLIPPING = [k for k in CASES if k.startswith(("rep", "multi"))]
BANDED = [k for k in CASES if CASES[k]["band"]]

_built = {}


def sequence(name):
    """-> (bytes as lastz holds them, separators or [], the plain sequence, the record lengths or None)"""
    c = CASES[name]
    key = (c["seq"], None if c["records"] is None else tuple(c["records"]))
    if key not in _built:
        s = SEQS[c["seq"]]()
        _built[key] = lay_out(s, c["records"]) + (s,)
    v, seps, s = _built[key]
    return v, seps, s


WHOLE = 1 << 28                                     # the hit capacity that chunks nothing here


def run(g, name):
    """tests/gpu_child.py: one run per hit capacity of the case"""
    import helpers as H
    from oracle import lzo
    c = CASES[name]
    v, seps, _ = sequence(name)
    _, masked = H.scoring()
    for capacity in c["capacities"]:
        g.set_scan_mode(c["force_mode"])
        g.set_hit_capacity(capacity or WHOLE)
        try:
            g.table_prepare(v, g.seed(c["pattern"], c["trans"]), lzo.upper_nuc_to_bits(), step=c["step"])
            run = H.search_strands(g, lambda strand: g.seed_hit_search_self(
                masked, q=v if strand == "+" else minus(v, seps), same_strand=(strand == "+"), band_width=c["band"], sep1=seps or None,
                sep2=seps or None, xdrop=c["xdrop"], hsp_threshold=c["hsp_threshold"], entropic=c["entropic"], extend=c["extend"]), c["strands"])
        finally:
            g.set_hit_capacity(WHOLE)
            g.set_scan_mode(0)
        yield dict(run, capacity=capacity)


def record_names(seps):
    return ["r%d" % k for k in range(len(seps) - 1)] if seps else ["s"]


def oracle_search(lzo, name, masked, table=None, self_filter=True, mode=None):
    """the oracle's statement of a case: ([HSP array per strand], counters summed over the strands).  self_filter=False:
    the same search without the self-comparison; mode: the oracle's processor (default: the case's)."""
    c = CASES[name]
    v, seps, _ = sequence(name)
    tab = table or lzo.Table(v, lzo.seed(c["pattern"], c["trans"]), step=c["step"])
    if mode is None:
        mode = 0 if c["extend"] else 1
    hs, tot = [], dict.fromkeys(COUNTERS, 0)
    for strand in c["strands"]:
        q = v if strand == "+" else minus(v, seps)
        kw = dict(self_strand="same" if strand == "+" else "opposite", band=c["band"], sep1=seps or None,
                  sep2=seps or None) if self_filter else {}
        h, st = lzo.seed_hit_search(tab, q, masked, xdrop=c["xdrop"], hsp_threshold=c["hsp_threshold"],
                                    entropic=c["entropic"], mode=mode, **kw)
        hs.append(h)
        for k in COUNTERS:
            tot[k] += st[k]
    return hs, tot
