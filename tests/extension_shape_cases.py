"""--exact, --mismatch and --filter under seeds and tables beyond those of tests/exact_cases.py, tests/mismatch_cases.py and
tests/filter_cases.py: one table of cases for four tiers -- the statement on the CPU (tests/test_extension_shapes.py), the goldens
from the pristine binary (tests/golden/make_extension_shapes_golden.py), the library on the GPU
(tests/test_gpu_extension_shapes.py) and the bound command line (tests/test_gpu_extension_shapes_cli.py).

What depends on the seed in these kernels is written around L <= 31 < 32: lz_exact_runs' `back >= seed_len` on a 32-base compare,
lz_mm_hit's window mask 0xFFFFFFFF << (32 - L), lz_filter_counts' one 32-pair compare from pos - L, filter_check's
`L < 32 && positions >> L`.  So: L = 31 (long31, parts6 with two transitions), L = 29 with 27 don't-care positions (ends29: the
window check decides nearly every hit), 28-bit tables (14of22, match14) and L = 4, 3, 2 (thresholds far above L).  What depends
on the table is which hits arrive and in what order: --step=3, a table on an interval of the target, a table under a word-count
limit (lzgpu_table_limit: the limited copy every search reads), a limit lifted again, and a table masked in place
(lzgpu_table_mask / lzgpu_target_update, which also invalidates the match codes both --mismatch and the filter read).

The statement.  Expected values are never the code under test's: the raw hits of a case are the ORACLE's, in discovery order,
from its own table (lzo.Table with the case's step / start / end, limited from outside by word_limit_cases.limited(), or built
from the masked bytes as table_mask_cases says); the filter's verdicts are filter_cases.by_bytes', the reference's routine
byte by byte; and the search over the hits it keeps is emul_exact_serial, emul_mismatch_serial or emul_filter_xdrop.  The
goldens pin all of it against the pristine binary wherever lastz's command line can say the case (everything but the interval
table and the masked one).

Sequences are the generators of exact_cases / mismatch_cases (SEQS) and table_mask_cases' target; nothing is committed for
them.  Pairs x seeds with more than about 2 M raw hits stay out (spaced x ends29: 73 M; long x 101: 19 M).  Every case names
`reach`: counters of the serial routine (exact_cases.COUNTERS, mismatch_cases.COUNTERS) and verdict counts of the filter
(filter_cases.REACH) that must not be zero on the plus strand, besides HSPs > 0.

(test infrastructure: data and helpers, no test in this file)"""
import numpy as np

from lastz_amd import seqio
import exact_cases as EC
import mismatch_cases as MC
import filter_cases as FC
import self_cases as S
import table_mask_cases as TM
import word_limit_cases as W

WHOLE = EC.WHOLE
GOLDEN_FORMAT = EC.GOLDEN_FORMAT
match_bits = EC.match_bits
EXACT_THR, MM, MM_THR = 30, 2, 40

# name: pattern, transitions, the seed on lastz's command line
SEEDS = {
    "12of19":  (EC.DEFAULT_SEED, 1, ["--seed=12of19"]),
    "long31":  ("1100100100100100100100100100111", 1, None),
    "parts6":  ("1010001010000100000011001000001", 2, None),
    "ends29":  ("1" + "0" * 27 + "1", 1, None),
    "14of22":  ("1110101100110010101111", 1, ["--seed=14of22"]),
    "match14": ("1" * 14, 0, ["--seed=match14", "--notransition"]),
    "1111":    ("1111", 1, None),
    "11":      ("11", 0, None),
    "101":     ("101", 1, None),
}
MULTI = {"bytes": (1500,)}                                  # pairs whose target has several records
EXTRA = {"bytes": ["--ambiguous=iupac"]}                    # (lastz reads an R only when told to)
BOTH = ("spaced",)                                          # pairs with something on the minus strand: the GPU tier searches both
MASKED = "two_events"                                       # table_mask_cases' case whose FIRST event the masking group applies


def _case(seed, seq, kind, reach, step=1, interval=None, limit=None, filt=None, capacity=None, thr=None, mask=False, lifted=False):
    """seed: a name of SEEDS; seq: a pair of mismatch_cases.SEQS (mask: table_mask_cases' target and a query cut from it);
    kind: exact, mismatch or xdrop; interval: the table's [start, end); limit: --maxwordcount=<limit>; filt: (T or None, M,
    cares) = --filter=[cares:][T,]M; capacity: a hit capacity that makes chunks; lifted: the GPU tier sets the limit `lifted`
    and lifts it again before it searches (the statement has no limit)"""
    pattern, trans, option = SEEDS[seed]
    return dict(seed=seed, pattern=pattern, trans=trans, seq=seq, kind=kind, reach=tuple(reach), step=step, interval=interval, limit=limit,
                filt=filt, capacity=capacity, mask=mask, lifted=lifted, multi=MULTI.get(seq), extra=EXTRA.get(seq, []),
                thr=thr or (EXACT_THR if kind == "exact" else MM_THR if kind == "mismatch" else None), mm=MM if kind == "mismatch" else None,
                option=option or ["--seed=" + pattern, ("--notransition", "--transition", "--transition=2")[trans]],
                strands=("+", "-") if seq in BOTH else ("+",),
                # what filter_cases' predicates read
                M=filt[1] if filt else 0, T=filt[0] if filt else None, cares=bool(filt and filt[2]))


CASES = {}


def _pair(name, seed, seq, exact=(), mismatch=(), **kw):
    """one shape as an --exact and a --mismatch search; exact / mismatch: what each must reach"""
    CASES[name + "_exact"] = _case(seed, seq, "exact", exact, **kw)
    CASES[name + "_mismatch"] = _case(seed, seq, "mismatch", mismatch, **kw)


def _filtered(name, seed, seq, filt, reach, **kw):
    """one filter as an X-drop, an --exact and a --mismatch search"""
    for kind in ("xdrop", "exact", "mismatch"):
        CASES["%s_%s" % (name, kind)] = _case(seed, seq, kind, reach, filt=filt, **kw)


# L = 31, one transition: `back` is 31 or 32, the window mask is shifted by 1, the filter's highest position is bit 30
_pair("long31_edges", "long31", "edges", ("not_matching", "dropped"), ("too_many", "seed_mm", "shortfall"))
_pair("long31_spaced", "long31", "spaced", ("not_matching", "dropped"), ("too_many", "seed_mm", "clipped", "shortfall", "dropped"))
_pair("long31_long", "long31", "long", ("dropped", "past_cap"), ("dropped", "past_cap", "past_step"))
_pair("long31_collide", "long31", "collide", ("clipped", "dropped", "other_diagonal"), ("dropped",))
_pair("long31_collide_mm", "long31", "collide_mm", ("dropped",), ("clipped", "other_diagonal", "dropped"))
_pair("long31_bytes", "long31", "bytes", ("not_matching", "dropped"), ("nul_left", "dropped"))
# L = 31, two transitions: 46 probes, most windows do not match
_pair("parts6_spaced", "parts6", "spaced", ("not_matching", "dropped"), ("too_many", "seed_mm", "dropped"))
_pair("parts6_bytes", "parts6", "bytes", ("not_matching", "dropped"), ("too_many", "nul_left", "dropped"))
# 27 don't-care positions between two cares: the window check decides
_pair("ends29_edges", "ends29", "edges", ("not_matching", "dropped"), ("too_many", "seed_mm", "dropped"))
_pair("ends29_bytes", "ends29", "bytes", ("not_matching", "dropped"), ("too_many", "seed_mm", "nul_left", "dropped"))
# 28-bit tables
_pair("s14of22_spaced", "14of22", "spaced", ("not_matching", "dropped"), ("seed_mm", "clipped", "shortfall", "dropped"))
_pair("s14of22_collide", "14of22", "collide", ("clipped", "dropped", "other_diagonal"), ("dropped",))
_pair("match14_spaced", "match14", "spaced", ("dropped",), ("clipped", "shortfall", "dropped"))
_pair("match14_collide", "match14", "collide", ("clipped", "dropped", "other_diagonal"), ("dropped",))
# L <= 4: L - 1 - back, thresholds far above L, chunks
_pair("s1111_edges", "1111", "edges", ("not_matching", "dropped"), ("seed_mm", "dropped"), capacity=2048)
_pair("s1111_bytes", "1111", "bytes", ("not_matching", "dropped"), ("seed_mm", "nul_left", "dropped"))
_pair("s11_edges", "11", "edges", ("dropped",), ("dropped",), capacity=1 << 17)
_pair("s11_bytes", "11", "bytes", ("dropped",), ("nul_left", "dropped"))
_pair("s101_edges", "101", "edges", ("not_matching", "dropped"), ("seed_mm", "dropped"), capacity=1 << 18)
_pair("s101_bytes", "101", "bytes", ("not_matching", "dropped"), ("seed_mm", "nul_left", "dropped"))
# --step=3
_pair("step3_12of19_spaced", "12of19", "spaced", ("not_matching", "dropped"), ("seed_mm", "clipped", "shortfall", "dropped"), step=3)
_pair("step3_long31_spaced", "long31", "spaced", ("not_matching", "dropped"), ("seed_mm", "clipped", "shortfall", "dropped"), step=3)
_pair("step3_long31_collide", "long31", "collide", ("clipped", "dropped", "other_diagonal"), ("dropped",), step=3)
_pair("step3_s1111_edges", "1111", "edges", ("not_matching", "dropped"), ("seed_mm", "dropped"), step=3)
_pair("step3_s14of22_spaced", "14of22", "spaced", ("not_matching", "dropped"), ("seed_mm", "clipped", "shortfall", "dropped"), step=3)
# a table on the middle third of spaced's target
_pair("interval_long31_spaced", "long31", "spaced", ("not_matching", "dropped"), ("seed_mm", "clipped", "shortfall", "dropped"), interval=(6667, 13334))
# a word-count limit (the limits are among word_limit_cases.limits_of() of the table's list lengths; test_extension_shapes.py
# asserts that, that a list goes and that an HSP stays)
_pair("limit_s1111_edges", "1111", "edges", ("not_matching", "dropped"), ("seed_mm", "dropped"), limit=17)
_pair("limit_s1111_bytes", "1111", "bytes", ("not_matching", "dropped"), ("seed_mm", "nul_left", "dropped"), limit=20)
_pair("limit_12of19_spaced", "12of19", "spaced", ("not_matching", "dropped"), ("seed_mm", "clipped", "shortfall", "dropped"), limit=1)
# ... and a limit set and lifted again: the case without a limit
_pair("lifted_s1111_edges", "1111", "edges", ("not_matching", "dropped"), ("seed_mm", "dropped"), lifted=17)
# the filter: bit 30 of positions, M close to L, cares of a spaced pattern, a two-care pattern, M = 3 of L = 4
ALL3 = ("few_matches", "many_transversions", "kept")
_filtered("f_2_25_long31", "long31", "spaced", (2, 25, False), ALL3)
_filtered("f_27_long31", "long31", "spaced", (None, 27, False), ("few_matches", "kept"))
_filtered("f_cares_1_12_long31", "long31", "spaced", (1, 12, True), ("kept",))         # (12 of its 13 cares: what one transition leaves -- every hit stays)
_filtered("f_cares_13_long31", "long31", "spaced", (None, 13, True), ("few_matches", "kept"))
_filtered("f_cares_2_ends29", "ends29", "edges", (None, 2, True), ("few_matches", "kept"))
# (--filter=1,3 keeps every hit of 1111 with one transition, and no hit of it has a transversion: 1,4 rejects the transitions)
_filtered("f_1_4_s1111", "1111", "edges", (1, 4, False), ("few_matches", "kept"))
CASES["f_2_25_long31_chunks_xdrop"] = _case("long31", "spaced", "xdrop", ALL3, filt=(2, 25, False), capacity=2048)
# every table form at once, as one command line says it: seed + --step + --maxwordcount + --filter + --exact
CASES["all_s1111_exact"] = _case("1111", "edges", "exact", ("few_matches", "kept", "dropped"), step=3, limit=4, filt=(1, 4, False))
# masking: one event on table_mask_cases' target, then --mismatch and a filtered X-drop search
CASES["masked_mismatch"] = _case("12of19", "masked", "mismatch", ("too_many", "clipped", "dropped"), mask=True)
CASES["masked_f_2_15_xdrop"] = _case("12of19", "masked", "xdrop", ALL3, filt=(2, 15, False), mask=True)

GOLDEN_CASES = [n for n, c in CASES.items() if not (c["interval"] or c["mask"] or c["lifted"])]
# cases that run the same command line as another one share its golden
GOLDEN_OF = {"f_2_25_long31_chunks_xdrop": "f_2_25_long31_xdrop"}


def golden_name(name):
    return GOLDEN_OF.get(name, name)


# ---------------------------------------------------------------------------------------- sequences

def _masked_pair():
    """table_mask_cases' target with the cores of the case's first event written over, and 3 kbp of the unmasked target around
    them with every 37th base changed: a query whose hits lie on both sides of and inside what the event took away"""
    t = TM.target(MASKED)
    q = t[6500:9500].copy()
    q[::37] = EC.ACGT[(np.searchsorted(EC.ACGT, q[::37]) + 1) % 4]
    return t, q


def unmasked_target():
    return TM.target(MASKED)


def mask_event(lzo):
    """(widened intervals, cores, the masked target) of the masking group's one event"""
    widened, cores = TM.events(lzo, MASKED)[0]
    return widened, cores, TM.masked_targets(lzo, MASKED)[0]


def records(name):
    """(target, query) as the FASTA files hold them"""
    c = CASES[name]
    assert not c["mask"]
    return EC._once(("seq", c["seq"]), MC.SEQS[c["seq"]])


def sequences(lzo, name):
    """(target bytes as the search sees them -- a masked case's after its event --, its separators or [], the query of the plus
    strand)"""
    c = CASES[name]
    if c["mask"]:
        _, q = EC._once(("xseq", "masked"), _masked_pair)
        return mask_event(lzo)[2], [], q
    t, q = records(name)
    v, seps = S.lay_out(t, c["multi"])
    return v, seps, q


def target_records(name):
    t, _ = records(name)
    m = CASES[name]["multi"]
    if m is None:
        return [("target", t)]
    cuts = np.cumsum([0] + list(m) + [len(t) - sum(m)])
    return [("t%d" % k, t[cuts[k]:cuts[k + 1]]) for k in range(len(cuts) - 1)]


def query_of(lzo, name, strand):
    q = sequences(lzo, name)[2]
    return q if strand == "+" else seqio.revcomp(q)


def filter_option(name):
    c = CASES[name]
    return "--filter=%s%s%d" % ("cares:" if c["cares"] else "", "" if c["T"] is None else "%d," % c["T"], c["M"])


def lastz_options(name):
    """the case on lastz's command line (after the two files): both strands, lastz's default"""
    c = CASES[name]
    assert name in GOLDEN_CASES
    ext = {"xdrop": [], "exact": ["--exact=%d" % (c["thr"] or 0)], "mismatch": ["--mismatch=%d,%d" % (c["mm"] or 0, c["thr"] or 0)]}[c["kind"]]
    return (ext + c["option"] + (["--step=%d" % c["step"]] if c["step"] != 1 else []) + (["--maxwordcount=%d" % c["limit"]] if c["limit"] else [])
            + ([filter_option(name)] if c["filt"] else []) + c["extra"])


# ---------------------------------------------------------------------------------------- the statement

def _shape(c):
    return (c["seq"], c["pattern"], c["trans"], c["step"], c["interval"], c["limit"])


def fresh_table(lzo, name, limit=True):
    """the case's oracle table, made anew (limited() works in place); limit False: before the limit"""
    c = CASES[name]
    s, e = c["interval"] or (0, 0)
    tab = lzo.Table(sequences(lzo, name)[0], lzo.seed(c["pattern"], c["trans"]), step=c["step"], start=s, end=e)
    if c["limit"] and limit:
        W.limited(tab, c["limit"])
    return tab


def table(lzo, name):
    return EC._once(("xtab",) + _shape(CASES[name]), lambda: fresh_table(lzo, name))


def raw_hits(lzo, name, strand="+"):
    """the raw seed hits of the case's table and one strand of its query, in discovery order, from the oracle: (pos1, pos2, its
    counters)"""
    def make():
        import helpers as H
        h, st = lzo.seed_hit_search(table(lzo, name), query_of(lzo, name, strand), H.scoring()[1], mode=1)
        return np.ascontiguousarray(h["pos1"]), np.ascontiguousarray(h["pos2"]), st
    return EC._once(("xraw", strand) + _shape(CASES[name]), make)


def verdicts(lzo, name, strand="+"):
    """the reference's verdict on every raw hit (0 kept, 1 few matches, 2 many transversions) and its (matches, transversions);
    without a filter every hit is kept"""
    c = CASES[name]

    def make():
        p1, p2, _ = raw_hits(lzo, name, strand)
        if not c["filt"]:
            return np.zeros(len(p1), dtype=np.uint8), None
        return FC.by_bytes(c, sequences(lzo, name)[0], query_of(lzo, name, strand), p1, p2)
    return EC._once(("xverdict", strand, c["filt"]) + _shape(c), make)


def statement(lzo, name, strand="+"):
    """the case's search as the reference runs it: dict(hsps in the reporter's order, raw, dropped, words, extensions,
    bp_extended, counters = the serial routine's branch counters ({} for an X-drop search))"""
    def make():
        import helpers as H
        c = CASES[name]
        v = sequences(lzo, name)[0]
        q = query_of(lzo, name, strand)
        p1, p2, st = raw_hits(lzo, name, strand)
        keep = verdicts(lzo, name, strand)[0] == 0
        L = len(c["pattern"])
        out = dict(raw=len(p1), dropped=int(len(p1) - keep.sum()), words=st["words"], extensions=0, bp_extended=0, counters={})
        if c["kind"] == "exact":
            hs, cn = EC.run_on(EC.emul().emul_exact_serial, v, q, p1[keep], p2[keep], L, c["thr"], len(EC.COUNTERS))
            out.update(hsps=hs, counters=dict(zip(EC.COUNTERS, (int(x) for x in cn))))
        elif c["kind"] == "mismatch":
            cn = np.zeros(len(MC.COUNTERS), dtype=np.uint64)
            hs, _ = MC.run_on(MC.emul().emul_mismatch_serial, v, q, p1[keep], p2[keep], L, c["mm"], c["thr"], cn)
            out.update(hsps=hs, counters=dict(zip(MC.COUNTERS, (int(x) for x in cn))))
        else:
            out.update(FC.search_over(c, v, q, p1, p2, keep, st["words"], lzo.upper_nuc_to_bits(), H.scoring()[1]))
        return out
    return EC._once(("xstatement", name, strand), make)


def decomposed(lzo, name, strand="+"):
    """the GPU's decomposition on the host (phase A per hit, phase B per bucket, from lz_exact.hpp / lz_mismatch.hpp) over the
    hits the filter keeps: the HSPs in discovery order"""
    c = CASES[name]
    v = sequences(lzo, name)[0]
    q = query_of(lzo, name, strand)
    p1, p2, _ = raw_hits(lzo, name, strand)
    keep = verdicts(lzo, name, strand)[0] == 0
    L = len(c["pattern"])
    if c["kind"] == "exact":
        return EC.run_on(EC.emul().emul_exact_decomposed, v, q, p1[keep], p2[keep], L, c["thr"], 1)[0]
    form = np.zeros(max(int(keep.sum()), 1), dtype=np.uint8)
    return MC.run_on(MC.emul().emul_mismatch_decomposed, v, q, p1[keep], p2[keep], L, c["mm"], c["thr"], form)[0]


def reach(lzo, name):
    """{counter: value} of the plus strand: the serial routine's branch counters, the filter's verdict counts and hsps"""
    e = statement(lzo, name)
    verdict = verdicts(lzo, name)[0]
    out = dict(e["counters"], hsps=len(e["hsps"]), raw=e["raw"])
    if CASES[name]["filt"]:
        out.update(few_matches=int((verdict == 1).sum()), many_transversions=int((verdict == 2).sum()), kept=int((verdict == 0).sum()))
    return out


def rows_of(lzo, name, strand, hsps):
    """HSPs of one strand -> the golden's rows (name1, start1, end1, name2, start2, end2, strand2, score), positions relative to
    the target record the HSP lies in, and in the query along the strand"""
    _, seps, _ = sequences(lzo, name)
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


def sweep(lzo, name, n=400, seed=7):
    """filter_cases.sweep for a case of this table: window ends at both ends of both sequences, at random, on the main diagonal
    and across every NUL of a [multi] target; (pos1, pos2)"""
    v, seps, q = sequences(lzo, name)
    return FC.sweep_over(v, seps, q, len(CASES[name]["pattern"]), n, seed)
