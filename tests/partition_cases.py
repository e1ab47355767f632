"""The gapped stage on partitioned ("file[multi]") sequences: one table of cases for the three tiers -- the oracle against
the pristine binary (tests/test_partition_oracle.py), the device decomposition on the CPU (tests/test_emul_partitions.py)
and the library on the GPU (tests/test_gpu_partitions.py).

A case names its records (a list per sequence; one record and parted=False: no partitions), the arguments of the gapped
stage, the flags that say the same on lastz's command line (None: the command line cannot say it), the strands it runs and
what it is for.  `reaches(name)` states the latter as a condition on the ORACLE's results alone; test_partition_oracle.py
asserts it for every case, so that a case which no longer meets what it was built for fails on the CPU.

Layouts stay below 40 kbp a side.  A sequence is laid out as lastz holds it (self_cases.lay_out); the minus strand of a
partitioned query is every partition reverse-complemented in place (self_cases.minus); on that strand the sequences'
strand flags differ (strands_differ), as in lastz.

(test infrastructure: data and helpers, no test in this file)"""
import numpy as np

from oracle import lzo
from lastz_amd import seqio
import helpers as H
import scorings
from self_cases import lay_out, minus

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
GOLDEN_FORMAT = "--format=general-:name1,zstart1,end1,name2,strand2,zstart2,end2,score,cigar"

_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


# ---- the material the cases are cut from

def _pair():
    """a pair whose homologous blocks (0.9-2.5 kbp, 95 % of the query) are shorter than the pieces it is cut into"""
    return _once("pair", lambda: seqio.synth_pair(14000, 12000, seed=77, block_min=900, block_max=2500, homolog_frac=0.95))


def _cut_points():
    """three points (p1, p2) in the middle of the three longest plus-strand alignments of the uncut pair, each on a
    diagonal piece with 40 matched bases on either side: a cut there has homology running into it from both sides"""
    def make():
        t, q = _pair()
        sub, masked = H.scoring()
        hsps, _ = lzo.seed_hit_search(lzo.Table(t, lzo.seed()), q, masked)
        al, ops, _ = lzo.gapped_extend(t, q, sub, lzo.reduce_to_points(t, q, sub, lzo.hsps_to_segments(hsps, 0)))
        order = sorted(range(len(al)), key=lambda k: -(int(al[k]["end1"]) - int(al[k]["beg1"])))
        pts = []
        for k in order:
            a = al[k]
            mid = (int(a["beg1"]) + int(a["end1"])) // 2
            pieces = [p for p in H.align_segments(a, ops) if p[2] - p[0] >= 80]
            if pieces and int(a["end1"]) - int(a["beg1"]) > 900:
                b1, b2, e1, e2 = min(pieces, key=lambda p: abs((p[0] + p[2]) // 2 - mid))
                at = (b1 + e1) // 2
                if abs(at - mid) < 300 and all(abs(at - 1 - p1) > 700 and abs(b2 + at - b1 - 1 - p2) > 700 for p1, p2 in pts):
                    pts.append((at - 1, b2 + (at - b1) - 1))                 # zero-based
            if len(pts) == 3:
                break
        assert len(pts) == 3, pts
        return pts
    return _once("cuts", make)


def _cut(seq, points):
    """the records a sequence falls into when cut in front of each of `points`"""
    at = [0] + sorted(points) + [len(seq)]
    return [seq[at[k]:at[k + 1]] for k in range(len(at) - 1)]


def _flush():
    t, q = _pair()
    pts = _cut_points()
    return _cut(t, [p1 for p1, _ in pts]), _cut(q, [p2 for _, p2 in pts])


def _staggered():
    """the query's cuts 300 bases further on than the target's: an extension meets the target's cut in mid-partition of
    the query on one side of it, and the query's cut in mid-partition of the target on the other"""
    t, q = _pair()
    pts = _cut_points()
    return _cut(t, [p1 for p1, _ in pts]), _cut(q, [p2 + 300 for _, p2 in pts])


def _near_copy(rec):
    """the record with every 53rd base replaced (never the first or the last)"""
    r = rec.copy()
    at = np.arange(25, len(r) - 1, 53)
    r[at] = ACGT[(np.searchsorted(ACGT, r[at]) + 1) % 4]
    return r


def _ragged():
    """records of 1, 2 and 18 bases (shorter than the 19-base seed), two of a few thousand and a last record of three N;
    the query's records are near copies of the target's in another order, so that base k of a record meets base k"""
    t, _ = _pair()
    n3 = np.frombuffer(b"NNN", dtype=np.uint8)
    return ([t[0:1], t[1:3], t[3:21], t[21:5000], t[5000:9000], n3],
            [_near_copy(t[3:21]), _near_copy(t[21:5000]), t[0:1], t[1:3], _near_copy(t[5000:9000]), n3])


def _overlap():
    """synth_overlap's recipe cut down: 20 kbp of query blocks copied from a 7 kbp target, so that several alignments lie
    over the same target bases and bound each other, inside a partition pair and across partitions"""
    t, q = _once("overlap", lambda: seqio.synth_pair(7000, 20000, seed=5, block_min=1500, block_max=4000, homolog_frac=0.8))
    return [t[:3400], t[3400:]], [q[:6100], q[6100:13300], q[13300:]]


def _with_repeat():
    """a 4.2 kbp record with a 700-base stretch repeated 1.3 kbp further on: besides the main diagonal it aligns to itself
    off the diagonal twice"""
    def make():
        rng = np.random.default_rng(311)
        p = ACGT[rng.integers(0, 4, 4200)].copy()
        p[2300:3000] = p[1000:1700]
        p[2500] = ord("A") if p[2500] != ord("A") else ord("C")
        return p
    return _once("repeat", make)


def _fill(seed, n):
    return ACGT[np.random.default_rng(seed).integers(0, 4, n)]


def _soft_masked(p):
    m = p.copy()
    m[300:900] |= 0x20
    m[3500:3520] |= 0x20
    return m


def _palindrome():
    x = _fill(312, 1500)
    return np.concatenate([x, seqio.revcomp(x)])


def _three():
    return [_fill(321, 2500), _with_repeat(), _fill(323, 1800)]


def _diverged(rec, seed):
    """a copy with a substitution every 9 bases on average and a few bases taken out: aligns, but never as one piece"""
    rng = np.random.default_rng(seed)
    r = rec.copy()
    hit = np.flatnonzero(rng.random(len(r)) < 0.11)
    r[hit] = ACGT[(np.searchsorted(ACGT, r[hit]) + rng.integers(1, 4, len(hit))) % 4]
    return np.delete(r, [len(r) // 3, len(r) // 3 + 1, 2 * len(r) // 3])


# ---- the table

def _case(what, records, parted=(True, True), kw=None, flags=(), strands=("+", "-"), matrix=None, declined=False, points=None):
    return dict(what=what, records=records, parted=parted, kw=kw or {}, flags=None if flags is None else list(flags),
                strands=strands, matrix=matrix, declined=declined, points=points)


def _ragged_points(lay):
    """hand-made point anchors on the first and on the last base of partitions of both sequences (the one-sided DP on
    that side has M or N of 1 and of 0), one in an 18-base record against a long one, and one in mid-partition"""
    (v1, s1), (v2, s2) = lay
    pts = [(s1[3] + 1, s2[1] + 1, 5000),                 # first base of a long record in both: M == N == 1 to the left
           (s1[5] - 1, s2[5] - 1, 4900),                 # last base of another long record in both: M == N == 0 to the right
           (s1[4] + 1, s2[2] - 1, 4800),                 # first base in the target, last in the query
           (s1[2] + 1, s2[0] + 1, 4700),                 # first base of the 18-base record in both
           (s1[3] - 1, s2[4] + 18, 4650),                # last base of the 18-base record, in mid-partition of the query
           (s1[0] + 1, s2[2] + 1, 4600),                 # the 1-base record against its copy
           (s1[1] + 2, s2[3] + 2, 4500),                 # last base of the 2-base record in both
           (s1[4] + 2000, s2[1] + 2000, 4400),           # mid-partition, records that are not copies
           (s1[5] + 1, s2[5] + 2, 4300)]                 # inside the N records
    segs = np.zeros(len(pts), dtype=lzo.SEG_DTYPE)
    for k, (p1, p2, s) in enumerate(pts):
        segs[k] = (p1, p2, 0, s, 0)
    return segs


CASES = {
    # group 1: cuts
    "flush":            _case("cuts at corresponding points of t and q, default trimming: only the limits end an extension", _flush),
    "flush_notrim":     _case("the same under --noytrim: the end is taken on the partition's last row and column", _flush,
                              kw=dict(no_trim=True), flags=["--noytrim"]),
    "stagger":          _case("cuts 300 bases apart in t and q, default trimming", _staggered),
    "stagger_notrim":   _case("the same under --noytrim: row == M in mid-partition of the query, col == N the other way round", _staggered,
                              kw=dict(no_trim=True), flags=["--noytrim"]),
    # group 2: layouts
    "q_only":           _case("only seq2 partitioned", lambda: ([_pair()[0]], _flush()[1]), parted=(False, True)),
    "q_only_notrivial": _case("only seq2 partitioned, inhibit_trivial: the delayed check is on and finds nothing",
                              lambda: ([_pair()[0]], _flush()[1]), parted=(False, True), kw=dict(inhibit_trivial=True), flags=["--notrivial"]),
    "t_only":           _case("only seq1 partitioned", lambda: (_flush()[0], [_pair()[1]]), parted=(True, False)),
    "ragged":           _case("records of 1, 2 and 18 bases, long ones and a last record of N", _ragged),
    "ragged_points":    _case("hand-made point anchors on the first and last base of partitions: one-sided DPs of 1 and 0 rows and columns",
                              _ragged, flags=None, strands=("+",), points=_ragged_points, kw=dict(score_thresh=0, no_trim=True)),
    # group 3: bounds, bands, scoring
    "bounds":           _case("overlapping alignments bound each other inside a partition pair and across partitions", _overlap),
    "flush_bounds_notrim": _case("--allgappedbounds with --noytrim on the flush cuts", _flush,
                                 kw=dict(no_trim=True, all_bounds=True, score_thresh=40000), flags=["--noytrim", "--allgappedbounds", "--gappedthresh=40000"]),
    "wide":             _case("bands wider than the LDS ring (gap 200 / 5) on a partitioned pair", _staggered,
                              kw=dict(gap_open=200, gap_extend=5), flags=["--gap=200,5", "--ydrop=9400"]),
    "eight":            _case("a matrix that is not symmetric on the staggered cuts", _staggered, matrix="eight", flags=["--scores={scores}"]),
    # group 4: trivial alignments
    "triv_first":       _case("seq2 equals two partitions of seq1: the first wins; its repeat aligns off the diagonal, bounded by the trivial alignment",
                              lambda: ([_fill(331, 1500), _with_repeat(), _fill(332, 900), _with_repeat()], [_with_repeat()]), parted=(True, False)),
    "triv_masked":      _case("seq2 equals a soft-masked partition of seq1: the comparison folds case",
                              lambda: ([_fill(331, 1500), _soft_masked(_with_repeat()), _fill(332, 900)], [_with_repeat()]), parted=(True, False)),
    "triv_strands":     _case("seq2 is its own reverse complement: on the minus strand the same bytes get no trivial alignment",
                              lambda: ([_fill(331, 1500), _palindrome(), _fill(332, 900)], [_palindrome()]), parted=(True, False)),
    "triv_notrivial":   _case("inhibit_trivial: the trivial alignment is dropped from the output and still bounds the others",
                              lambda: ([_fill(331, 1500), _with_repeat(), _fill(332, 900), _with_repeat()], [_with_repeat()]), parted=(True, False),
                              kw=dict(inhibit_trivial=True), flags=["--notrivial"]),
    "both_ident":       _case("both partitioned, every pair (k, k) identical up to case: one trivial alignment per pair",
                              lambda: (_three(), [_three()[0], _soft_masked(_three()[1]), _three()[2]])),
    "both_ident_notrivial": _case("the same with inhibit_trivial", lambda: (_three(), [_three()[0], _soft_masked(_three()[1]), _three()[2]]),
                                  kw=dict(inhibit_trivial=True), flags=["--notrivial"]),
    "reorder":          _case("the same records in another order: no trivial alignments, an ordinary run",
                              lambda: (_three(), [_three()[1], _three()[0], _three()[2]])),
    "reorder_notrivial": _case("... with inhibit_trivial: whole-partition diagonal alignments exist, the reference decides by name: declined",
                               lambda: (_three(), [_three()[1], _three()[0], _three()[2]]), kw=dict(inhibit_trivial=True), flags=None, declined=True),
    "diverged_notrivial": _case("reordered records too diverged to align whole, inhibit_trivial: the delayed check finds nothing",
                                lambda: (_three(), [_diverged(_three()[1], 341), _diverged(_three()[0], 342), _diverged(_three()[2], 343)]),
                                kw=dict(inhibit_trivial=True), flags=["--notrivial"]),
}
GOLDEN = [k for k, c in CASES.items() if c["flags"] is not None]
NO_TRIM = [k for k, c in CASES.items() if c["kw"].get("no_trim")]
TRIVIAL = [k for k in CASES if k.startswith(("triv", "both"))]


# ---- what a case runs on

def records(name):
    return _once(("records", name), CASES[name]["records"])


def names(name):
    """the records' names in the FASTA files, per sequence"""
    r1, r2 = records(name)
    return ["t%d" % k for k in range(len(r1))], ["q%d" % k for k in range(len(r2))]


def layout(name):
    """-> ((bytes of seq1, its separators or []), (bytes of seq2, its separators or []))"""
    def make():
        out = []
        for recs, parted in zip(records(name), CASES[name]["parted"]):
            if not parted:
                assert len(recs) == 1
                out.append((recs[0], []))
            else:
                out.append(lay_out(np.concatenate(recs), [len(r) for r in recs[:-1]]))
        return tuple(out)
    return _once(("layout", name), make)


def scoring(name):
    m = CASES[name]["matrix"]
    return H.scoring() if m is None else scorings.m4_scoring(scorings.MATRICES[m])


def problems(name):
    """one problem per strand of the case: dict(strand, rev, t, sep1, q, sep2, segs, reduce, kw) -- segs are the oracle's HSPs
    of the strand as segments (or the case's hand-made points), kw the arguments of the gapped stage in the library's names"""
    def make():
        c = CASES[name]
        (v1, s1), (v2, s2) = layout(name)
        sub, masked = scoring(name)
        tab = lzo.Table(v1, lzo.seed())
        out = []
        for strand in c["strands"]:
            rev = int(strand == "-")
            qq = v2 if not rev else minus(v2, s2)
            if c["points"] is not None:
                segs, reduce = c["points"](layout(name)), False
            else:
                hsps, _ = lzo.seed_hit_search(tab, qq, masked)
                segs, reduce = lzo.hsps_to_segments(hsps, rev), True
            kw = dict(c["kw"])
            kw["strands_differ"] = bool(rev) or kw.get("strands_differ", False)
            out.append(dict(strand=strand, rev=rev, t=v1, sep1=s1 or None, q=qq, sep2=s2 or None, segs=segs, reduce=reduce, kw=kw))
        return out
    return _once(("problems", name), make)


def oracle_kw(kw):
    """the library's names of the gapped arguments -> lzo.gapped_extend's"""
    kw = dict(kw)
    kw["trim_to_peak"] = not kw.pop("no_trim", False)
    return kw


def oracle_problem(pr, sub, **override):
    """the oracle's answer to one problem -> (alignments, ops, stats)"""
    anchors = lzo.reduce_to_points(pr["t"], pr["q"], sub, pr["segs"]) if pr["reduce"] else pr["segs"]
    kw = oracle_kw(pr["kw"])
    kw.update(sep1=pr["sep1"], sep2=pr["sep2"])
    kw.update(override)
    return lzo.gapped_extend(pr["t"], pr["q"], sub, anchors, **kw)


def oracle(name):
    """the shared reference of a case, computed once: [(alignments, ops, stats)] per strand"""
    return _once(("oracle", name), lambda: [oracle_problem(pr, scoring(name)[0]) for pr in problems(name)])


def same(a, b):
    """two (alignments, ops[, ...]) results are equal: rows, order and edit scripts"""
    return len(a[0]) == len(b[0]) and bool((a[0] == b[0]).all()) and len(a[1]) == len(b[1]) and bool((np.asarray(a[1]) == np.asarray(b[1])).all())


# ---- the results as the binary prints them

def _part_of(seps, pos):
    for k in range(len(seps) - 1):
        if seps[k] < pos < seps[k + 1]:
            return k
    raise AssertionError("position %d lies in no partition" % pos)


def rows_of(name, strand, al, ops):
    """alignments of one strand -> the rows of GOLDEN_FORMAT: partition names, zero-based partition-relative starts and
    ends (the query's along the strand aligned), score, and the edit script as a CIGAR string"""
    (_, s1), (_, s2) = layout(name)
    n1, n2 = names(name)
    rows = []
    for a in al:
        b1, b2, e1, e2 = int(a["beg1"]) - 1, int(a["beg2"]) - 1, int(a["end1"]), int(a["end2"])
        k1 = _part_of(s1, b1) if s1 else 0
        k2 = _part_of(s2, b2) if s2 else 0
        o1 = s1[k1] + 1 if s1 else 0
        o2 = s2[k2] + 1 if s2 else 0
        assert not s1 or e1 <= s1[k1 + 1]
        assert not s2 or e2 <= s2[k2 + 1]
        cigar = "".join("%d%s" % (int(w) >> 2, " IDM"[int(w) & 3]) for w in ops[int(a["script_off"]):int(a["script_off"]) + int(a["script_len"])])
        rows.append((n1[k1], b1 - o1, e1 - o1, n2[k2], strand, b2 - o2, e2 - o2, int(a["s"]), cigar))
    return rows


def parse_rows(text):
    out = []
    for line in text.split("\n"):
        f = line.split("\t")
        if len(f) == 9:
            out.append((f[0], int(f[1]), int(f[2]), f[3], f[4], int(f[5]), int(f[6]), int(f[7]), f[8]))
    return out


def oracle_rows(name):
    """the whole case as the binary prints it (strand after strand), and the DP cells of all strands"""
    rows, cells = [], 0
    for pr, (al, ops, st) in zip(problems(name), oracle(name)):
        rows += rows_of(name, pr["strand"], al, ops)
        cells += st["dp_cells"]
    return rows, cells


# ---- what each case is for, as a condition on the oracle's results

def _is_whole_diagonal(a, lo1, hi1, lo2, hi2):
    return (int(a["beg1"]) - 1, int(a["end1"]), int(a["beg2"]) - 1, int(a["end2"])) == (lo1, hi1, lo2, hi2) and int(a["script_len"]) == 1


def reaches(name):
    """None if the case meets what it was built for, else what is missing"""
    c = CASES[name]
    sub = scoring(name)[0]
    prs, res = problems(name), oracle(name)
    (v1, s1), (v2, s2) = layout(name)
    n_al = sum(len(r[0]) for r in res)
    if n_al == 0 and not c["declined"]:
        return "no alignments at all"
    parted = [pr for pr in prs if pr["sep1"] or pr["sep2"]]
    # the limits decide something: without the separators the same bytes give another result or visit other cells
    if name not in TRIVIAL and c["points"] is None and not name.startswith(("reorder", "diverged")):
        changed = cells = False
        for pr, r in zip(prs, res):
            r0 = oracle_problem(pr, sub, sep1=None, sep2=None)
            changed = changed or not same(r, r0)
            cells = cells or r[2]["dp_cells"] != r0[2]["dp_cells"]
        if c["kw"].get("no_trim") and not changed:
            return "with --noytrim the limits must change the alignments"
        if not (changed or cells):
            return "the limits change neither the alignments nor the cells visited"
    if c["kw"].get("no_trim") and c["points"] is None:
        trimmed = [oracle_problem(pr, sub, trim_to_peak=True) for pr in prs]
        if all(same(a, b) for a, b in zip(res, trimmed)):
            return "--noytrim changes nothing"
    if name.startswith("stagger") or name in ("wide", "eight"):
        # an alignment ends on a cut of one sequence in mid-partition of the other, on either side
        ends_t = ends_q = False
        for pr, (al, _, _) in zip(prs, res):
            for a in al:
                k1, k2 = _part_of(s1, int(a["beg1"])), _part_of(s2, int(a["beg2"]))
                at_t = int(a["end1"]) == s1[k1 + 1] - 1 or int(a["beg1"]) == s1[k1] + 2
                at_q = int(a["end2"]) == s2[k2 + 1] - 1 or int(a["beg2"]) == s2[k2] + 2
                ends_t = ends_t or (at_t and not at_q)
                ends_q = ends_q or (at_q and not at_t)
        if name == "stagger_notrim" and not (ends_t and ends_q):
            return "no alignment ends on a cut of one sequence alone (t: %s, q: %s)" % (ends_t, ends_q)
    if name == "wide" and max(r[2]["max_cols"] for r in res) <= 2048:
        return "no band wider than 2048 columns"
    if name == "eight":
        hox = [oracle_problem(pr, H.scoring()[0]) for pr in prs]
        if all(same(a, b) for a, b in zip(res, hox)):
            return "the matrix changes nothing"
    if name == "bounds":
        if res[0][2]["anchors_extended"] + res[1][2]["anchors_extended"] < 8:
            return "fewer than 8 anchors extended"
        overl = 0
        for al, _, _ in res:
            for i in range(len(al)):
                for j in range(i + 1, len(al)):
                    if al[i]["beg1"] <= al[j]["end1"] and al[j]["beg1"] <= al[i]["end1"]:
                        overl += 1
        if overl < 3:
            return "alignments do not overlap in the target"
    if name == "flush_bounds_notrim":
        plain = [oracle_problem(pr, sub, all_bounds=False) for pr in prs]
        if all(same(a, b) and a[2]["dp_cells"] == b[2]["dp_cells"] for a, b in zip(res, plain)):
            return "--allgappedbounds changes nothing"
    if name == "ragged_points":
        al = res[0][0]
        ones = [a for a in al if int(a["end1"]) == int(a["beg1"])]
        if len(al) < 5 or not ones:
            return "the point anchors on the edges gave %d alignments, %d of one base" % (len(al), len(ones))
    if name.endswith("_notrivial") and not c["declined"] and name not in ("triv_notrivial", "both_ident_notrivial"):
        if any(r[2]["trivial_candidate"] for r in res):
            return "the delayed check finds a candidate"
        if not any(int(a["script_len"]) >= 1 for r in res for a in r[0]):
            return "nothing to check"
    if c["declined"]:
        if not any(r[2]["trivial_candidate"] for r in res):
            return "no whole-partition diagonal alignment: nothing to decline"
        free = [oracle_problem(pr, sub, inhibit_trivial=False) for pr in prs]
        if any(r[2]["trivial_candidate"] for r in free):
            return "a candidate without inhibit_trivial"
    if name in TRIVIAL:
        pr, (al, ops, st) = prs[0], res[0]                     # the plus strand
        inhibit = c["kw"].get("inhibit_trivial", False)
        if name.startswith("triv"):
            k = 1
            want = [(s1[k] + 1, s1[k + 1], 0, len(v2))]
        else:
            want = [(s1[k] + 1, s1[k + 1], s2[k] + 1, s2[k + 1]) for k in range(len(s1) - 1)]
        have = [w for w in want if any(_is_whole_diagonal(a, *w) for a in al)]
        if inhibit and have:
            return "a trivial alignment in the output under inhibit_trivial"
        if not inhibit and len(have) != len(want):
            return "trivial alignments missing: %d of %d" % (len(have), len(want))
        no_triv = oracle_problem(pr, sub, strands_differ=True, inhibit_trivial=False)
        if no_triv[2]["dp_cells"] == st["dp_cells"]:
            return "the trivial alignments bound nothing: same cells without them"
        if inhibit:
            kept = oracle_problem(pr, sub, inhibit_trivial=False)
            rows = [tuple(a)[:5] for a in kept[0] if not any(_is_whole_diagonal(a, *w) for w in want)]
            if rows != [tuple(a)[:5] for a in al] or kept[2]["dp_cells"] != st["dp_cells"] or not rows:
                return "under inhibit_trivial the others must be what they are beside the trivial alignment"
        if name in ("triv_first", "triv_notrivial"):
            lo, hi = s1[1] + 1, s1[2]
            off = [a for a in al if lo <= int(a["beg1"]) - 1 < hi and not _is_whole_diagonal(a, lo, hi, 0, len(v2))]
            if not off:
                return "no alignment off the diagonal inside the identical partition"
            if not any(_is_whole_diagonal(a, s1[3] + 1, s1[4], 0, len(v2)) for a in al):
                return "the second identical partition has no alignment of its own"
        if name == "triv_masked" and not ((v1[s1[1] + 1:s1[2]] != v2).any()):
            return "the partition is not soft-masked"
        if name == "triv_strands":
            if len(prs) != 2 or not (prs[1]["q"] == prs[0]["q"]).all():
                return "the minus strand's bytes differ from the plus strand's"
            if res[1][2]["dp_cells"] == st["dp_cells"]:
                return "the minus strand visits the same cells: a trivial alignment there too?"
    return None
