"""The oracle's statement of lastz --self / --band (oracle/lz_oracle_seed.c, lzo.seed_hit_search(self_strand=...)):
the raw hits the reference drops in find_table_matches (src/seed_search.c:841-848, 2052-2235), pinned

  (a) against the three recorded runs of the pristine binary that tests/test_gpu_self.py uses,
  (b) against an independent restatement: with the plain-hit processor, its hits are the non-self oracle's hits
      filtered by tests/test_self_bounds.py::kept, in order,
  (c) against the pristine binary on the cases of tests/self_cases.py that a command line can say -- recorded under
      tests/golden/self_<case>.* by tools/make_self_golden.py, and live where oracle/_ref/lastz was built,
  (d) and the cases themselves against what they are for: lists cut inside, bands that drop, enough HSPs.

tests/test_gpu_self_matrix.py then holds the kernels against this statement.  CPU only."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from oracle import lzo
import helpers as H
import self_cases as S
from test_gpu_self import as_rows, load, minus, REF_BIN
from test_self_bounds import kept

sys.path.insert(0, os.path.join(H.ROOT, "tools"))
MASKED = H.scoring()[1]
GOLDEN_CASES = [k for k, c in S.CASES.items() if c["cli"] is not None]
# the searches whose raw hits differ: scoring, chunking and scan modes change nothing before the processor
HIT_SETS = ["rep", "rep_b1", "rep_b61", "rep_b500", "rep_b40000", "repx", "seed_t0", "seed_t2", "seed_7", "seed_12s3",
            "plainhits", "multi_ragged", "multi_one"]
SAME_HITS = {"rep_chunks": "rep", "rep_b500_chunks": "rep_b500", "rep_m1": "rep", "rep_m2": "rep", "repx_m2": "repx",
             "scoring": "rep", "scoring_noent": "rep", "multi_chunks": "multi_ragged"}


def test_every_case_is_covered_by_a_hit_set():
    assert sorted(HIT_SETS + list(SAME_HITS)) == sorted(S.CASES)
    for k, base in SAME_HITS.items():
        a, b = S.CASES[k], S.CASES[base]
        for f in ("seq", "records", "band", "pattern", "trans", "step", "strands"):
            assert a[f] == b[f], (k, f)


# ---- (a) the recorded runs of tests/test_gpu_self.py
@pytest.mark.parametrize("name", ["plain", "multi", "band"])
def test_oracle_reproduces_the_recorded_runs(name):
    v, seps, names, want, stats = load(name)
    band = 2000 if name == "band" else 0
    tab = lzo.Table(v, lzo.seed())
    rows, tot = [], dict.fromkeys(S.COUNTERS, 0)
    for strand in ("+",) if name == "band" else ("+", "-"):
        q = v if strand == "+" else minus(v, seps)
        hs, st = lzo.seed_hit_search(tab, q, MASKED, self_strand="same" if strand == "+" else "opposite", band=band,
                                     sep1=seps or None, sep2=seps or None)
        rows += as_rows(hs, seps, names, strand)
        for k in S.COUNTERS:
            tot[k] += st[k]
    assert len(want) > 20 and rows == want                               # discovery order
    for k in S.COUNTERS:
        assert tot[k] == stats[k], k                                      # (raw_hits: counted after the drops, :865)


# ---- the searches, once per module
@pytest.fixture(scope="module")
def searches():
    """per case: (HSPs per strand, counters) as the case states it; per hit set also the plain hits with and without
    the self filter"""
    out = {"table": {}, "hsps": {}, "plain": {}}

    def table(name):
        c = S.CASES[name]
        key = (c["seq"], None if c["records"] is None else tuple(c["records"]), c["pattern"], c["trans"], c["step"])
        if key not in out["table"]:
            out["table"][key] = lzo.Table(S.sequence(name)[0], lzo.seed(c["pattern"], c["trans"]), step=c["step"])
        return out["table"][key]
    for name in S.CASES:
        out["hsps"][name] = S.oracle_search(lzo, name, MASKED, table=table(name))
    for name in HIT_SETS:
        out["plain"][name] = (S.oracle_search(lzo, name, MASKED, table=table(name), mode=1),
                              S.oracle_search(lzo, name, MASKED, table=table(name), mode=1, self_filter=False),
                              table(name))
    return out


# ---- (b) the independent restatement
def kept_many(p1, p2, same, L, len2, band, seps):
    """test_self_bounds.kept for arrays of hits (checked against it hit by hit in test_kept_many_is_kept)"""
    p1, p2 = p1.astype(np.int64), p2.astype(np.int64)
    if same:
        keep = p1 < p2
        if band > 0:
            keep &= (p2 - p1) <= band
        return keep
    a, b = p1 - L, p2 - L
    if not seps:
        return a < (len2 - 1) - b
    sp = np.array(seps, dtype=np.int64)
    i1, i2 = np.searchsorted(sp, a, side="left") - 1, np.searchsorted(sp, b, side="left") - 1
    assert (sp[i1] < a).all() and (a < sp[i1 + 1]).all() and (sp[i2] < b).all() and (b < sp[i2 + 1]).all()
    return np.where(i1 != i2, i1 < i2, a < (sp[i2] + sp[i2 + 1]) - b)


def strand_args(name, k):
    c = S.CASES[name]
    v, seps, _ = S.sequence(name)
    return (c["strands"][k] == "+", len(c["pattern"]), len(v), c["band"], seps)


def probe_points(keep, n_random=20_000):
    """hits on both sides of every place where consecutive hits' fates differ (at most 20,000 of them) + an even sample"""
    flips = np.flatnonzero(keep[1:] != keep[:-1])[:10_000]
    even = np.arange(0, len(keep), max(1, len(keep) // n_random))
    return np.unique(np.concatenate([flips, flips + 1, even]))


@pytest.mark.parametrize("name", HIT_SETS)
def test_kept_many_is_kept(searches, name):
    (_, _), (raw, _), _ = searches["plain"][name]
    for k, h in enumerate(raw):
        same, L, n, band, seps = strand_args(name, k)
        keep = kept_many(h["pos1"], h["pos2"], same, L, n, band, seps)
        at = probe_points(keep)
        want = [kept(int(h["pos1"][i]), int(h["pos2"][i]), same, L, n, band, seps, seps) for i in at]
        assert (keep[at] == np.array(want)).all()
        assert 0 < keep[at].sum() < len(at)


@pytest.mark.parametrize("name", HIT_SETS)
def test_self_hits_are_the_plain_hits_the_restatement_keeps(searches, name):
    (got, st), (raw, st_raw), _ = searches["plain"][name]
    n_kept = 0
    for k, h in enumerate(raw):
        keep = kept_many(h["pos1"], h["pos2"], *strand_args(name, k))
        assert len(got[k]) == int(keep.sum()) and (got[k] == h[keep]).all(), (name, k)
        n_kept += int(keep.sum())
    assert st["raw_hits"] == n_kept and st["words"] == st_raw["words"]


# ---- (c) the pristine binary, recorded and live
def rows_of(name, hs):
    _, seps, _ = S.sequence(name)
    names = S.record_names(seps)
    rows = []
    for strand, h in zip(S.CASES[name]["strands"], hs):
        rows += as_rows(h, seps, names, strand)
    return "".join("\t".join(r) + "\n" for r in rows).encode()


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_oracle_reproduces_the_recorded_cases(searches, name):
    from make_self_golden import stored_rows
    hs, tot = searches["hsps"][name]
    rows = rows_of(name, hs)
    stats = json.load(open(os.path.join(H.GOLDEN, "self_%s.stats.json" % name)))
    assert stored_rows(rows) == open(os.path.join(H.GOLDEN, "self_%s.hsp.tsv" % name), "rb").read()
    assert rows.count(b"\n") == stats["rows"] and hashlib.sha256(rows).hexdigest() == stats["rows_sha256"]
    for k in S.COUNTERS:
        assert tot[k] == stats[k], k


@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/lastz not built (needs the reference sources at build time)")
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_oracle_against_the_pristine_binary_live(searches, name):
    from make_self_golden import matrix_case, run_reference
    seq, records, extra = matrix_case(name)
    want, _ = run_reference(seq, records, extra, with_stats=False)
    assert rows_of(name, searches["hsps"][name][0]) == want


def test_recorded_fixtures_are_small():
    for name in GOLDEN_CASES:
        assert os.path.getsize(os.path.join(H.GOLDEN, "self_%s.hsp.tsv" % name)) <= 8 << 10


# ---- (d) the cases reach what they are for
@pytest.mark.parametrize("name", list(S.CASES))
def test_case_has_hits_and_hsps(searches, name):
    hs, tot = searches["hsps"][name]
    assert tot["raw_hits"] > 0
    if name == "plainhits":
        assert tot["extensions"] == 0 and sum(len(h) for h in hs) == tot["raw_hits"]
    elif name != "rep_b1":
        assert tot["hsps"] >= 10 and sum(len(h) for h in hs) == tot["hsps"]


@pytest.mark.parametrize("name", [k for k in HIT_SETS if k in S.CLIPPING])
def test_clipping_case_cuts_inside_lists(searches, name):
    """the plain hits of a strand are the table's lists one after the other, each from its head (Table.csr(): a word's
    positions, descending), once per probe of a query position that meets it.  On every strand some long list survives
    in part."""
    (_, st), (raw, st_raw), tab = searches["plain"][name]
    assert st["raw_hits"] < st_raw["raw_hits"]
    ws, wp = tab.csr()
    words = np.flatnonzero(ws[1:] > ws[:-1])
    list_len = np.zeros(int(wp.max()) + 1, dtype=np.int64)               # by head position; 0: not the head of a list
    list_len[wp[ws[words]]] = (ws[words + 1] - ws[words]).astype(np.int64)
    word_of = dict(zip(wp[ws[words]].tolist(), words.tolist()))
    for k, h in enumerate(raw):
        p1, p2 = h["pos1"].astype(np.int64), h["pos2"].astype(np.int64)
        args = strand_args(name, k)
        keep = kept_many(p1, p2, *args)
        first = np.flatnonzero(list_len[p1] > 0)
        size = np.diff(np.concatenate([first, [len(h)]]))
        assert first[0] == 0 and (size == list_len[p1[first]]).all()
        alive = np.add.reduceat(keep.astype(np.int64), first)
        part = np.flatnonzero((alive > 0) & (alive < size))
        assert len(part) > 0 and size[part].max() >= 30, (name, k)       # a long list, not a pair of entries
        for r in part[np.argsort(-size[part], kind="stable")[:5]]:
            w = word_of[int(p1[first[r]])]
            assert (wp[ws[w]:ws[w + 1]] == p1[first[r]:first[r] + size[r]]).all()
            inside = np.array([kept(int(a), int(p2[first[r]]), *args, args[4]) for a in wp[ws[w]:ws[w + 1]]])
            assert 0 < inside.sum() < len(inside)


@pytest.mark.parametrize("name", S.BANDED)
def test_band_keeps_some_and_drops_some(searches, name):
    band = S.CASES[name]["band"]
    plus_of_rep = searches["plain"]["rep"][0][0][0]                      # band 0, the same strand
    n = len(searches["plain"][SAME_HITS.get(name, name)][0][0][0])
    assert n > 0
    if band < len(S.sequence(name)[0]):
        assert n < len(plus_of_rep)
    else:
        assert n == len(plus_of_rep)
