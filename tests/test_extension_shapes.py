"""--exact, --mismatch and --filter under other seeds and tables, on the CPU: the cases of tests/extension_shape_cases.py.

The raw hits in discovery order are the oracle's, from its own table (stepped, on an interval, limited from outside, or built from
the masked bytes); the verdicts are the byte-wise transcription of the reference's filter routine; the searches are the serial
routines of tests/emul/emul_exact.cpp, emul_mismatch.cpp and emul_filter.cpp.

  * every case reaches what it names (extension_shape_cases: `reach`) and has an HSP; the limited cases' limits are among
    word_limit_cases.limits_of(), take a list away and leave hits; the lifted case is the case without a limit;
  * the GPU's decomposition on the host -- phase A per hit, phase B per bucket, compiled from lz_exact.hpp / lz_mismatch.hpp --
    equals the serial routine at L = 31, 29, 22, 14, 4, 3 and 2: rows and order;
  * lz_filter.hpp's predicate on match codes equals the byte-wise one, verdicts and both counts, on every raw hit of every
    filtered case and on a sweep of windows at L = 31, 29, 4, 3 and 2 (both ends of both sequences, across the NULs);
  * the statement's rows, both strands, sorted, are what the pristine binary printed (tests/golden/extshape_<case>.tsv, recorded
    by tests/golden/make_extension_shapes_golden.py with the command lines of extension_shapes_index.json; run again where
    oracle/_ref/lastz is present).
CPU only."""
import sys

import numpy as np
import pytest

from oracle import lzo
import helpers as H
import extension_shape_cases as X
import filter_cases as FC
import word_limit_cases as W

sys.path.insert(0, H.GOLDEN)
import make_extension_shapes_golden as M            # noqa: E402

EXTENDED = [n for n, c in X.CASES.items() if c["kind"] != "xdrop"]
FILTERED = [n for n, c in X.CASES.items() if c["filt"] and c["kind"] == "xdrop"]      # (one search kind per filter: the hits are the same)
# the sweep: one filter per window length, whole-window and cares; (pattern, trans, pair, T, M, cares)
SWEPT = {"L31": ("long31", "spaced", 2, 25, False), "L31_cares": ("long31", "bytes", 1, 12, True), "L29_cares": ("ends29", "bytes", None, 2, True),
         "L29": ("ends29", "spaced", 3, 20, False), "L4": ("1111", "bytes", 1, 3, False), "L3": ("101", "bytes", 0, 2, False),
         "L3_cares": ("101", "spaced", None, 2, True), "L2": ("11", "bytes", 0, 1, False)}


@pytest.mark.parametrize("name", list(X.CASES))
def test_case_reaches_what_it_is_for(name):
    r = X.reach(lzo, name)
    print("\n%s: %s" % (name, {k: v for k, v in r.items() if v}))
    for x in X.CASES[name]["reach"]:
        assert r[x] > 0, (name, x, r)
    assert r["hsps"] > 0 and r["raw"] > 0, (name, r)
    assert r["raw"] <= 2_000_000                                            # (what the GPU tier can run in a few seconds)
    if X.CASES[name]["capacity"]:
        assert r["raw"] > 2 * X.CASES[name]["capacity"]                     # at least three chunks


@pytest.mark.parametrize("name", [n for n, c in X.CASES.items() if c["limit"]])
def test_limits_take_a_list_away_and_leave_hits(name):
    c = X.CASES[name]
    n = W.list_lengths(X.fresh_table(lzo, name, limit=False))
    assert c["limit"] in W.limits_of(n) and int(n.max()) > c["limit"], (name, W.limits_of(n))
    kept = W.list_lengths(X.table(lzo, name))
    assert 0 < kept.sum() < n.sum() and int(kept.max()) <= c["limit"]
    assert len(X.statement(lzo, name)["hsps"]) > 0


def test_lifted_cases_are_the_cases_without_a_limit():
    for name in (n for n, c in X.CASES.items() if c["lifted"]):
        twin = name.replace("lifted_", "")
        a, b = X.statement(lzo, name), X.statement(lzo, twin)
        assert a["raw"] == b["raw"] and (a["hsps"] == b["hsps"]).all()


@pytest.mark.parametrize("name", EXTENDED)
def test_decomposition_is_the_serial_routine(name):
    for strand in X.CASES[name]["strands"]:
        want = X.statement(lzo, name, strand)["hsps"]
        got = X.decomposed(lzo, name, strand)
        assert len(got) == len(want) and (got == want).all(), (name, strand, len(got), len(want))
    assert len(X.statement(lzo, name)["hsps"]) > 0


def _agree(c, t, q, p1, p2):
    verdict, cb = FC.by_bytes(c, t, q, p1, p2)
    keeps, cc = FC.by_codes(c, t, q, p1, p2)
    assert ((verdict == 0) == (keeps == 1)).all()
    assert (cb == cc).all()
    return verdict, cb


@pytest.mark.parametrize("name", FILTERED)
def test_predicates_agree_on_every_raw_hit(name):
    for strand in X.CASES[name]["strands"]:
        p1, p2, _ = X.raw_hits(lzo, name, strand)
        assert len(p1) > 0
        verdict, _ = _agree(X.CASES[name], X.sequences(lzo, name)[0], X.query_of(lzo, name, strand), p1, p2)
        assert (verdict == X.verdicts(lzo, name, strand)[0]).all()


@pytest.mark.parametrize("what", list(SWEPT))
def test_predicates_agree_on_the_sweep(what):
    seed, seq, T, M_, cares = SWEPT[what]
    c = X._case(seed, seq, "xdrop", (), filt=(T, M_, cares))
    t, q = X.EC._once(("seq", seq), X.MC.SEQS[seq])
    v, seps = X.S.lay_out(t, c["multi"])
    L = len(c["pattern"])
    p1, p2 = FC.sweep_over(v, seps, q, L)
    verdict, counts = _agree(c, v, q, p1, p2)
    assert (p1 == L).any() and (p1 == len(v)).any() and (p2 == L).any() and (p2 == len(q)).any()
    assert (verdict != 0).any(), what
    if seq == "spaced" or L <= 4:                                           # (homologous along the main diagonal, or a window chance fills)
        assert (verdict == 0).any(), what
    n_pos = bin(FC.positions(c)).count("1")
    assert int(counts[:, 0].max()) <= n_pos and len(np.unique(counts[:, 0])) >= min(n_pos, 3), what
    if seps:                                                                # windows across a NUL: it counts as a transversion
        over = np.array([any(a - L <= s < a and (FC.positions(c) >> (s - (a - L))) & 1 for s in seps) for a in p1])
        assert over.sum() > 4 and (counts[over, 1] >= 1).all(), what


@pytest.mark.parametrize("name", X.GOLDEN_CASES)
def test_statement_rows_are_the_goldens(name):
    gold = X.parse_rows(M.golden(name))
    assert len(gold) > 0
    assert M.index()[X.golden_name(name)] == M.options(X.golden_name(name)) == M.options(name)      # the command line the golden was recorded with
    if X.CASES[name]["seq"] == "spaced" and X.CASES[name]["kind"] != "xdrop":       # (3 kbp of its query are of the other strand)
        assert {r[6] for r in gold} == {"+", "-"}
    rows = []
    for strand in ("+", "-"):
        rows += X.rows_of(lzo, name, strand, X.statement(lzo, name, strand)["hsps"])
    assert sorted(rows) == sorted(gold)


def test_every_expressible_case_has_a_golden():
    for name, c in X.CASES.items():
        assert (name in X.GOLDEN_CASES) == (not (c["interval"] or c["mask"] or c["lifted"])), name
    assert sorted(M.index()) == sorted(M.names())
    line = M.options("all_s1111_exact")                                     # seed + --step + --maxwordcount + --filter + --exact on one line
    assert all(any(o.startswith(p) for o in line) for p in ("--seed=", "--step=", "--maxwordcount=", "--filter=", "--exact="))


@pytest.mark.parametrize("name", M.names())
def test_live_reference_run(tmp_path, name):
    if lzo.ref_binary() is None:
        pytest.skip("oracle/_ref/lastz is not built here (the goldens above always run)")
    assert M.run(name, tmp_path) == M.golden(name)
