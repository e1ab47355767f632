"""The seed-hit filter (lastz --filter) on the CPU, over the cases of tests/filter_cases.py.

tests/emul/emul_filter.cpp holds filter_seed_hit_by_subs transcribed byte by byte, the predicate the kernels compile
(lastz_amd/csrc/lz_filter.hpp) on match codes laid out as the library lays them out, and a serial X-drop pass over a hit list.
The raw hits in discovery order are the oracle's.

  * the two predicates agree, verdict and both counts, on every raw hit of every case and on a sweep of windows at both ends of
    both sequences (pos = L, pos = len), at random and across the NULs of a [multi] target;
  * every case reaches what it is for (filter_cases.REACH); empty_chunks' first three chunks' worth of raw hits are all rejected;
  * cares_12 -- the filter asks for a match at each of the seed's 12 care positions -- is the oracle's --notransition search of
    the same pair, and noop the oracle's unfiltered search: rows, order and counters.  Neither pin involves the new code;
  * the sorted rows of every golden case, both strands, are what the pristine binary printed with --filter on its command line
    (tests/golden/filter_<case>.tsv, recorded by tests/golden/make_filter_golden.py; run again where oracle/_ref/lastz is present);
  * the match-code predicate under the address and undefined-behaviour sanitizers, in a program of its own
    (tests/emul/emul_filter_main.cpp), over the sweep: its 9-byte loads stay inside the arrays' padding.
CPU only."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import lzo
import helpers as H
import filter_cases as FC

sys.path.insert(0, H.GOLDEN)
import make_filter_golden as M                      # noqa: E402

SWEPT = ["whole_2_15", "cares_12", "bytes", "empty_chunks"]


def _agree(name, t, q, p1, p2):
    verdict, cb = FC.by_bytes(name, t, q, p1, p2)
    keeps, cc = FC.by_codes(name, t, q, p1, p2)
    assert ((verdict == 0) == (keeps == 1)).all(), name
    assert (cb == cc).all(), name
    return verdict, cb


@pytest.mark.parametrize("name", list(FC.CASES))
def test_predicates_agree_on_every_raw_hit(name):
    for strand in FC.CASES[name]["strands"]:
        p1, p2, _ = FC.raw_hits(lzo, name, strand)
        assert len(p1) > 0
        _agree(name, FC.sequences(name)[0], FC.query_of(name, strand), p1, p2)


@pytest.mark.parametrize("name", SWEPT)
def test_predicates_agree_on_the_sweep(name):
    v, seps, q = FC.sequences(name)
    L = len(FC.CASES[name]["pattern"])
    p1, p2 = FC.sweep(name)
    verdict, counts = _agree(name, v, q, p1, p2)
    assert (p1 == L).any() and (p1 == len(v)).any() and (p2 == L).any() and (p2 == len(q)).any()
    assert len(np.unique(counts[:, 0])) > 4 and len(np.unique(counts[:, 1])) > 4
    if FC.CASES[name]["seq"] == "spaced":                                   # (homologous along the main diagonal)
        assert (verdict == 0).any() and (verdict == 1).any() and (verdict == 2).any() == (FC.CASES[name]["T"] is not None)
    if seps:                                                                # windows across a NUL: it counts as a transversion
        over = np.array([any(a - L <= s < a for s in seps) for a in p1])
        assert over.sum() > 20 and (counts[over, 1] >= 1).all()


@pytest.mark.parametrize("name", list(FC.CASES))
def test_case_reaches_what_it_is_for(name):
    r = FC.reach(lzo, name)
    print("\n%s: %s" % (name, r))
    for x in FC.CASES[name]["reach"]:
        assert r[x] > 0, (name, r)


def test_empty_chunks_are_empty():
    c = FC.CASES["empty_chunks"]
    verdict, _ = FC.verdicts(lzo, "empty_chunks")
    assert len(verdict) >= 10 * c["capacity"]                               # (at least ten chunks)
    assert (verdict[:FC.EMPTY_CHUNKS * c["capacity"]] != 0).all()
    assert len(FC.expected(lzo, "empty_chunks")["hsps"]) >= 1


def test_bytes_on_the_command_line_has_no_special_byte_under_a_window():
    """why `bytes` cannot reach what bytes_seeding reaches (filter_cases.CASES)"""
    r = FC.reach(lzo, "bytes")
    assert r["special_only"] == 0 and r["lower_kept"] == 0
    v, _, q = FC.sequences("bytes")
    p1, p2, _ = FC.raw_hits(lzo, "bytes")
    up = lzo.upper_nuc_to_bits()
    L = len(FC.CASES["bytes"]["pattern"])
    k = np.arange(L)
    assert (up[v[(p1.astype(np.int64) - L)[:, None] + k]] >= 0).all() and (up[q[(p2.astype(np.int64) - L)[:, None] + k]] >= 0).all()


def _same(a, b):
    return len(a) == len(b) and bool((a == b).all())


def test_cares_12_is_the_search_without_transitions():
    c = FC.CASES["cares_12"]
    v, _, q = FC.sequences("cares_12")
    want, st = lzo.seed_hit_search(lzo.Table(v, lzo.seed(c["pattern"], 0)), q, H.scoring()[1])
    e = FC.expected(lzo, "cares_12")
    assert len(want) > 0 and _same(e["hsps"], want)
    assert (e["extensions"], e["bp_extended"], len(e["hsps"])) == (st["extensions"], st["bp_extended"], st["hsps"]), (e, st)
    assert e["raw"] - e["dropped"] == st["raw_hits"]                        # the kept hits are the exact word's
    assert e["dropped"] > 0


def test_noop_is_the_unfiltered_search():
    c = FC.CASES["noop"]
    v, _, q = FC.sequences("noop")
    want, st = lzo.seed_hit_search(lzo.Table(v, lzo.seed(c["pattern"], c["trans"])), q, H.scoring()[1])
    e = FC.expected(lzo, "noop")
    assert len(want) > 0 and _same(e["hsps"], want) and e["dropped"] == 0
    assert (e["raw"], e["extensions"], e["bp_extended"], len(e["hsps"])) == (st["raw_hits"], st["extensions"], st["bp_extended"], st["hsps"]), (e, st)


def test_chunks_has_at_least_three():
    assert FC.expected(lzo, "chunks")["raw"] > 2 * FC.CASES["chunks"]["capacity"]


@pytest.mark.parametrize("name", FC.GOLDEN_CASES)
def test_statement_rows_are_the_goldens(name):
    gold = FC.parse_rows(M.golden(name))
    assert len(gold) > 0
    if FC.CASES[name]["seq"] == "spaced":                                   # (3 kbp of its query are of the other strand; bytes has none)
        assert {r[6] for r in gold} == {"+", "-"}
    rows = []
    for strand in ("+", "-"):
        rows += FC.rows_of(name, strand, FC.expected(lzo, name, strand)["hsps"])
    assert sorted(rows) == sorted(gold)


@pytest.mark.parametrize("name", M.names())
def test_live_reference_run(tmp_path, name):
    if lzo.ref_binary() is None:
        pytest.skip("oracle/_ref/lastz is not built here (the goldens above always run)")
    assert M.run(name, tmp_path) == M.golden(name)


def _sanitizer_runtime_missing():
    """g++ links -fsanitize=address,undefined only where libasan and libubsan are installed"""
    if shutil.which("g++") is None:
        return "no g++"
    p = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull], input=b"int main() { return 0; }",
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    return None if p.returncode == 0 else "g++ cannot link -fsanitize=address,undefined: " + p.stderr.decode()[-200:]


def test_match_code_predicate_under_the_sanitizers(tmp_path):
    """tests/emul/emul_filter_main.cpp: a program of its own, run as a child process"""
    why = _sanitizer_runtime_missing()
    if why:
        pytest.skip(why)
    exe = str(tmp_path / "emul_filter_main")
    srcs = FC.emul_sources()
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(os.path.dirname(srcs[0]), "emul_filter_main.cpp"), srcs[1]])
    for name in ("whole_2_15", "bytes"):
        c = FC.CASES[name]
        v, _, q = FC.sequences(name)
        p1, p2 = FC.sweep(name)
        files = []
        for tag, a in (("t", v), ("q", q), ("mb", FC.match_bits()), ("p1", p1), ("p2", p2)):
            files.append(str(tmp_path / ("%s_%s.bin" % (name, tag))))
            np.ascontiguousarray(a).tofile(files[-1])
        r = subprocess.run([exe] + files + [str(len(c["pattern"])), str(FC.positions(name)), str(c["M"]), str(-1 if c["T"] is None else c["T"])],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, (name, r.stderr.decode()[-2000:])
        got = np.array([int(x) for x in r.stdout.split()], dtype=np.int64).reshape(-1, 3)
        verdict, counts = FC.by_bytes(name, v, q, p1, p2)
        assert len(got) == len(p1) and (got[:, 0] == (verdict == 0)).all() and (got[:, 1:] == counts).all(), name
