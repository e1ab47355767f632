"""N-mismatch extension of seed hits (lastz --mismatch) on the CPU, over the cases of tests/mismatch_cases.py.

tests/emul/emul_mismatch.cpp holds a plain serial transcription of what the reference does per raw hit (drop test, the
window's mismatches right to left, the left scan's starts with its three stops, the right scan with shortfall and right stop,
the tie-break, the three forms of the extent) and the GPU's decomposition, compiled from the same header as the kernels
(lastz_amd/csrc/lz_mismatch.hpp): the summary of every hit on its own, then every bucket's records settled in order.  The raw
hits in discovery order are the oracle's, found with the case's real seed (transitions included).

  * the decomposition equals the serial routine: rows, order and the diagEnd it leaves;
  * the serial routine's rows, sorted, are what the pristine binary printed (tests/golden/mismatch_<case>.tsv, recorded by
    tests/golden/make_mismatch_golden.py; run again where oracle/_ref/lastz is present);
  * every case reaches the branches it is for, and the summary's forms occur where the table says;
  * on `background` phase A does not pass by calling everything SLOW;
  * the decomposition alone, in a program of its own, is clean under the address and undefined-behaviour sanitizers.
CPU only."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import lzo
import helpers as H
import mismatch_cases as MC

sys.path.insert(0, H.GOLDEN)
import make_mismatch_golden as M                    # noqa: E402

# the forms of the summary a case must show: SLOW everywhere, and both FAST forms but where the other one was MEASURED to be
# absent -- zero hits of it with the sequences as they stand, printed by the first test below.  `low`'s threshold is about the
# seed's length (no bound is below it), `many` has M = 50 > the seed's length and `edges_m11`'s seed has no don't-care position
# (no window has more than M mismatches); `collide` and `long` merely have no such hit.  Whoever changes a case's sequences
# looks at the printed counts again and puts back the form that has appeared.
FORMS = {name: ("fast_too_many", "fast_no_hsp", "slow") for name in MC.CASES}
FORMS["low"] = ("fast_too_many", "slow")
FORMS["collide"] = FORMS["long"] = ("fast_too_many", "slow")
FORMS["many"] = FORMS["edges_m11"] = ("fast_no_hsp", "slow")


@pytest.mark.parametrize("name", list(MC.CASES))
def test_decomposition_is_the_serial_routine(name):
    want, _, dend_want = MC.serial(lzo, name)
    got, form, dend_got = MC.decomposed(lzo, name)
    assert len(got) == len(want) and (got == want).all(), name
    assert (dend_got == dend_want).all(), name
    seen = np.bincount(form, minlength=3)
    print("\n%s: %d hits, forms %s" % (name, len(form), dict(zip(MC.FORMS, seen.tolist()))))
    for f in FORMS[name]:
        assert seen[MC.FORMS.index(f)] > 0, (name, f, seen)


@pytest.mark.parametrize("name", list(MC.CASES))
def test_serial_rows_are_the_goldens(name):
    gold = MC.parse_rows(M.golden("spaced" if name == "chunks" else name))
    assert len(gold) > 0
    assert sorted(MC.rows_of(name, MC.serial(lzo, name)[0])) == sorted(gold)


@pytest.mark.parametrize("name", list(MC.CASES))
def test_case_reaches_what_it_is_for(name):
    hs, cn, _ = MC.serial(lzo, name)
    print("\n%s: %s" % (name, cn))
    for x in MC.CASES[name]["reach"]:
        assert cn[x] > 0, (name, x, cn)
    assert len(hs) > 0


def test_cases_hold_what_their_names_say():
    assert set(int(x) for x in MC.serial(lzo, "edges")[0]["length"]) == {62}
    c = MC.CASES["edges_m11"]
    assert set(int(x) for x in MC.serial(lzo, "edges_m11")[0]["length"]) == {c["thr"]}        # the >= boundary
    hs = MC.serial(lzo, "many")[0]
    assert MC.CASES["many"]["M"] == 50 and len(hs) > 16
    hs = MC.serial(lzo, "long")[0]
    assert int(hs["length"].max()) == 6004 and len(hs) > 16                 # the 6 kbp block and what matches around it by chance
    rows = MC.rows_of("bytes", MC.serial(lzo, "bytes")[0])
    assert ("t1", 501, 700, "query", 1201, 1400, "+", 200) in rows          # N against N: one mismatch, spanned
    assert len(MC.raw_hits(lzo, "chunks")[0]) > 2 * MC.CASES["chunks"]["capacity"]
    # collide: the HSP whose left end is where the OTHER diagonal's HSP (the short copy, 65,536 further up) ended + 1
    rows = MC.rows_of("collide", MC.serial(lzo, "collide")[0])
    up = [r for r in rows if r[1] > 65536]
    assert len(up) == 1 and any(r[1] < 65536 and r[4] == up[0][5] + 2 for r in rows), rows
    assert MC.serial(lzo, "collide")[1]["other_diagonal"] <= MC.serial(lzo, "collide")[1]["clipped"]


def test_background_is_mostly_fast():
    """SLOW hits are at most the hits inside the planted blocks plus 2 % of the rest"""
    p1, p2, _ = MC.raw_hits(lzo, "background")
    _, form, _ = MC.decomposed(lzo, "background")
    L = len(MC.CASES["background"]["pattern"])
    inside = np.zeros(len(p1), dtype=bool)
    for tp, qp in MC.PLANTED:
        inside |= (p1.astype(np.int64) - p2 == tp - qp) & (p2 - L >= qp) & (p2 <= qp + MC.PLANTED_LEN)
    slow = form == MC.FORMS.index("slow")
    n_in, n_slow = int(inside.sum()), int(slow.sum())
    print("\nbackground: %d hits, %d inside the planted blocks, %d SLOW (%d of them outside), %d FAST with E <= M"
          % (len(p1), n_in, n_slow, int((slow & ~inside).sum()), int((form == 1).sum())))
    assert n_in > 0 and n_slow > 0
    assert n_slow <= n_in + 0.02 * (len(p1) - n_in)
    assert 2 * n_slow < len(p1)                                             # most hits are FAST
    assert (form == MC.FORMS.index("fast_no_hsp")).any()


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


def test_decomposition_under_the_sanitizers(tmp_path):
    """tests/emul/emul_mismatch_main.cpp: a program of its own, run as a child process"""
    why = _sanitizer_runtime_missing()
    if why:
        pytest.skip(why)
    exe = str(tmp_path / "emul_mismatch_main")
    src = os.path.join(os.path.dirname(MC.emul_source()), "emul_mismatch_main.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    for name in ("long", "bytes", "many"):
        c = MC.CASES[name]
        v, _, q = MC.sequences(name)
        p1, p2, _ = MC.raw_hits(lzo, name)
        files = []
        for tag, a in (("t", v), ("q", q), ("mb", MC.match_bits()), ("p1", p1), ("p2", p2)):
            files.append(str(tmp_path / ("%s_%s.bin" % (name, tag))))
            np.ascontiguousarray(a).tofile(files[-1])
        r = subprocess.run([exe] + files + [str(len(c["pattern"])), str(c["M"]), str(c["thr"])], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, (name, r.stderr.decode()[-2000:])
        want = MC.serial(lzo, name)[0]
        got = np.array([int(x) for x in r.stdout.split()], dtype=np.uint32).reshape(-1, 4)
        assert got.tolist() == [[int(h["pos1"]), int(h["pos2"]), int(h["length"]), int(h["score"])] for h in want], name
