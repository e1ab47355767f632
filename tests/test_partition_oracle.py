"""Pins the oracle's gapped stage on partitioned sequences (lzo_gapped_extend_parts: the limits of the partition holding an
anchor, the trivial alignments of identical sequences and partitions, what inhibit_trivial drops) against outputs of the
pristine reference binary on the cases of tests/partition_cases.py (tests/golden/partition_*.tsv and partition_stats.json,
made by tests/golden/make_partition_golden.py) -- and, where oracle/_ref/lastz is present, against a fresh run.  The oracle
runs end to end: its seed search on the laid-out bytes, reduce_to_points, the gapped stage; its alignments are mapped to
partition names and partition-relative positions and compared with the binary's rows, their order and its "DP cells
visited".  Every case must also reach what it was built for (partition_cases.reaches).  CPU only."""
import os
import sys

import numpy as np
import pytest

from oracle import lzo
import helpers as H
import partition_cases as P

sys.path.insert(0, H.GOLDEN)
import make_partition_golden as M                                  # noqa: E402


@pytest.mark.parametrize("name", list(P.CASES))
def test_case_reaches_what_it_is_for(name):
    assert P.reaches(name) is None, P.CASES[name]["what"]


def test_layouts_are_small():
    for name in P.CASES:
        (v1, _), (v2, _) = P.layout(name)
        assert len(v1) <= 40_000 and len(v2) <= 40_000, name


@pytest.mark.parametrize("name", P.GOLDEN)
def test_oracle_equals_the_recorded_output(name):
    text, cells = M.golden(name)
    rows, mine = P.oracle_rows(name)
    assert rows == P.parse_rows(text)
    assert mine == cells


@pytest.mark.skipif(lzo.ref_binary() is None or lzo.ref_binary(stats=True) is None, reason="oracle/_ref/lastz not built")
@pytest.mark.parametrize("name", P.GOLDEN)
def test_live_reference(tmp_path, name):
    rows, mine = P.oracle_rows(name)
    assert rows == P.parse_rows(M.run(name, tmp_path, binary=lzo.ref_binary()))
    assert mine == M.cells(name, tmp_path, binary=lzo.ref_binary(stats=True))


def test_the_two_older_entry_points_are_calls_of_the_new_one():
    """lzo_gapped_extend / _opts on an unpartitioned pair equal lzo_gapped_extend_parts without separators, and identical
    sequences no longer return 1: they get the trivial self-alignment (src/gapped_extend.c:1152-1189)"""
    import ctypes as C
    pr = P.problems("bounds")[0]
    sub = H.scoring()[0]
    want = P.oracle_problem(pr, sub, sep1=None, sep2=None)
    ta, qa = lzo.nul_terminated(pr["t"]), lzo.nul_terminated(pr["q"])
    anchors = lzo.reduce_to_points(pr["t"], pr["q"], sub, pr["segs"])
    out = C.c_void_p(); n = C.c_uint64(); ops = C.c_void_p(); nops = C.c_uint64(); st = lzo.GappedStats()
    rc = lzo.lib().lzo_gapped_extend(lzo._ptr(ta), len(ta) - 1, lzo._ptr(qa), len(qa) - 1, lzo._ptr(sub), 400, 30, lzo._ptr(anchors), len(anchors),
                                     9400, 1, 3000, 0, C.byref(out), C.byref(n), C.byref(ops), C.byref(nops), C.byref(st))
    assert rc == 0 and n.value == len(want[0]) and nops.value == len(want[1]) and st.dp_cells == want[2]["dp_cells"]
    al = np.zeros(n.value, dtype=lzo.ALIGN_DTYPE); C.memmove(lzo._ptr(al), out, n.value * al.itemsize)
    assert (al == want[0]).all()
    lzo.lib().lzo_free(out); lzo.lib().lzo_free(ops)
    t = pr["t"][1:3000]                                           # (no NUL inside)
    al, op, st = lzo.gapped_extend(t, t | 0x20, sub, np.zeros(0, dtype=lzo.SEG_DTYPE))
    assert len(al) == 1 and tuple(al[0])[:4] == (1, 1, len(t), len(t)) and list(op) == [(len(t) << 2) | 3]
    assert al[0]["s"] == int(sub[t & 0xDF, t & 0xDF].sum()) and st["dp_cells"] == 0
    assert len(lzo.gapped_extend(t, t, sub, np.zeros(0, dtype=lzo.SEG_DTYPE), inhibit_trivial=True)[0]) == 0
    assert len(lzo.gapped_extend(t, t, sub, np.zeros(0, dtype=lzo.SEG_DTYPE), strands_differ=True)[0]) == 0


def _spanning(al, seps):
    return [a for a in al if any(int(a["beg1"]) - 1 < s < int(a["end1"]) for s in seps[1:-1])]


def test_what_default_trimming_shows_of_the_limits():
    """Under default trimming a separator's NUL scores VERY_BAD, so an extension that ignored the limits can never pass
    THROUGH it -- but it passes AROUND it: where the homology goes on in the next partition a one-base gap over the NUL
    costs 430 and the alignment runs on.  So on the cut cases the run without separators has alignments that span a
    separator of the target and the run with them has none, and the cells visited differ everywhere.  Where the
    neighbouring partitions are unrelated (reorder) the alignments are the same with and without the limits and only the
    cells tell the two apart: that is the case the command-line tests of partitioned sequences are in."""
    sub = H.scoring()[0]
    for name in ("flush", "stagger", "reorder"):
        (_, s1), _ = P.layout(name)
        same, cells, spans = True, False, 0
        for pr, r in zip(P.problems(name), P.oracle(name)):
            r0 = P.oracle_problem(pr, sub, sep1=None, sep2=None)
            same = same and P.same(r, r0)
            cells = cells or r[2]["dp_cells"] != r0[2]["dp_cells"]
            spans += len(_spanning(r0[0], s1))
            assert not _spanning(r[0], s1)
        assert cells, name
        assert same == (name == "reorder") and (spans > 0) == (name != "reorder"), (name, same, spans)
