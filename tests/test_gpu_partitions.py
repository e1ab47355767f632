"""The gapped stage on partitioned sequences, GPU tier: every case of tests/partition_cases.py through lzgpu_gapped_extend /
_batch with sep1 / sep2, strands_differ and inhibit_trivial, against the oracle -- alignments, edit scripts, their order and
the reference's "DP cells visited" -- and, for the --noytrim and trivial-alignment cases, against the pristine binary's
recorded output (tests/golden/partition_*.tsv).  The cases are small (layouts below 40 kbp); what each is for is asserted
on the CPU by tests/test_partition_oracle.py.  Needs an MI355X; reads only the repository."""
import os
import sys

import numpy as np
import pytest

from oracle import lzo
from lastz_amd import lzgpu
import helpers as H
import partition_cases as P

sys.path.insert(0, H.GOLDEN)
import make_partition_golden as M                                  # noqa: E402

pytestmark = pytest.mark.gpu
NH_IDENTICAL = 6


def _kw(pr):
    """the library's arguments of one problem of a case"""
    return dict(pr["kw"], sep1=pr["sep1"], sep2=pr["sep2"], reduce=pr["reduce"])


def _run(gpu, name):
    """the case on the GPU, strand after strand -> [(alignments, ops, counters) or the decline code]"""
    sub = P.scoring(name)[0]
    prs = P.problems(name)
    gpu.target_upload(prs[0]["t"])
    out = []
    for pr in prs:
        gpu.counters_reset()
        try:
            al, ops = gpu.gapped_extend(sub, pr["segs"].view(lzgpu.SEG_DTYPE), q=pr["q"], **_kw(pr))
        except lzgpu.NotHandled as e:
            out.append(e.rc)
            continue
        out.append((al, ops, gpu.counters()))
    return out


def _check(name, got):
    """a case's GPU results against the oracle; a strand whose answer hangs on the sequences' names must be declined"""
    declined = False
    for pr, g, (oal, oops, ost) in zip(P.problems(name), got, P.oracle(name)):
        if ost["trivial_candidate"]:
            assert g == NH_IDENTICAL, (name, pr["strand"], g)
            declined = True
            continue
        assert not isinstance(g, int), (name, pr["strand"], g)
        al, ops, c = g
        assert len(al) == len(oal) and (al == oal).all() and len(ops) == len(oops) and (ops == oops).all(), (name, pr["strand"])
        assert c["dp_cells"] == ost["dp_cells"] and c["anchors_extended"] == ost["anchors_extended"], (name, pr["strand"], c, ost)
    assert declined == P.CASES[name]["declined"], name


@pytest.mark.parametrize("name", list(P.CASES))
def test_case_equals_the_oracle(gpu, name):
    if name == "wide":
        gpu.profile_reset(); gpu.profile_enable(True)
    try:
        got = _run(gpu, name)
    finally:
        prof = gpu.profile() if name == "wide" else None
        gpu.profile_enable(False)
    _check(name, got)
    if name == "wide":                                          # gap 200 / 5: the band does not fit the LDS ring
        assert prof.get("k_ydrop_wide", {"launches": 0})["launches"] > 0
    if name in P.GOLDEN and (name in P.NO_TRIM or name in P.TRIVIAL):
        text, cells = M.golden(name)                            # ... and the pristine binary's output
        rows = []
        for pr, (al, ops, _) in zip(P.problems(name), got):
            rows += P.rows_of(name, pr["strand"], al, ops)
        assert rows == P.parse_rows(text)
        assert sum(c["dp_cells"] for _, _, c in got) == cells


def test_bounds_across_rounds(gpu):
    """one anchor per round, three, and the default: later anchors are bounded by alignments of earlier rounds, of their own
    and of other partitions -- the same result whatever the window"""
    try:
        for window in (1, 3, 0):
            gpu.set_dp_window(window)
            _check("bounds", _run(gpu, "bounds"))
    finally:
        gpu.set_dp_window(0)


@pytest.mark.parametrize("narrow", ["0", "1"])
@pytest.mark.parametrize("repl", ["0", "1"])
def test_both_builds_and_row_setups(gpu, narrow, repl):
    """k_ydrop (four waves, 32-bit row) and k_ydrop_n (two waves, 16-bit row), the row set-up on one wave and on all: the
    partition's last row and column under --noytrim, and bounds across partitions"""
    os.environ["LZGPU_DP_NARROW"] = narrow; os.environ["LZGPU_DP_REPL"] = repl
    try:
        gpu.profile_reset(); gpu.profile_enable(True)
        for name in ("flush_notrim", "bounds"):
            _check(name, _run(gpu, name))
        prof = gpu.profile()
    finally:
        gpu.profile_enable(False)
        del os.environ["LZGPU_DP_NARROW"]; del os.environ["LZGPU_DP_REPL"]
    assert prof.get("k_ydrop_n" if narrow == "1" else "k_ydrop", {"launches": 0})["launches"] > 0
    assert prof.get("k_ydrop" if narrow == "1" else "k_ydrop_n", {"launches": 0})["launches"] == 0


def _rectangles():
    """two rectangles of the flush layouts, each starting on a separator and ending in front of one, with the separators
    inside them relative to the rectangle -> [(t_off, t_len, q_off, q_len, sep1, sep2)]"""
    (v1, s1), (v2, s2) = P.layout("flush")
    out = []
    for (a1, b1), (a2, b2) in (((1, 3), (1, 4)), ((0, 2), (0, 2))):
        out.append((s1[a1], s1[b1] - s1[a1], s2[a2], s2[b2] - s2[a2], [s - s1[a1] for s in s1[a1:b1 + 1]], [s - s2[a2] for s in s2[a2:b2 + 1]]))
    return out


@pytest.mark.parametrize("no_trim", [False, True])
def test_rectangle_with_separators(gpu, no_trim):
    """t_off / t_len / q_off / q_len on a resident partitioned pair, separators relative to the rectangle: the oracle on the
    cut-out pieces, one call each and as one batch"""
    (v1, s1), (v2, s2) = P.layout("flush")
    sub, masked = H.scoring()
    gpu.target_upload(v1)
    gpu.query_upload(0, v2)
    problems, want = [], []
    for t0, tl, q0, ql, r1, r2 in _rectangles():
        tt, qq = v1[t0:t0 + tl], v2[q0:q0 + ql]
        hsps, _ = lzo.seed_hit_search(lzo.Table(tt, lzo.seed()), qq, masked)
        segs = lzo.hsps_to_segments(hsps, 0)
        want.append(lzo.gapped_extend(tt, qq, sub, lzo.reduce_to_points(tt, qq, sub, segs), sep1=r1, sep2=r2, trim_to_peak=not no_trim))
        problems.append(dict(anchors=segs.view(lzgpu.SEG_DTYPE), slot=0, t_off=t0, t_len=tl, q_off=q0, q_len=ql, sep1=r1, sep2=r2, no_trim=no_trim))
    assert all(len(w[0]) >= 3 for w in want)
    for pr, (oal, oops, ost) in zip(problems, want):            # one at a time ...
        pr1 = dict(pr)
        gpu.counters_reset()
        al, ops = gpu.gapped_extend(sub, pr1.pop("anchors"), **pr1)
        assert len(al) == len(oal) and (al == oal).all() and (ops == oops).all()
        assert gpu.counters()["dp_cells"] == ost["dp_cells"]
    gpu.counters_reset()
    for (al, ops), (oal, oops, _) in zip(gpu.gapped_extend_batch(sub, problems), want):    # ... and as one batch
        assert len(al) == len(oal) and (al == oal).all() and (ops == oops).all()
    assert gpu.counters()["dp_cells"] == sum(w[2]["dp_cells"] for w in want)


def test_batch_of_partitionings(gpu):
    """three problems against one resident partitioned target -- the query cut at the target's points, cut elsewhere, and not
    cut at all -- in one batch: what one call each gives, and what the oracle gives"""
    sub = H.scoring()[0]
    prs = [P.problems(name)[0] for name in ("flush", "stagger", "t_only")]
    assert all((pr["t"] == prs[0]["t"]).all() for pr in prs)
    want = [P.oracle(name)[0] for name in ("flush", "stagger", "t_only")]
    gpu.target_upload(prs[0]["t"])
    problems = []
    for slot, pr in enumerate(prs):
        gpu.query_upload(slot, pr["q"])
        problems.append(dict(_kw(pr), anchors=pr["segs"].view(lzgpu.SEG_DTYPE), slot=slot))
    single = []
    for pr in problems:
        pr1 = dict(pr)
        single.append(gpu.gapped_extend(sub, pr1.pop("anchors"), **pr1))
    gpu.counters_reset()
    batch = gpu.gapped_extend_batch(sub, problems)
    assert gpu.counters()["dp_cells"] == sum(w[2]["dp_cells"] for w in want)
    for (al, ops), (sal, sops), (oal, oops, _) in zip(batch, single, want):
        assert len(al) == len(sal) and (al == sal).all() and (ops == sops).all()
        assert len(al) == len(oal) and (al == oal).all() and (ops == oops).all()
