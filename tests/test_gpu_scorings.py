"""The seed and DP kernels under score matrices other than HOXD70 (tests/scorings.py holds the family and says what each
member is for) against the oracle under the same matrix and parameters.

Seed stage: every row of scorings.SEED_CASES on a 300,000 x 250,000 pair (xDrop 15000 on 100,000 x 100,000, the matrix without
mismatch penalties on 20,000 x 20,000), plain and with special bytes sprinkled in, through

  fused    the fused scan kernel (k_scan_hits2, its windows from wctx)                      all rows, plain and specials
  split    LZGPU_FUSED_SCAN=0: k_fill_hits + k_scan_hits (half-overlapping blocks)          the eligible rows, plain and specials
  mode1    scan mode 1 forced: the special-byte masks without special bytes                 the eligible rows, plain
  mode2    scan mode 2 forced: the byte-code scans                                          eight, unit, ext
  chunks   at most 20,000 hits per chunk: diagEnd carries across chunks                     eight, unit

HSP arrays of both strands, the four counters, the scan mode each search took and the kernels the profile saw.  Every
setting runs in a fresh child process (LZGPU_FUSED_SCAN is read once) under its own time limit, one after the other; the
first child that fails ends the series -- nothing more is started on the GPU after a fault.

DP stage: every row of scorings.DP_CASES with either build of the DP kernel forced, in this process: alignments, edit
scripts, and which of k_ydrop / k_ydrop_n / k_ydrop_wide ran.  One window search under the matrix `eight`.  Needs an MI355X."""
import os

import pytest

from oracle import lzo
from lastz_amd import lzgpu
import helpers as H
import scorings as S

pytestmark = pytest.mark.gpu
CTB = lzo.upper_nuc_to_bits()
ALL = list(S.SEED_CASES)
#          key       cases                                                   scan mode  fused
RUNS = [("fused",   ALL + [n + ".s" for n in ALL],                           0,         "1"),
        ("split",   S.ELIGIBLE + [n + ".s" for n in S.ELIGIBLE],             0,         "0"),
        ("mode1",   S.ELIGIBLE,                                              1,         "1"),
        ("mode2",   ["eight", "unit", "ext"],                                2,         "1"),
        ("chunks",  ["eight.c", "unit.c"],                                   0,         "1")]


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    out = H.run_gpu_children(tmp_path_factory.mktemp("scorings"),
                             [(key, "scorings", cases, {"LZGPU_FUSED_SCAN": fused}, 300, mode) for key, cases, mode, fused in RUNS])
    return {key: (z, {case: m[0] for case, m in meta.items()}) for key, (z, meta) in out.items()}     # one run per case


@pytest.fixture(scope="module")
def oracle():
    """per (row, specials): the oracle's HSP arrays of both strands and its counters summed over them (computed once)"""
    cache = {}

    def get(name, specials):
        if (name, specials) not in cache:
            t, q, masked, kw, mode = S.seed_case(name, gpu=True, specials=specials)
            tab = lzo.Table(t, lzo.seed(H.DEFAULT_SEED, 1))
            hs, tot = [], dict.fromkeys(H.COUNTERS, 0)
            for _, _, qq in H.strands(q):
                h, st = lzo.seed_hit_search(tab, qq, masked, **kw)
                hs.append(h)
                for c in H.COUNTERS:
                    tot[c] += st[c]
            cache[(name, specials)] = (hs, tot, mode)
        return cache[(name, specials)]
    return get


@pytest.mark.parametrize("key,case", [(key, case) for key, cases, _, _ in RUNS for case in cases])
def test_hsps_and_counters_equal_the_oracle(runs, oracle, key, case):
    z, meta = runs[key]
    name, specials, _ = S.split_case(case)
    want, tot, _ = oracle(name, specials)
    for k in (0, 1):
        got = z["%s/0/%d" % (case, k)]
        print(key, case, "strand", k, "HSPs", len(got), "oracle", len(want[k]))
        assert len(want[k]) > 0, (key, case, k)                 # the row has HSPs on each strand
        assert len(got) == len(want[k]) and (got == want[k]).all(), (key, case, k)
    for c in H.COUNTERS:
        assert meta[case]["counters"][c] == tot[c], (key, case, c)


def test_the_path_that_ran(runs, oracle):
    for key, cases, forced, fused in RUNS:
        meta = runs[key][1]
        for case in cases:
            name, specials, _ = S.split_case(case)
            mode = max(forced, oracle(name, specials)[2])       # the row's expected mode; 1 at least with special bytes
            la = meta[case]["launches"]
            print(key, case, "scan modes", meta[case]["scan_modes"], "expected", mode,
                  {k: la.get(k, 0) for k in ("k_fill_hits", "k_build_wctx", "k_scan_tasks")})
            assert meta[case]["scan_modes"] == [mode, mode], (key, case)
            if fused == "1" and mode == 0:
                assert la.get("k_fill_hits", 0) == 0 and la.get("k_build_wctx", 0) > 0, (key, case, la)
            else:
                assert la.get("k_fill_hits", 0) > 0 and la.get("k_build_wctx", 0) == 0, (key, case, la)
            if name in ("x15000", "mis0") and mode < 2:
                assert la.get("k_scan_tasks", 0) > 0, (key, case, la)
    assert runs["chunks"][1]["eight.c"]["launches"]["k_settle2"] > runs["fused"][1]["eight"]["launches"]["k_settle2"]     # several chunks


def test_window_search_under_another_matrix(gpu):
    """lzgpu_window_search (the tweener's in-between windows: an exact 7-mer, no entropy) under the matrix `eight`: three
    windows against the oracle run on the cut-out pieces"""
    t, q, masked, kw, _ = S.seed_case("eight")
    gpu.table_prepare(t, gpu.seed(), CTB)
    wins = [(0, 20000, 0, 20000), (len(t) - 20480, 20480, len(q) - 20480, 20480), (27000, 12000, 20000, 9000)]
    isd, osd = gpu.seed("1111111", 0), lzo.seed("1111111", 0)
    got = gpu.window_search(masked, wins, isd, CTB, q=q, hsp_threshold=2200)
    total = 0
    for (t0, tl, q0, ql), g in zip(wins, got):
        want, _ = lzo.seed_hit_search(lzo.Table(t[t0:t0 + tl], osd), q[q0:q0 + ql], masked, hsp_threshold=2200, entropic=False)
        assert len(g) == len(want) and (g == want).all(), (t0, tl, q0, ql)
        total += len(g)
    assert total > 10


# ---- DP stage

@pytest.fixture(scope="module")
def dp_oracle():
    """per DP row: the inputs and, per strand, the oracle's segments, alignments, edit scripts and cell counts (computed once)"""
    cache = {}

    def get(name):
        if name not in cache:
            t, q, sub, masked, (xdrop, thr), kw, expect = S.dp_case(name)
            tab = lzo.Table(t, lzo.seed())
            per = []
            for _, rev, qq in H.strands(q):
                hsps, _ = lzo.seed_hit_search(tab, qq, masked, xdrop=xdrop, hsp_threshold=thr)
                segs = lzo.hsps_to_segments(hsps, rev)
                gkw = dict(gap_open=kw["gap_open"], gap_extend=kw["gap_extend"], ydrop=kw["ydrop"], score_thresh=kw["thresh"])
                oal, oops, ost = lzo.gapped_extend(t, qq, sub, lzo.reduce_to_points(t, qq, sub, segs), **gkw)
                per.append((qq, segs, gkw, oal, oops, ost))
            cache[name] = (t, sub, expect, per)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(S.DP_CASES))
@pytest.mark.parametrize("narrow", ["0", "1"], ids=["four-wave", "two-wave"])
def test_dp_kernels_equal_the_oracle(gpu, dp_oracle, narrow, name):
    t, sub, expect, per = dp_oracle(name)
    old = os.environ.get("LZGPU_DP_NARROW")
    os.environ["LZGPU_DP_NARROW"] = narrow
    try:
        gpu.table_prepare(t, gpu.seed(), CTB)
        gpu.profile_reset(); gpu.profile_enable(True); gpu.counters_reset()
        n_al = 0
        for qq, segs, gkw, oal, oops, ost in per:
            al, ops = gpu.gapped_extend(sub, segs.view(lzgpu.SEG_DTYPE), q=qq, **gkw)
            assert len(al) == len(oal) and (al == oal).all() and (ops == oops).all(), (name, narrow)
            n_al += len(al)
        cells = gpu.counters()["dp_cells"]
        prof = gpu.profile(); gpu.profile_enable(False)
        ran = {k: prof.get(k, {"launches": 0})["launches"] for k in ("k_ydrop", "k_ydrop_n", "k_ydrop_wide")}
        print(name, "LZGPU_DP_NARROW=" + narrow, ran, "alignments", n_al)
        assert n_al > 0
        assert cells == sum(p[5]["dp_cells"] for p in per), (name, narrow)
        # the two-wave kernel and its 16-bit row only where it is asked for and the rule yDrop + gapOE + 1025 + max(score) <= 65535 holds
        two_wave = narrow == "1" and expect != "row32"
        assert ran["k_ydrop_n" if two_wave else "k_ydrop"] > 0 and ran["k_ydrop" if two_wave else "k_ydrop_n"] == 0, (name, narrow, ran)
        assert (ran["k_ydrop_wide"] > 0) == (expect == "wide"), (name, narrow, ran)
    finally:
        if old is None: del os.environ["LZGPU_DP_NARROW"]
        else: os.environ["LZGPU_DP_NARROW"] = old
