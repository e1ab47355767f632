"""The fused path of scan mode 0 (k_scan_hits2: hit enumeration + phase A over the context-inlined table) against
the two kernels it replaces (LZGPU_FUSED_SCAN=0): identical HSP arrays and counters on synthetic pairs (both
strands), a tandem repeat whose waves' concatenations exceed LZ_F2_CAP, a seed with two transitions (79 probes),
several chunks, tiny task regions and a self-comparison; mode 0 everywhere; and the profile proves which path ran
(a k_fill_hits launch only without the fused path), so that a silent fall-back cannot pass.

Every setting runs in a fresh child process (the switches are read once) under its own time limit, one after the
other; the first child that fails ends the series -- nothing more is started on the GPU after a fault.  Needs an MI355X."""
import pytest

import helpers as H

pytestmark = pytest.mark.gpu
MAIN = ["synth3", "synth4", "synth2m", "tandem", "two_transitions", "chunks", "self_plain"]
SMALL_REGIONS = ["synth3", "tandem"]
#          key                      cases          fused  extra environment
RUNS = [("fused",                   MAIN,          "1",   {}),
        ("split",                   MAIN,          "0",   {}),
        ("fused_small_regions",     SMALL_REGIONS, "1",   {"LZGPU_TASK_REGION_CAP": "2"}),
        ("split_small_regions",     SMALL_REGIONS, "0",   {"LZGPU_TASK_REGION_CAP": "2"})]


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    out = H.run_gpu_children(tmp_path_factory.mktemp("fused"),
                             [(key, "fused_scan_cases", cases, dict(extra, LZGPU_FUSED_SCAN=fused), 600, None) for key, cases, fused, extra in RUNS])
    return {key: (z, {name: m[0] for name, m in meta.items()}) for key, (z, meta) in out.items()}     # one run per case


@pytest.mark.parametrize("a,b,cases", [("fused", "split", MAIN), ("fused_small_regions", "split_small_regions", SMALL_REGIONS),
                                       ("fused_small_regions", "split", SMALL_REGIONS)])
def test_same_hsps_and_counters(runs, a, b, cases):
    (za, ma), (zb, mb) = runs[a], runs[b]
    for name in cases:
        for k in (0, 1):
            x, y = za["%s/0/%d" % (name, k)], zb["%s/0/%d" % (name, k)]
            assert len(x) == len(y) and (x == y).all(), (name, k)
        assert sum(len(za["%s/0/%d" % (name, k)]) for k in (0, 1)) > 0, name
        for c in H.COUNTERS:
            assert ma[name]["counters"][c] == mb[name]["counters"][c], (name, c)


def test_mode_0_and_the_path_that_ran(runs):
    for key, cases, fused, _ in RUNS:
        meta = runs[key][1]
        for name in cases:
            assert meta[name]["scan_modes"] == [0, 0], (key, name)
            la = meta[name]["launches"]
            assert la.get("k_scan_hits", 0) > 0 and la.get("k_partition", 0) > 0, (key, name)
            if fused == "1":
                assert la.get("k_fill_hits", 0) == 0 and la.get("k_build_wctx", 0) > 0, (key, name, la)
            else:
                assert la.get("k_fill_hits", 0) > 0 and la.get("k_build_wctx", 0) == 0, (key, name, la)


def test_cases_reach_what_they_are_for(runs):
    meta = runs["fused"][1]
    assert meta["chunks"]["launches"]["k_scan_hits"] > 4                       # several chunks per strand
    assert meta["tandem"]["counters"]["raw_hits"] > 700 * 40 * 40              # the repeat's lists against the repeat's positions
