"""The self-comparison kernels (k_count_sorted_self, k_fill_hits2<true>, k_scan_hits2<true>; lastz --self / --band) against
the oracle's statement of the filter (lzo.seed_hit_search(self_strand=...), pinned on the CPU by
tests/test_self_oracle.py), on the cases of tests/self_cases.py: small repetitive sequences whose table lists are cut
INSIDE on both strands, with

  bands of 1, 61, 500 and 40,000 (both searches of the clip live; a band past the length is no band),
  chunk boundaries under the clip (hit capacities 4096 and 50,000),
  scan modes 1 and 2 forced, and special bytes (N runs, lower case, IUPAC) that make mode 1 by content,
  seeds of 1 and of 79 probes (five trips of the kernels' group loops, the last one partial), a short heavy seed, a
  stepped table, the plain-hit processor, another x-drop and threshold, with and without the entropy adjustment,
  [multi] layouts of 36 records (some no longer than the seed, one of a single base) and of one record.

Per case and strand the HSP arrays equal the oracle's, the five counters equal its sums, and the scan mode and the
profile's launches say that the path the case names is the one that ran.

The cases run in two child processes one after the other, LZGPU_FUSED_SCAN=1 (all cases) and =0 (five of them): the
switch is read once per process.  Each child has its own time limit; the first that fails ends the series -- nothing
more is started on the GPU after a fault, and nothing is tried again.  The entry point's declines are checked in
process.  Needs an MI355X."""
import json

import pytest

from oracle import lzo
from lastz_amd import lzgpu
import helpers as H
import self_cases as S

pytestmark = pytest.mark.gpu
CTB = lzo.upper_nuc_to_bits()
#          key       cases             LZGPU_FUSED_SCAN
RUNS = [("fused",   list(S.CASES),    "1"),
        ("split",   S.SPLIT_CASES,    "0")]
PAIRS = [(key, name) for key, cases, _ in RUNS for name in cases]


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    out = H.run_gpu_children(tmp_path_factory.mktemp("self_matrix"),
                             [(key, "self_cases", cases, {"LZGPU_FUSED_SCAN": fused}, 300, None) for key, cases, fused in RUNS])
    for key, cases, _ in RUNS:
        print("\nself matrix child %s" % key)
        for name in cases:
            for m in out[key][1][name]:
                print("  %-16s capacity %-6s mode %d  %6.3f s  %s" % (name, m["capacity"], m["scan_modes"][-1], m["seconds"],
                      " ".join("%s=%d" % kv for kv in sorted(m["launches"].items()))))
    return out


@pytest.fixture(scope="module")
def oracle():
    """per case: the oracle's HSP arrays of each strand and its counters summed over them (computed once per search:
    cases that differ in library settings only share one)"""
    _, masked = H.scoring()
    out, seen = {}, {}
    for name, c in S.CASES.items():
        key = json.dumps({k: v for k, v in c.items() if k not in ("capacities", "force_mode", "mode", "cli", "twin")})
        if key not in seen:
            seen[key] = S.oracle_search(lzo, name, masked)
        out[name] = seen[key]
    return out


@pytest.mark.parametrize("key,name", PAIRS)
def test_hsps_and_counters_equal_the_oracle(runs, oracle, key, name):
    z, meta = runs[key]
    want, tot = oracle[name]
    assert len(meta[name]) == len(S.CASES[name]["capacities"])
    for r, m in enumerate(meta[name]):
        for k in range(len(S.CASES[name]["strands"])):
            got = z["%s/%d/%d" % (name, r, k)]
            assert len(got) == len(want[k]) and (got == want[k]).all(), (key, name, m["capacity"], k)
        for c in ("words", "raw_hits") if name == "plainhits" else S.COUNTERS:
            assert m["counters"][c] == tot[c], (key, name, m["capacity"], c)
    assert sum(len(h) for h in want) > 0 and tot["raw_hits"] > 0


@pytest.mark.parametrize("key,name", PAIRS)
def test_the_path_that_ran(runs, key, name):
    c = S.CASES[name]
    fused = key == "fused"
    for m in runs[key][1][name]:
        la = m["launches"]
        assert m["scan_modes"] == [c["mode"]] * len(c["strands"]), (key, name, m)
        assert la.get("k_count_hits", 0) > 0, (key, name, la)
        if fused and c["mode"] == 0:
            assert la.get("k_build_wctx", 0) > 0 and la.get("k_fill_hits", 0) == 0, (key, name, la)
        else:                                                           # the split kernels: LZGPU_FUSED_SCAN=0, mode >= 1, plain hits
            assert la.get("k_fill_hits", 0) > 0 and la.get("k_build_wctx", 0) == 0, (key, name, la)
        if c["extend"]:
            assert la.get("k_settle2", 0) > 0 and la.get("k_scan_hits", 0) > 0, (key, name, la)
        else:                                                           # the plain-hit processor extends nothing: no scan, no phase B
            assert la.get("k_settle2", 0) == 0 and la.get("k_scan_hits", 0) == 0, (key, name, la)


@pytest.mark.parametrize("key,name", [(key, name) for key, name in PAIRS if S.CASES[name]["twin"]])
def test_chunked_case_ran_in_more_chunks_than_its_twin(runs, oracle, key, name):
    meta = runs[key][1]
    twin = S.CASES[name]["twin"]
    assert oracle[name] is oracle[twin]                                  # the same rows are expected of both
    whole = runs["fused"][1][twin][0]["launches"] if twin not in meta else meta[twin][0]["launches"]
    for m in meta[name]:
        assert m["launches"]["k_scan_hits"] > whole["k_scan_hits"], (key, name, m["capacity"])
        assert m["launches"]["k_settle2"] > whole["k_settle2"], (key, name, m["capacity"])
    per_capacity = [m["launches"]["k_scan_hits"] for m in meta[name]]
    assert per_capacity == sorted(per_capacity, reverse=True)           # the smaller capacity makes at least as many chunks


def test_entry_point_declines_and_leaves_no_trace(gpu):
    """every condition under which lzgpu_seed_hit_search_self declines -> NotHandled; after each one a plain search on
    the same table is the oracle's non-self search: the self state did not stay behind"""
    _, masked = H.scoring()
    v, _, _ = S.sequence("seed_t0")                                      # rep20, one sequence
    n = len(v)
    gpu.table_prepare(v, gpu.seed(), CTB)
    tab = lzo.Table(v, lzo.seed())
    queries = (v, S.minus(v, []))
    want = [lzo.seed_hit_search(tab, q, masked) for q in queries]

    def plain_search_is_the_oracles():
        for q, (hs, st) in zip(queries, want):
            gpu.counters_reset()
            got = gpu.seed_hit_search(masked, q=q)
            assert len(got) == len(hs) and (got == hs).all()
            c = gpu.counters()
            for k in S.COUNTERS:
                assert c[k] == st[k], k

    half = [0, n // 2, n]
    declines = [("qlen != tlen",            dict(q=v[:-1], same_strand=True)),
                ("a band, opposite strand", dict(q=queries[1], same_strand=False, band_width=500)),
                ("n_sep1 == 1",             dict(q=v, same_strand=True, sep1=[0], sep2=[0])),
                ("n_sep1 != n_sep2",        dict(q=v, same_strand=True, sep1=half, sep2=[0, n])),
                ("separators not ascending", dict(q=v, same_strand=True, sep1=[0, n // 2, n // 2, n], sep2=[0, n // 4, n // 2, n])),
                ("separators descending",   dict(q=queries[1], same_strand=False, sep1=half, sep2=[0, n, n // 2])),
                ("separator past the end",  dict(q=v, same_strand=True, sep1=[0, n + 5], sep2=[0, n]))]
    plain_search_is_the_oracles()
    for what, kw in declines:
        with pytest.raises(lzgpu.NotHandled):
            gpu.seed_hit_search_self(masked, **kw)
        plain_search_is_the_oracles()
    try:
        gpu.set_bucket_owner(2, 0)
        with pytest.raises(lzgpu.NotHandled):
            gpu.seed_hit_search_self(masked, q=v, same_strand=True)
    finally:
        gpu.set_bucket_owner(1, 0)
    plain_search_is_the_oracles()
    # and a self search after all of them still is the oracle's
    got = gpu.seed_hit_search_self(masked, q=v, same_strand=True)
    hs, _ = lzo.seed_hit_search(tab, v, masked, self_strand="same")
    assert len(hs) > 10 and len(got) == len(hs) and (got == hs).all()
