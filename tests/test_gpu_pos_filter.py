"""lzgpu_seed_hit_search_within (lastz --chores: seed hits limited to a target and a query interval) against the oracle's
statement of it -- the search of a position table that holds only the words inside the target interval, over the search
interval intersected with the query interval (pinned against the pristine binary by tests/test_pos_filter_oracle.py) --
on the cases of tests/pos_filter_cases.py: a 40 kbp / 22 kbp pair whose table lists of 150 entries are cut INSIDE on both
ends, with

  the whole target as the window (= the unfiltered search), ends beyond the sequences (clamped),
  windows of one seed length and of one base less (empty), in the target and in the query,
  a window edge on a list's first and last entry, each +- 1,
  three and more chunks of surviving hits (hit capacities 4096 and 50,000), the query interval ending inside one,
  scan modes 1 and 2 forced, and special bytes (N, lower case, IUPAC; the NULs of a [multi] target) that make mode 1,
  seeds of 1 and of 79 probes, a stepped table of a short seed, the plain-hit processor.

Per case and strand the HSP arrays equal the oracle's, the five counters equal its sums, and the scan mode and the
profile's launches say that the path the case names is the one that ran.

The cases run in two child processes one after the other, LZGPU_FUSED_SCAN=1 (all cases) and =0 (seven of them): the
switch is read once per process.  Each child has its own time limit; the first that fails ends the series -- nothing more
is started on the GPU after a fault, and nothing is tried again.  Declines, argument errors, a self-comparison after a
filtered search and the chores of the goldens with lastz's fences are checked in process.  Needs an MI355X."""
import json

import numpy as np
import pytest

from oracle import lzo
from lastz_amd import lzgpu
import helpers as H
import self_cases as S
import pos_filter_cases as P
import chores_golden as CG

pytestmark = pytest.mark.gpu
CTB = lzo.upper_nuc_to_bits()
#          key       cases             LZGPU_FUSED_SCAN
RUNS = [("fused",   list(P.CASES),    "1"),
        ("split",   P.SPLIT_CASES,    "0")]
PAIRS = [(key, name) for key, cases, _ in RUNS for name in cases]


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    out = H.run_gpu_children(tmp_path_factory.mktemp("pos_filter"),
                             [(key, "pos_filter_cases", cases, {"LZGPU_FUSED_SCAN": fused}, 300, None) for key, cases, fused in RUNS])
    for key, cases, _ in RUNS:
        print("\nposition filter child %s" % key)
        for name in cases:
            for m in out[key][1][name]:
                print("  %-14s capacity %-6s modes %s  %6.3f s  %s" % (name, m["capacity"], m["scan_modes"], m["seconds"],
                      " ".join("%s=%d" % kv for kv in sorted(m["launches"].items()))))
    return out


@pytest.fixture(scope="module")
def oracle():
    """per case: the oracle's HSP arrays of each strand and its counters summed over them (cases that differ in library
    settings only share one search)"""
    _, masked = H.scoring()
    out, seen = {}, {}
    for name, c in P.CASES.items():
        key = json.dumps({k: v for k, v in c.items() if k not in ("capacity", "force_mode", "mode", "empty", "min_chunks")})
        if key not in seen:
            seen[key] = P.oracle_search(lzo, name, masked)
        out[name] = seen[key]
    return out


@pytest.mark.parametrize("key,name", PAIRS)
def test_hsps_and_counters_equal_the_oracle(runs, oracle, key, name):
    z, meta = runs[key]
    want, tot = oracle[name]
    (m,) = meta[name]
    for k in range(2):
        got = z["%s/0/%d" % (name, k)]
        assert len(got) == len(want[k]) and (got == want[k]).all(), (key, name, k)
    for c in ("words", "raw_hits") if not P.CASES[name]["extend"] else P.COUNTERS:
        assert m["counters"][c] == tot[c], (key, name, c)
    if P.CASES[name]["empty"]:
        assert tot["raw_hits"] == 0 and sum(len(h) for h in want) == 0
    else:
        assert sum(len(h) for h in want) > 0 and tot["raw_hits"] > 0


def test_the_cases_cut_what_they_say(oracle):
    """the expectations themselves: lists cut inside, the whole window = the unfiltered search, every +- 1 moves a hit"""
    _, masked = H.scoring()
    plain = P.oracle_search(lzo, "whole", masked, filtered=False)
    for twin in P.UNFILTERED_TWINS:
        assert all((a == b).all() for a, b in zip(oracle[twin][0], plain[0])) and oracle[twin][1] == plain[1]
    raw = {k: oracle[k][1]["raw_hits"] for k in P.CASES}
    assert 0 < raw["inside"] < raw["whole"] and raw["inside_q"] < raw["inside"]
    assert raw["first_m1"] < raw["first_0"] < raw["first_p1"] and raw["last_m1"] > raw["last_0"] > raw["last_p1"]
    assert 0 < raw["one_seed"] < 200 and 0 < raw["q_one_seed"] < 200
    assert raw["probes_1"] < raw["probes_79"]


@pytest.mark.parametrize("key,name", PAIRS)
def test_the_path_that_ran(runs, key, name):
    c = P.CASES[name]
    fused = key == "fused"
    (m,) = runs[key][1][name]
    la = m["launches"]
    if c["empty"]:                                                      # no window fits: nothing is launched
        assert not la.get("k_count_hits", 0) and not la.get("k_scan_hits", 0) and not la.get("k_fill_hits", 0), (key, name, la)
        return
    assert m["scan_modes"] == [c["mode"]] * 2, (key, name, m)
    assert la.get("k_count_hits", 0) > 0, (key, name, la)
    if fused and c["mode"] == 0:
        assert la.get("k_build_wctx", 0) > 0 and la.get("k_fill_hits", 0) == 0, (key, name, la)
    else:                                                               # the split kernels: LZGPU_FUSED_SCAN=0, mode >= 1, plain hits
        assert la.get("k_fill_hits", 0) > 0 and la.get("k_build_wctx", 0) == 0, (key, name, la)
    if c["extend"]:
        assert la.get("k_settle2", 0) >= c["min_chunks"] and la.get("k_scan_hits", 0) >= c["min_chunks"], (key, name, la)
    else:                                                               # the plain-hit processor extends nothing: no scan, no phase B
        assert la.get("k_settle2", 0) == 0 and la.get("k_scan_hits", 0) == 0, (key, name, la)


def test_declines_and_argument_errors_leave_no_trace(gpu):
    """every decline and argument error of the entry point; after each one a plain search on the same table is the oracle's
    unfiltered search, and so is a self-comparison after a filtered search"""
    _, masked = H.scoring()
    v, _, _ = S.sequence("seed_t0")                                      # rep20, one sequence
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

    plain_search_is_the_oracles()
    errors = [("t_start > t_end", dict(t_interval=(5000, 4999), q_interval=(0, 20000))),
              ("q_start > q_end", dict(t_interval=(0, 20000), q_interval=(300, 299))),
              ("void search interval", dict(t_interval=(0, 20000), q_interval=(0, 20000), start=500, end=400)),
              ("search interval past the end", dict(t_interval=(0, 20000), q_interval=(0, 20000), end=len(v) + 1))]
    for what, kw in errors:
        with pytest.raises(lzgpu.LzGpuError, match="rc=-4"):             # LZGPU_ERR_ARG
            gpu.seed_hit_search_within(masked, q=v, **kw)
        plain_search_is_the_oracles()
    try:
        gpu.set_bucket_owner(2, 0)
        with pytest.raises(lzgpu.NotHandled) as e:
            gpu.seed_hit_search_within(masked, (4000, 6000), (0, 20000), q=v)
        assert e.value.rc == 7                                           # LZGPU_NH_UNSUPPORTED
    finally:
        gpu.set_bucket_owner(1, 0)
    plain_search_is_the_oracles()
    # a filtered search, an empty one, then the plain search and a self-comparison: each its usual result
    t_iv, q_iv = (4000 + 61 * 10, 4000 + 61 * 30), (0, len(v))
    got = gpu.seed_hit_search_within(masked, t_iv, q_iv, q=v)
    hs, _ = lzo.seed_hit_search(lzo.Table(v, lzo.seed(), start=t_iv[0], end=t_iv[1]), v, masked)
    assert len(hs) > 10 and len(got) == len(hs) and (got == hs).all()
    order = gpu.last_hsp_order(len(got))                                 # discovery order: query position, then descending target
    assert gpu.last_scan_mode() == 0 and (np.diff(order[:, 0].astype(np.int64)) >= 0).all()
    assert len(gpu.seed_hit_search_within(masked, (7000, 7000), q_iv, q=v)) == 0
    plain_search_is_the_oracles()
    got = gpu.seed_hit_search_self(masked, q=v, same_strand=True)
    hs, _ = lzo.seed_hit_search(tab, v, masked, self_strand="same")
    assert len(hs) > 10 and len(got) == len(hs) and (got == hs).all()
    plain_search_is_the_oracles()


@pytest.mark.parametrize("name", CG.NAMES)
def test_chores_of_the_goldens_with_fences(gpu, name):
    """a chores run as lastz drives it: the target's fences patched into the device's copy, the query handed in with its own,
    the filtered search, the fences taken away -- per chore and strand the oracle's rows (which are the pristine binary's:
    tests/test_pos_filter_oracle.py), and afterwards the unfenced target is back"""
    _, masked = H.scoring()
    t, qs = CG.sequences()
    gpu.table_prepare(t, gpu.seed(), CTB)
    n_rows = 0
    for qname, strand, tf, qf, t_iv, q_iv in CG.searches(name):
        at = np.flatnonzero(tf != t)
        gpu.target_patch(at, tf[at])
        try:
            got = gpu.seed_hit_search_within(masked, t_iv, q_iv, q=qf)
        finally:
            gpu.target_patch(at, t[at])
        want, _ = CG.oracle_hsps(tf, qf, t_iv, q_iv, masked)
        assert len(got) == len(want) and (got == want).all(), (name, qname, strand, t_iv, q_iv)
        n_rows += len(want)
    assert n_rows > 5
    q = qs["pig1"]
    got = gpu.seed_hit_search(masked, q=q)
    want, _ = lzo.seed_hit_search(lzo.Table(t, lzo.seed()), q, masked)
    assert len(want) > 0 and len(got) == len(want) and (got == want).all()
    with pytest.raises(lzgpu.LzGpuError, match="rc=-4"):
        gpu.target_patch([len(t)], [0])
