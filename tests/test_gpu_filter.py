"""lzgpu_set_hit_filter (lastz --filter: k_filter_mark, k_filter_move) over the cases of tests/filter_cases.py, against the CPU
statement (the reference's predicate over the oracle's raw hits, then the serial search over the hits it keeps; pinned against
the pristine binary by tests/test_filter_cases.py).

Per case: the HSPs equal the statement's, rows and order; raw_hits is the unfiltered count, lzgpu_last_filter_dropped the
statement's rejected count, hsps / extensions / bp_extended those of the surviving hits; the filter kernels ran once per chunk,
on the two-kernel path (k_fill_hits ran: the fused k_scan_hits2 launches none).  After the filter is lifted the plain search
of the same pair is fused again and gives the unfiltered result.  empty_chunks: chunks without a survivor launch nothing
after the filter.  Arguments the header rules out return LZGPU_ERR_ARG, bucket owners LZGPU_NH_UNSUPPORTED, and the next
search without a filter is the unfiltered one.  Needs an MI355X."""
import numpy as np
import pytest

from oracle import lzo
from lastz_amd import lzgpu
import helpers as H
import filter_cases as FC
import pos_filter_cases as PF

pytestmark = pytest.mark.gpu
MB = FC.match_bits()


def _prepare(gpu, name):
    c = FC.CASES[name]
    gpu.table_prepare(FC.sequences(name)[0], gpu.seed(c["pattern"], c["trans"]), FC.table_bits(lzo, name))


def _dispatch(gpu, name, q):
    c = FC.CASES[name]
    if c["kind"] == "exact":
        return gpu.seed_hit_search_exact(MB, c["thr"], q=q)
    if c["kind"] == "mismatch":
        return gpu.seed_hit_search_mismatch(MB, c["mm"], c["thr"], q=q)
    if c["kind"] == "within":
        p = PF.CASES[c["sub"]]
        return gpu.seed_hit_search_within(FC.scoring(name), p["t_iv"], p["q_iv"], q=q, start=p["start"], end=p["end"])
    if c["kind"] == "self":
        return gpu.seed_hit_search_self(FC.scoring(name), q=q, same_strand=True)
    return gpu.seed_hit_search(FC.scoring(name), q=q, extend=c["kind"] != "plain")


def _search(gpu, name, strand="+", filtered=True, capacity=None):
    """-> (HSPs, counters, launches per kernel, dropped) of the case's search at its hit capacity"""
    c = FC.CASES[name]
    gpu.set_hit_capacity(capacity or c["capacity"] or FC.WHOLE)
    if filtered:
        gpu.set_hit_filter(MB, c["M"], -1 if c["T"] is None else c["T"], FC.positions(name))
    gpu.profile_enable(True)
    try:
        gpu.profile_reset(); gpu.counters_reset()
        hs = _dispatch(gpu, name, FC.query_of(name, strand))
        return hs, gpu.counters(), {n: v["launches"] for n, v in gpu.profile().items()}, gpu.last_filter_dropped()
    finally:
        gpu.profile_enable(False)
        gpu.set_hit_filter(None)
        gpu.set_hit_capacity(FC.WHOLE)


def _eq(got, want):
    return len(got) == len(want) and bool((got == want).all())


@pytest.mark.parametrize("name", list(FC.CASES))
def test_case_equals_the_statement(gpu, name):
    c = FC.CASES[name]
    _prepare(gpu, name)
    for strand in c["strands"]:
        e = FC.expected(lzo, name, strand)
        got, cn, la, dropped = _search(gpu, name, strand)
        print("\n%s %s: %d HSPs, %d of %d hits dropped, launches %s" % (name, strand, len(got), dropped, cn["raw_hits"], {k: v for k, v in sorted(la.items()) if v}))
        assert _eq(got, e["hsps"]), (name, strand, len(got), len(e["hsps"]))
        assert cn["raw_hits"] == e["raw"] and cn["words"] == e["words"] and dropped == e["dropped"], (cn, dropped, e["raw"], e["dropped"])
        if c["kind"] != "plain":
            assert (cn["hsps"], cn["extensions"], cn["bp_extended"]) == (len(e["hsps"]), e["extensions"], e["bp_extended"]), (cn, e["extensions"], e["bp_extended"])
            order = gpu.last_hsp_order(len(got))                            # discovery order, as lzgpu_last_hsp_order states it
            keys = [(int(a), int(b)) for a, b in order]
            assert keys == sorted(keys) and len(set(keys)) == len(keys)
        # the filter kernels once per chunk, between the two kernels of the unfused path
        assert la.get("k_fill_hits", 0) >= 1 and la.get("k_filter_mark", 0) == la.get("k_filter_move", 0) == la["k_fill_hits"], la
        if c["capacity"]:
            assert la["k_fill_hits"] >= 3, la
        if name == "noop":
            assert dropped == 0 and la["k_filter_move"] >= 1


def test_chunks_equals_the_whole_capacity_run(gpu):
    _prepare(gpu, "chunks")
    parts, _, la2, d2 = _search(gpu, "chunks")
    whole, _, la1, d1 = _search(gpu, "chunks", capacity=FC.WHOLE)
    assert la1["k_filter_mark"] == 1 and la2["k_filter_mark"] >= 3, (la1, la2)
    assert len(whole) > 0 and _eq(parts, whole) and d1 == d2


def test_lifted_filter_is_the_fused_unfiltered_search(gpu):
    name = "whole_2_15"
    c = FC.CASES[name]
    v, _, q = FC.sequences(name)
    want, st = lzo.seed_hit_search(lzo.Table(v, lzo.seed(c["pattern"], c["trans"])), q, H.scoring()[1])
    _prepare(gpu, name)
    got, _, la, dropped = _search(gpu, name)
    assert dropped > 0 and la["k_fill_hits"] == 1
    got, cn, la, dropped = _search(gpu, name, filtered=False)
    assert _eq(got, want) and dropped == 0
    assert (cn["raw_hits"], cn["extensions"], cn["bp_extended"], cn["hsps"]) == (st["raw_hits"], st["extensions"], st["bp_extended"], st["hsps"])
    # k_scan_hits2 again: enumeration and phase A in one launch, no fill and no filter kernels
    assert la.get("k_scan_hits", 0) == 1 and la.get("k_fill_hits", 0) == 0 and la.get("k_filter_mark", 0) == 0 and la.get("k_filter_move", 0) == 0, la


def test_empty_chunks_launch_nothing_downstream(gpu):
    _prepare(gpu, "empty_chunks")
    got, _, la, _ = _search(gpu, "empty_chunks")
    assert len(got) >= 1
    assert la["k_fill_hits"] >= 10 and la["k_filter_mark"] == la["k_fill_hits"]
    for k in ("k_partition", "k_scan_hits", "k_hist_scan", "k_settle2"):
        assert 1 <= la.get(k, 0) <= la["k_fill_hits"] - FC.EMPTY_CHUNKS, (k, la)


def _unfiltered(gpu, name):
    c = FC.CASES[name]
    v, _, q = FC.sequences(name)
    want, _ = lzo.seed_hit_search(lzo.Table(v, lzo.seed(c["pattern"], c["trans"])), q, H.scoring()[1])
    return _eq(gpu.seed_hit_search(H.scoring()[1], q=q), want) and len(want) > 0


L19 = len(FC.SEED_12OF19)
BAD = {"bit_at_L": dict(min_matches=1, positions=1 << L19), "no_position": dict(min_matches=0, positions=0),
       "more_matches_than_positions": dict(min_matches=13, positions=FC.positions("cares_12")), "negative_matches": dict(min_matches=-1, positions=(1 << L19) - 1)}


@pytest.mark.parametrize("what", list(BAD))
def test_bad_filter_is_an_argument_error(gpu, what):
    name = "whole_2_15"
    _prepare(gpu, name)
    gpu.set_hit_filter(MB, max_transversions=-1, **BAD[what])
    try:
        with pytest.raises(lzgpu.LzGpuError) as e:
            gpu.seed_hit_search(H.scoring()[1], q=FC.sequences(name)[2])
        assert "rc=-4" in str(e.value)                                      # LZGPU_ERR_ARG
    finally:
        gpu.set_hit_filter(None)
    assert _unfiltered(gpu, name)


def test_exact_search_with_other_match_bits_is_an_argument_error(gpu):
    name = "whole_2_15"
    _prepare(gpu, name)
    other = MB.copy()
    other[ord("a")] = -1
    gpu.set_hit_filter(MB, 15, 2, FC.positions(name))
    try:
        with pytest.raises(lzgpu.LzGpuError) as e:
            gpu.seed_hit_search_exact(other, 25, q=FC.sequences(name)[2])
        assert "rc=-4" in str(e.value)
        assert _eq(gpu.seed_hit_search_exact(MB, 25, q=FC.sequences(name)[2]), FC.expected(lzo, "exact")["hsps"])
    finally:
        gpu.set_hit_filter(None)
    assert _unfiltered(gpu, name)


def test_bucket_owners_are_declined(gpu):
    name = "whole_2_15"
    _prepare(gpu, name)
    gpu.set_hit_filter(MB, 15, 2, FC.positions(name))
    gpu.set_bucket_owner(2, 0)
    try:
        with pytest.raises(lzgpu.NotHandled) as e:
            gpu.seed_hit_search(H.scoring()[1], q=FC.sequences(name)[2])
        assert e.value.rc == 7                                              # LZGPU_NH_UNSUPPORTED
    finally:
        gpu.set_bucket_owner(1, 0)
        gpu.set_hit_filter(None)
    assert _unfiltered(gpu, name)


def test_table_calls_do_not_lift_the_filter(gpu):
    name = "whole_2_15"
    c = FC.CASES[name]
    gpu.set_hit_filter(MB, c["M"], c["T"], FC.positions(name))
    try:
        _prepare(gpu, name)
        gpu.table_rebuild()
        assert _eq(gpu.seed_hit_search(FC.scoring(name), q=FC.sequences(name)[2]), FC.expected(lzo, name)["hsps"])
        assert gpu.last_filter_dropped() == FC.expected(lzo, name)["dropped"]
    finally:
        gpu.set_hit_filter(None)
