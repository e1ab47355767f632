"""lzgpu_seed_hit_search_mismatch (lastz --mismatch=<count>,<length>: k_scan_mismatch and k_settle_mismatch) over the cases of
tests/mismatch_cases.py, against the serial CPU routine of tests/emul/emul_mismatch.cpp (pinned against the pristine binary by
tests/test_mismatch_cases.py) and the goldens themselves.

Per case: the HSPs equal the serial routine's, rows and order; words, raw_hits and hsps equal its counts, extensions and
bp_extended stay where they were; the sorted rows are the golden's; the kernels that ran are the mismatch ones, once per chunk.
`chunks` (spaced at a hit capacity that makes several chunks: diagEnd carried from chunk to chunk) equals `spaced`.  A
resident query slot and an explicit interval work; bucket owners are declined (LZGPU_NH_UNSUPPORTED); more candidates than the
HSP capacity are declined (LZGPU_NH_HSP_OVERFLOW: `long`, at the smallest capacity lzgpu_set_hsp_capacity takes) and the search
succeeds afterwards; M = 0, M = 51 and a length of 0 are LZGPU_ERR_ARG; an --exact search and an X-drop search after a mismatch
search on the same target still give their goldens.  Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

from oracle import lzo
from lastz_amd import lzgpu
import helpers as H
import exact_cases as EC
import mismatch_cases as MC
import window_cases as WC

sys.path.insert(0, H.GOLDEN)
import make_exact_golden as ME                      # noqa: E402
import make_mismatch_golden as M                    # noqa: E402

pytestmark = pytest.mark.gpu
CTB = lzo.upper_nuc_to_bits()
MB = MC.match_bits()
SMALLEST_HSP_CAPACITY = 16                           # lzgpu_set_hsp_capacity declines less
OTHERS = ("k_scan_exact", "k_settle_exact", "k_scan_hits", "k_settle2", "k_scan_hits2", "k_scan_tasks")


def _prepare(gpu, name):
    c = MC.CASES[name]
    v, _, q = MC.sequences(name)
    gpu.table_prepare(v, gpu.seed(c["pattern"], c["trans"]), CTB)
    return q


def _search(gpu, name, q):
    """-> (HSPs, counters, launches per kernel) of the case's search at its hit capacity"""
    c = MC.CASES[name]
    gpu.set_hit_capacity(c["capacity"] or MC.WHOLE)
    gpu.profile_enable(True)
    try:
        gpu.profile_reset(); gpu.counters_reset()
        hs = gpu.seed_hit_search_mismatch(MB, c["M"], c["thr"], q=q)
        return hs, gpu.counters(), {n: v["launches"] for n, v in gpu.profile().items()}
    finally:
        gpu.profile_enable(False)
        gpu.set_hit_capacity(MC.WHOLE)


def _eq(got, want):
    return len(got) == len(want) and bool((got == want).all())


@pytest.mark.parametrize("name", list(MC.CASES))
def test_case_equals_the_serial_routine_and_the_golden(gpu, name):
    want, _, _ = MC.serial(lzo, name)
    _, _, st = MC.raw_hits(lzo, name)
    got, cn, la = _search(gpu, name, _prepare(gpu, name))
    print("\n%s: %d HSPs, launches %s" % (name, len(got), {k: v for k, v in sorted(la.items()) if v}))
    assert _eq(got, want), (name, len(got), len(want))
    assert (got["score"] == got["length"].astype(np.int32)).all()
    assert cn["words"] == st["words"] and cn["raw_hits"] == st["raw_hits"] and cn["hsps"] == len(want), (cn, st)
    assert cn["extensions"] == 0 and cn["bp_extended"] == 0, cn
    assert sorted(MC.rows_of(name, got)) == sorted(MC.parse_rows(M.golden("spaced" if name == "chunks" else name)))
    # the mismatch kernels, once per chunk, and none of the exact-match or X-drop ones
    assert la.get("k_scan_mismatch", 0) >= 1 and la["k_scan_mismatch"] == la.get("k_settle_mismatch", 0) == la.get("k_fill_hits", 0), la
    assert all(la.get(k, 0) == 0 for k in OTHERS), la
    if MC.CASES[name]["capacity"]:
        assert la["k_settle_mismatch"] >= 3, la
    # discovery order, as lzgpu_last_hsp_order states it: ascending sort words
    order = gpu.last_hsp_order(len(got))
    keys = [(int(a), int(b)) for a, b in order]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_chunks_equals_spaced(gpu):
    q = _prepare(gpu, "spaced")
    whole, _, la1 = _search(gpu, "spaced", q)
    parts, _, la2 = _search(gpu, "chunks", q)
    assert la1["k_settle_mismatch"] == 1 and la2["k_settle_mismatch"] >= 3, (la1, la2)
    assert len(whole) > 0 and _eq(parts, whole)


INTERVALS = {"spaced": (842, 3650), "bytes": (251, 2011)}      # both ends cut through an HSP of the whole search


def test_query_slot_and_interval(gpu):
    """a resident query slot (its bytes are what phase B asks for NULs), and a search interval inside the query: the hits of the
    words inside [start, end), extended beyond it as the bases allow (the serial routine on the oracle's hits of that interval)"""
    for name in ("spaced", "bytes"):
        c = MC.CASES[name]
        q = _prepare(gpu, name)
        gpu.query_upload(3, q)
        want, _, _ = MC.serial(lzo, name)
        assert _eq(gpu.seed_hit_search_mismatch(MB, c["M"], c["thr"], slot=3), want), name
        a, b = INTERVALS[name]
        part, _, _ = MC.serial(lzo, name, (a, b))
        assert 0 < len(part) < len(want), (name, len(part), len(want))
        assert int((part["pos2"] - part["length"]).min()) < a and int(part["pos2"].max()) > b, name     # HSPs leave the interval on both sides
        assert _eq(gpu.seed_hit_search_mismatch(MB, c["M"], c["thr"], q=q, start=a, end=b), part), name
        assert _eq(gpu.seed_hit_search_mismatch(MB, c["M"], c["thr"], slot=3, start=a, end=b), part), name


def test_bucket_owners_are_declined(gpu):
    c = MC.CASES["edges"]
    q = _prepare(gpu, "edges")
    gpu.set_bucket_owner(2, 0)
    try:
        with pytest.raises(lzgpu.NotHandled) as e:
            gpu.seed_hit_search_mismatch(MB, c["M"], c["thr"], q=q)
        assert e.value.rc == 7                                              # LZGPU_NH_UNSUPPORTED
    finally:
        gpu.set_bucket_owner(1, 0)
    assert _eq(gpu.seed_hit_search_mismatch(MB, c["M"], c["thr"], q=q), MC.serial(lzo, "edges")[0])


def test_hsp_capacity_overflow_is_declined(gpu):
    c = MC.CASES["long"]
    want, _, _ = MC.serial(lzo, "long")
    assert len(want) > SMALLEST_HSP_CAPACITY
    q = _prepare(gpu, "long")
    gpu.set_hsp_capacity(SMALLEST_HSP_CAPACITY)
    try:
        with pytest.raises(lzgpu.NotHandled) as e:
            gpu.seed_hit_search_mismatch(MB, c["M"], c["thr"], q=q)
        assert e.value.rc == 4                                              # LZGPU_NH_HSP_OVERFLOW
    finally:
        gpu.set_hsp_capacity(WC.HSP_CAPACITY_DEFAULT)
    assert _eq(gpu.seed_hit_search_mismatch(MB, c["M"], c["thr"], q=q), want)


@pytest.mark.parametrize("count,length", [(0, 40), (51, 40), (2, 0)])
def test_bad_arguments(gpu, count, length):
    q = _prepare(gpu, "edges")
    with pytest.raises(lzgpu.LzGpuError) as e:
        gpu.seed_hit_search_mismatch(MB, count, length, q=q)
    assert "rc=-4" in str(e.value)                                          # LZGPU_ERR_ARG


def test_exact_and_xdrop_searches_after_a_mismatch_one(gpu):
    """--exact's `spaced` golden and the adversarial golden (tests/golden/adversarial.hsp.tsv, X-drop) on targets that have
    just been searched with --mismatch: the same match codes serve both, and they do not disturb the scoring codes"""
    c = EC.CASES["spaced"]
    v, _, q = EC.sequences("spaced")
    gpu.table_prepare(v, gpu.seed(c["pattern"], c["trans"]), CTB)
    assert len(gpu.seed_hit_search_mismatch(MB, 2, 40, q=q)) > 0
    got = gpu.seed_hit_search_exact(MB, c["thr"], q=q)
    assert sorted(EC.rows_of("spaced", got)) == sorted(EC.parse_rows(ME.golden("spaced")))
    t, q = H.load_case("adversarial")
    _, masked = H.scoring()
    gpu.table_prepare(t, gpu.seed(), CTB)
    assert len(gpu.seed_hit_search_mismatch(MB, 2, 40, q=q)) > 0
    rows = []
    for strand, _, qq in H.strands(q):
        rows += H.hsps_as_tsv_rows("query", strand, gpu.seed_hit_search(masked, q=qq))
        gpu.seed_hit_search_mismatch(MB, 2, 40, q=qq)                       # ... and in between
    assert rows == H.read_hsp_tsv(os.path.join(H.GOLDEN, "adversarial.hsp.tsv"))
