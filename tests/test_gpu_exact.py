"""lzgpu_seed_hit_search_exact (lastz --exact=<length>: k_scan_exact and k_settle_exact) over the cases of
tests/exact_cases.py, against the serial CPU routine of tests/emul/emul_exact.cpp (pinned against the pristine binary by
tests/test_exact_cases.py) and the goldens themselves.

Per case: the HSPs equal the serial routine's, rows and order; words, raw_hits and hsps equal its counts, extensions and
bp_extended stay where they were; the sorted rows are the golden's; the kernels that ran are the exact ones.  `chunks`
(spaced at a hit capacity that makes several chunks: diagEnd carried from chunk to chunk) equals `spaced`.  Bucket owners
are declined (LZGPU_NH_UNSUPPORTED), more candidates than the HSP capacity are declined (LZGPU_NH_HSP_OVERFLOW: `long`, at
the smallest capacity lzgpu_set_hsp_capacity takes), and a plain X-drop search after an exact one on the same target still
gives the X-drop golden: the match codes do not disturb the scoring codes.  Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

from oracle import lzo
from lastz_amd import lzgpu
import helpers as H
import exact_cases as EC
import window_cases as WC

sys.path.insert(0, H.GOLDEN)
import make_exact_golden as M                       # noqa: E402

pytestmark = pytest.mark.gpu
CTB = lzo.upper_nuc_to_bits()
MB = EC.match_bits()
SMALLEST_HSP_CAPACITY = 16                           # lzgpu_set_hsp_capacity declines less


def _prepare(gpu, name):
    c = EC.CASES[name]
    v, _, q = EC.sequences(name)
    gpu.table_prepare(v, gpu.seed(c["pattern"], c["trans"]), CTB)
    return q


def _search(gpu, name, q):
    """-> (HSPs, counters, launches per kernel) of the case's search at its hit capacity"""
    c = EC.CASES[name]
    gpu.set_hit_capacity(c["capacity"] or EC.WHOLE)
    gpu.profile_enable(True)
    try:
        gpu.profile_reset(); gpu.counters_reset()
        hs = gpu.seed_hit_search_exact(MB, c["thr"], q=q)
        return hs, gpu.counters(), {n: v["launches"] for n, v in gpu.profile().items()}
    finally:
        gpu.profile_enable(False)
        gpu.set_hit_capacity(EC.WHOLE)


def _eq(got, want):
    return len(got) == len(want) and bool((got == want).all())


@pytest.mark.parametrize("name", list(EC.CASES))
def test_case_equals_the_serial_routine_and_the_golden(gpu, name):
    want, _ = EC.serial(lzo, name)
    _, _, st = EC.raw_hits(lzo, name)
    got, cn, la = _search(gpu, name, _prepare(gpu, name))
    print("\n%s: %d HSPs, launches %s" % (name, len(got), {k: v for k, v in sorted(la.items()) if v}))
    assert _eq(got, want), (name, len(got), len(want))
    assert (got["score"] == got["length"].astype(np.int32)).all()
    assert cn["words"] == st["words"] and cn["raw_hits"] == st["raw_hits"] and cn["hsps"] == len(want), (cn, st)
    assert cn["extensions"] == 0 and cn["bp_extended"] == 0, cn
    assert sorted(EC.rows_of(name, got)) == sorted(EC.parse_rows(M.golden("spaced" if name == "chunks" else name)))
    # the exact kernels, once per chunk, and none of the X-drop ones
    assert la.get("k_scan_exact", 0) >= 1 and la["k_scan_exact"] == la.get("k_settle_exact", 0) == la.get("k_fill_hits", 0), la
    assert la.get("k_scan_hits", 0) == 0 and la.get("k_settle2", 0) == 0 and la.get("k_scan_tasks", 0) == 0, la
    if EC.CASES[name]["capacity"]:
        assert la["k_settle_exact"] >= 3, la
    # discovery order, as lzgpu_last_hsp_order states it: ascending sort words
    order = gpu.last_hsp_order(len(got))
    keys = [(int(a), int(b)) for a, b in order]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_chunks_equals_spaced(gpu):
    q = _prepare(gpu, "spaced")
    whole, _, la1 = _search(gpu, "spaced", q)
    parts, _, la2 = _search(gpu, "chunks", q)
    assert la1["k_settle_exact"] == 1 and la2["k_settle_exact"] >= 3, (la1, la2)
    assert len(whole) > 0 and _eq(parts, whole)


def test_query_slot_and_interval(gpu):
    """a resident query slot, and the search interval: the hits of the words inside [start, end)"""
    name = "spaced"
    q = _prepare(gpu, name)
    gpu.query_upload(3, q)
    want, _ = EC.serial(lzo, name)
    assert _eq(gpu.seed_hit_search_exact(MB, EC.CASES[name]["thr"], slot=3), want)
    a = gpu.seed_hit_search_exact(MB, EC.CASES[name]["thr"], q=q, start=0, end=len(q))
    assert _eq(a, want)


def test_bucket_owners_are_declined(gpu):
    q = _prepare(gpu, "edges")
    gpu.set_bucket_owner(2, 0)
    try:
        with pytest.raises(lzgpu.NotHandled) as e:
            gpu.seed_hit_search_exact(MB, EC.CASES["edges"]["thr"], q=q)
        assert e.value.rc == 7                                              # LZGPU_NH_UNSUPPORTED
    finally:
        gpu.set_bucket_owner(1, 0)
    assert _eq(gpu.seed_hit_search_exact(MB, EC.CASES["edges"]["thr"], q=q), EC.serial(lzo, "edges")[0])


def test_hsp_capacity_overflow_is_declined(gpu):
    want, _ = EC.serial(lzo, "long")
    assert len(want) > SMALLEST_HSP_CAPACITY
    q = _prepare(gpu, "long")
    gpu.set_hsp_capacity(SMALLEST_HSP_CAPACITY)
    try:
        with pytest.raises(lzgpu.NotHandled) as e:
            gpu.seed_hit_search_exact(MB, EC.CASES["long"]["thr"], q=q)
        assert e.value.rc == 4                                              # LZGPU_NH_HSP_OVERFLOW
    finally:
        gpu.set_hsp_capacity(WC.HSP_CAPACITY_DEFAULT)
    assert _eq(gpu.seed_hit_search_exact(MB, EC.CASES["long"]["thr"], q=q), want)


def test_xdrop_search_after_an_exact_one(gpu):
    """the adversarial golden (tests/golden/adversarial.hsp.tsv, X-drop) on a target that has just been searched with --exact"""
    t, q = H.load_case("adversarial")
    _, masked = H.scoring()
    gpu.table_prepare(t, gpu.seed(), CTB)
    assert len(gpu.seed_hit_search_exact(MB, 40, q=q)) > 0
    rows = []
    for strand, _, qq in H.strands(q):
        rows += H.hsps_as_tsv_rows("query", strand, gpu.seed_hit_search(masked, q=qq))
        gpu.seed_hit_search_exact(MB, 40, q=qq)                             # ... and in between
    assert rows == H.read_hsp_tsv(os.path.join(H.GOLDEN, "adversarial.hsp.tsv"))
