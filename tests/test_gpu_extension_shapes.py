"""lzgpu_seed_hit_search_exact, lzgpu_seed_hit_search_mismatch and lzgpu_set_hit_filter (k_scan_exact / k_settle_exact,
k_scan_mismatch / k_settle_mismatch, k_filter_mark / k_filter_move) over the cases of tests/extension_shape_cases.py: seeds of
length 31, 29, 22, 14, 4, 3 and 2, tables with --step=3, on an interval, under a word-count limit, with the limit lifted again,
and a table masked in place -- against the CPU statement (the oracle's raw hits of its own table, the reference's filter routine
byte by byte, the serial routines; pinned against the pristine binary by tests/test_extension_shapes.py) and the goldens.

Per case and strand: the HSPs equal the statement's, rows and order; words, raw_hits and hsps equal its counts, extensions and
bp_extended are 0 for --exact / --mismatch and the statement's for an X-drop search; lzgpu_last_filter_dropped is the statement's;
the kernels that ran are the family's own, once per chunk, with the filter kernels between k_fill_hits and the scan; a chunked
run equals the run at whole capacity; the plus and minus rows together are the golden's.  Needs an MI355X."""
import sys

import numpy as np
import pytest

from oracle import lzo
import helpers as H
import extension_shape_cases as X
import table_mask_cases as TM

sys.path.insert(0, H.GOLDEN)
import make_extension_shapes_golden as M            # noqa: E402

pytestmark = pytest.mark.gpu
CTB = lzo.upper_nuc_to_bits()
MB = X.match_bits()
FAMILY = {"exact": ("k_scan_exact", "k_settle_exact"), "mismatch": ("k_scan_mismatch", "k_settle_mismatch"), "xdrop": ("k_scan_hits", "k_settle2")}
FOREIGN = {"exact": ("k_scan_mismatch", "k_settle_mismatch", "k_scan_hits", "k_settle2", "k_scan_hits2", "k_scan_tasks"),
           "mismatch": ("k_scan_exact", "k_settle_exact", "k_scan_hits", "k_settle2", "k_scan_hits2", "k_scan_tasks"),
           "xdrop": ("k_scan_exact", "k_settle_exact", "k_scan_mismatch", "k_settle_mismatch")}


def _prepare(gpu, name):
    """the case's table on the device; a masked case's as lastz leaves it after the event: the 'x' bytes, then one table_mask"""
    c = X.CASES[name]
    s, e = c["interval"] or (0, 0)
    v = X.unmasked_target() if c["mask"] else X.sequences(lzo, name)[0]
    gpu.table_prepare(v, gpu.seed(c["pattern"], c["trans"]), CTB, step=c["step"], start=s, end=e)
    if c["limit"]:
        gpu.table_limit(c["limit"])
    if c["lifted"]:
        gpu.table_limit(c["lifted"])
        assert gpu.table_num_words() < int(X.table(lzo, name).pt.contents.words_in_table)
        gpu.table_limit(0)


def _mask(gpu):
    widened, cores, t_masked = X.mask_event(lzo)
    for s, e in widened:
        gpu.target_update(s, t_masked[s:e])
    gpu.table_mask(widened)


def _dispatch(gpu, c, q):
    if c["kind"] == "exact":
        return gpu.seed_hit_search_exact(MB, c["thr"], q=q)
    if c["kind"] == "mismatch":
        return gpu.seed_hit_search_mismatch(MB, c["mm"], c["thr"], q=q)
    return gpu.seed_hit_search(H.scoring()[1], q=q)


def _search(gpu, name, strand="+", capacity=None):
    """-> (HSPs, counters, launches per kernel, dropped) of the case's search of one strand at its hit capacity"""
    c = X.CASES[name]
    gpu.set_hit_capacity(capacity or c["capacity"] or X.WHOLE)
    if c["filt"]:
        gpu.set_hit_filter(MB, c["M"], -1 if c["T"] is None else c["T"], X.FC.positions(c))
    gpu.profile_enable(True)
    try:
        gpu.profile_reset(); gpu.counters_reset()
        hs = _dispatch(gpu, c, X.query_of(lzo, name, strand))
        return hs, gpu.counters(), {n: v["launches"] for n, v in gpu.profile().items()}, gpu.last_filter_dropped()
    finally:
        gpu.profile_enable(False)
        gpu.set_hit_filter(None)
        gpu.set_hit_capacity(X.WHOLE)


def _eq(got, want):
    return len(got) == len(want) and bool((got == want).all())


def _check(gpu, name, strand, got, cn, la, dropped):
    c = X.CASES[name]
    e = X.statement(lzo, name, strand)
    print("\n%s %s: %d HSPs, %d of %d hits dropped, launches %s" % (name, strand, len(got), dropped, cn["raw_hits"], {k: v for k, v in sorted(la.items()) if v}))
    assert _eq(got, e["hsps"]), (name, strand, len(got), len(e["hsps"]))
    assert cn["words"] == e["words"] and cn["raw_hits"] == e["raw"] and cn["hsps"] == len(e["hsps"]), (cn, e["words"], e["raw"])
    assert (cn["extensions"], cn["bp_extended"]) == (e["extensions"], e["bp_extended"]), (cn, e["extensions"], e["bp_extended"])
    assert dropped == e["dropped"], (dropped, e["dropped"])
    if c["kind"] != "xdrop":
        assert (got["score"] == got["length"].astype(np.int32)).all()
    # the family's own kernels, once per chunk that has a hit left, and none of the other families'
    scan, settle = FAMILY[c["kind"]]
    fills = la.get("k_fill_hits", 0)
    assert fills >= 1 and 1 <= la.get(scan, 0) <= fills and 1 <= la.get(settle, 0) <= fills, la
    assert c["kind"] == "xdrop" or la[scan] == la[settle], la
    assert all(la.get(k, 0) == 0 for k in FOREIGN[c["kind"]]), la
    if c["filt"]:
        assert la.get("k_filter_mark", 0) == la.get("k_filter_move", 0) == fills, la
    else:
        assert la[scan] == fills and la.get("k_filter_mark", 0) == 0 and la.get("k_filter_move", 0) == 0, la
    if c["capacity"] and e["raw"] > 2 * c["capacity"]:                     # (the plus strand always: test_extension_shapes.py)
        assert fills >= 3, la
    order = gpu.last_hsp_order(len(got))                                    # discovery order, as lzgpu_last_hsp_order states it
    keys = [(int(a), int(b)) for a, b in order]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


@pytest.mark.parametrize("name", [n for n, c in X.CASES.items() if not c["mask"]])
def test_case_equals_the_statement_and_the_golden(gpu, name):
    c = X.CASES[name]
    rows = []
    try:
        _prepare(gpu, name)
        for strand in c["strands"]:
            got, cn, la, dropped = _search(gpu, name, strand)
            _check(gpu, name, strand, got, cn, la, dropped)
            rows += X.rows_of(lzo, name, strand, got)
            if c["capacity"]:                                                   # chunks: diagEnd carried from chunk to chunk
                whole, _, la1, d1 = _search(gpu, name, strand, capacity=X.WHOLE)
                assert la1["k_fill_hits"] == 1 and _eq(whole, got) and d1 == dropped, (name, strand, la1)
    finally:
        gpu.table_limit(0)
    if name in X.GOLDEN_CASES:
        gold = X.parse_rows(M.golden(name))
        assert sorted(rows) == sorted(r for r in gold if r[6] in c["strands"])
        assert c["strands"] == ("+", "-") or all(r[6] == "+" for r in gold)    # (a case searched on one strand has nothing on the other)


@pytest.mark.parametrize("name", [n for n, c in X.CASES.items() if c["mask"]])
def test_masked_case_equals_the_statement(gpu, name):
    """the table and the target's bytes change under a prepared table: the searches read the masked table and match codes made
    again, and give what a table built from the masked bytes gives"""
    want = X.statement(lzo, name)["hsps"]
    _prepare(gpu, name)
    before, _, _, _ = _search(gpu, name)
    assert not _eq(before, want)                                            # (the event matters to this search)
    _mask(gpu)
    assert gpu.table_num_words() == int(X.table(lzo, name).pt.contents.words_in_table)
    got, cn, la, dropped = _search(gpu, name)
    _check(gpu, name, "+", got, cn, la, dropped)
    gpu.table_prepare(X.sequences(lzo, name)[0], gpu.seed(X.CASES[name]["pattern"], X.CASES[name]["trans"]), CTB)
    fresh, _, _, d2 = _search(gpu, name)                                    # ... and what a fresh table of the masked bytes gives
    assert _eq(fresh, got) and d2 == dropped
