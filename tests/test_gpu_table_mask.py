"""Dynamic masking on the device (lastz --masking): lzgpu_table_mask and lzgpu_target_update over the cases of
tests/table_mask_cases.py, against the oracle's table BUILT from the masked bytes (table_mask_cases.py says why that is the
expected value; tests/test_emul_table_mask.py pins the same statement on the CPU)."""
import numpy as np
import pytest

from oracle import lzo
from lastz_amd import lzgpu
import helpers as H
import table_mask_cases as TM

pytestmark = pytest.mark.gpu
CTB = lzo.upper_nuc_to_bits()


def _prepare(gpu, name, t):
    g = TM.geometry(name)
    gpu.table_prepare(t, gpu.seed(g["pattern"], g["trans"]), CTB, step=g["step"], start=g["start"], end=g["end"])


def _arrays(tab):
    pt = tab.pt.contents
    return (np.ctypeslib.as_array(pt.last, shape=(int(pt.word_entries),)), np.ctypeslib.as_array(pt.prev, shape=(int(pt.prev_entries),)))


def _lists(last, prev, adj, step):
    """the exported last[] / prev[] as CSR lists of end positions (src/pos_table.h:126-167)"""
    ws, wp = np.zeros(len(last) + 1, dtype=np.uint32), []
    for w in np.flatnonzero((last != 0) & (last != 0xFFFFFFFF)):
        ws[w + 1] = len(wp)
        ix = int(last[w])
        while ix != 0xFFFFFFFF:
            wp.append(adj + step * ix)
            ix = int(prev[ix])
        ws[w + 1] = len(wp) - ws[w + 1]
    return np.cumsum(ws, dtype=np.uint64).astype(np.uint32), np.array(wp, dtype=np.uint32)


def _mask_event(gpu, t_masked, widened, cores):
    """what the binding does for one (query, strand): the 'x' bytes of the widened intervals, then one table_mask"""
    for s, e in widened:
        if cores:
            gpu.target_update(s, t_masked[s:e])
    gpu.table_mask(widened)


def _run_events(gpu, name):
    _prepare(gpu, name, TM.target(name))
    for (widened, cores), (t_masked, _) in zip(TM.events(lzo, name), TM.expected(lzo, name)):
        _mask_event(gpu, t_masked, widened, cores)


@pytest.mark.parametrize("name", list(TM.CASES))
def test_masked_table_is_the_table_of_the_masked_bytes(gpu, name):
    g = TM.geometry(name)
    adj = g["start"] - g["start"] % g["step"]
    _prepare(gpu, name, TM.target(name))
    exports = []
    for (widened, cores), (t_masked, tab) in zip(TM.events(lzo, name), TM.expected(lzo, name)):
        _mask_event(gpu, t_masked, widened, cores)
        pt = tab.pt.contents
        want_last, want_prev = _arrays(tab)
        last, prev = gpu.table_export(int(pt.prev_entries))
        print("\n%s: %d entries stay" % (name, gpu.table_num_words()))
        assert gpu.table_num_words() == int(pt.words_in_table) == int(gpu.table_geom().num_words)
        assert (last == want_last).all() and (prev == want_prev).all()
        ws, wp = tab.csr()
        gws, gwp = _lists(last, prev, adj, g["step"])
        assert len(gwp) == len(wp) and (gws == ws).all() and (gwp == wp).all()
        exports.append((last, prev))
    _prepare(gpu, name, TM.expected(lzo, name)[-1][0])           # ... and a fresh table of the masked bytes exports the same
    last, prev = gpu.table_export(len(exports[-1][1]))
    assert (last == exports[-1][0]).all() and (prev == exports[-1][1]).all()


@pytest.mark.parametrize("name", TM.SEARCHED)
def test_searches_see_the_masked_table_and_target(gpu, name):
    """the target's codes follow the masking.  (These targets hold N, lower case and 'x', so the searches run scan modes 1 / 2;
    the fused kernel and wctx have test_fused_scan_follows_the_masking.)"""
    _, masked = H.scoring()
    _run_events(gpu, name)
    t_masked, tab = TM.expected(lzo, name)[-1]
    found = 0
    for rev in (False, True):
        q = TM.query(name, rev)
        want, _ = lzo.seed_hit_search(tab, q, masked)
        got = gpu.seed_hit_search(masked, q=q)
        assert len(got) == len(want) and (got == want).all(), (name, rev)
        found += len(want)
    assert found > 0
    unmasked, _ = lzo.seed_hit_search(TM.table(lzo, name, TM.target(name)), TM.query(name), masked)
    want, _ = lzo.seed_hit_search(tab, TM.query(name), masked)
    assert name == "list_ends" or len(unmasked) != len(want) or (unmasked != want).any()    # (the masking matters to the search)


def test_gapped_stage_sees_the_masked_target(gpu):
    """anchors next to a masked run: the DP encodings are made again"""
    sub, masked = H.scoring()
    _run_events(gpu, "two_events")
    t_masked, tab = TM.expected(lzo, "two_events")[-1]
    q = TM.query("two_events")
    hsps, _ = lzo.seed_hit_search(tab, q, masked)
    assert len(hsps) > 0
    segs = lzo.hsps_to_segments(hsps, 0)
    want_al, want_ops, _ = lzo.gapped_extend(t_masked, q, sub, lzo.reduce_to_points(t_masked, q, sub, segs))
    plain_al, _, _ = lzo.gapped_extend(TM.target("two_events"), q, sub, lzo.reduce_to_points(TM.target("two_events"), q, sub, segs))
    assert len(want_al) > 0 and (len(plain_al) != len(want_al) or (plain_al != want_al).any())   # the 'x' run changes the alignments
    al, ops = gpu.gapped_extend(sub, segs.view(lzgpu.SEG_DTYPE), q=q)
    assert len(al) == len(want_al) and (al == want_al.view(lzgpu.ALIGN_DTYPE)).all() and (ops == want_ops).all()


def test_exact_search_sees_the_masked_target(gpu):
    """the match codes are made again"""
    name = "two_events"
    mb = lzo.upper_nuc_to_bits().copy()
    mb[[ord(c) for c in "acgt"]] = mb[[ord(c) for c in "ACGT"]]
    q = TM.target(name)[7000:9000].copy()
    _prepare(gpu, name, TM.target(name))
    before = gpu.seed_hit_search_exact(mb, 40, q=q)
    for (widened, cores), (t_masked, _) in zip(TM.events(lzo, name), TM.expected(lzo, name)):
        _mask_event(gpu, t_masked, widened, cores)
    got = gpu.seed_hit_search_exact(mb, 40, q=q)
    _prepare(gpu, name, TM.expected(lzo, name)[-1][0])
    want = gpu.seed_hit_search_exact(mb, 40, q=q)
    assert len(want) > 0 and len(got) == len(want) and (got == want).all()
    assert len(before) != len(want) or (before != want).any()


def test_contract(gpu):
    name = "overlap"
    g = TM.geometry(name)
    widened = TM.events(lzo, name)[0][0]
    _prepare(gpu, name, TM.target(name))
    n0 = gpu.table_num_words()
    pe = 1 + g["tlen"]
    last0, prev0 = gpu.table_export(pe)
    gpu.table_mask([])                                          # n == 0
    gpu.table_mask([(100, 110), (0, 18)])                       # shorter than L: nothing goes
    assert gpu.table_num_words() == n0
    for bad in ([(10, 10)], [(20, 10)], [(0, g["tlen"] + 1)], widened + [(5, 5)]):
        with pytest.raises(lzgpu.LzGpuError):
            gpu.table_mask(bad)
    with pytest.raises(lzgpu.LzGpuError):
        gpu.target_update(g["tlen"] - 3, np.zeros(4, dtype=np.uint8))
    with pytest.raises(lzgpu.LzGpuError):
        gpu.target_update(g["tlen"] + 1, np.zeros(0, dtype=np.uint8))
    gpu.target_update(g["tlen"], np.zeros(0, dtype=np.uint8))
    gpu.table_limit(7)
    try:
        with pytest.raises(lzgpu.NotHandled):
            gpu.table_mask(widened)
    finally:
        gpu.table_limit(0)
    last, prev = gpu.table_export(pe)
    assert gpu.table_num_words() == n0 and (last == last0).all() and (prev == prev0).all()
    gpu.table_mask(widened)                                     # and without the limit it is taken
    assert gpu.table_num_words() == int(TM.expected(lzo, name)[0][1].pt.contents.words_in_table) < n0


def _profiled(gpu, search):
    """-> (the search's HSPs, the kernels it launched, by the library's timer)"""
    gpu.profile_reset(); gpu.profile_enable(True)
    try:
        got = search()
        assert gpu.last_scan_mode() == 0
        return got, {k: v["launches"] for k, v in gpu.profile().items() if v["launches"]}
    finally:
        gpu.profile_enable(False)


def test_fused_scan_follows_the_masking(gpu):
    """Scan mode 0 (the fused kernel) reads wctx, the copy of the target's codes beside every table entry.  The case tables' targets
    hold N, lower case and, once masked, 'x': their searches run modes 1 / 2 and read no wctx.  Here the target is upper-case
    A, C, G, T only and stays so: a table_mask without bytes, then a table_mask and a target_update with other bases.  After each, a mode-0 search
    must build wctx again (the kernel timer shows it) and give what the two-kernel scan of mode 1, which reads no wctx, gives."""
    _, masked = H.scoring()
    rng = np.random.default_rng(77)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    t = acgt[rng.integers(0, 4, 40000)].copy()
    q = acgt[rng.integers(0, 4, 6000)].copy()
    for k, at in enumerate((7000, 12000, 20000)):                # three blocks of the target in the query
        q[500 + 2000 * k: 1100 + 2000 * k] = t[at: at + 600]
    search = lambda: gpu.seed_hit_search(masked, q=q)           # noqa: E731

    def two_kernel():
        gpu.set_scan_mode(1)
        try:
            got = search()
            assert gpu.last_scan_mode() == 1
            return got
        finally:
            gpu.set_scan_mode(0)

    gpu.table_prepare(t, gpu.seed(), CTB)
    before, ran = _profiled(gpu, search)
    want, _ = lzo.seed_hit_search(lzo.Table(t, lzo.seed()), q, masked)
    assert ran.get("k_build_wctx") == 1 and "k_fill_hits" not in ran, ran      # the fused path
    assert len(before) == 3 and (before == want).all()
    again, ran = _profiled(gpu, search)
    assert "k_build_wctx" not in ran and (again == before).all(), ran           # (wctx is kept while nothing changes)

    gpu.table_mask([(6900, 7700)])                              # the first block's seeds go; no byte changes
    after, ran = _profiled(gpu, search)
    assert ran.get("k_build_wctx") == 1 and "k_fill_hits" not in ran, ran
    assert len(after) == 2 and (after == before[(before["pos1"] < 6900) | (before["pos1"] > 7700)]).all()
    assert (after == two_kernel()).all()

    # the second block: 100 of its bases lose their seeds, then every 7th of them becomes another base, still A, C, G, T --
    # an event whose bytes are not special.  The update alone changes no table entry and leaves the codes' key as it was.
    gpu.table_mask([TM.widen(12200, 12300, 19, len(t))])
    cut, ran = _profiled(gpu, search)
    assert ran.get("k_build_wctx") == 1 and len(cut) == 2, ran                      # (the block's other seeds still find it)
    t2 = t.copy()
    t2[12200:12300:7] = acgt[(np.searchsorted(acgt, t2[12200:12300:7]) + 1) % 4]
    gpu.target_update(12200, t2[12200:12300])
    changed, ran = _profiled(gpu, search)
    assert ran.get("k_build_wctx") == 1 and "k_fill_hits" not in ran, ran
    ref = two_kernel()
    assert len(changed) == len(ref) and (changed == ref).all()
    assert len(changed) != len(cut) or (changed != cut).any()
