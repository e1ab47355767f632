"""The seed stage under the seed shapes of tests/seed_shape_cases.py, against the oracle (pinned for these shapes against
the pristine binary by tests/test_seed_shapes_oracle.py): 28-bit seeds (14of22, match14: the 29-bit table sort, 2^28 + 1
bounds, a 1 GiB last[]), 106 / 92 / 67 probes (seven probe rounds of 16, the last one partial), length 31 with seed hits
on the first and the last base of both sequences, 6 parts, 4- to 8-bit seeds whose every list is long (a wave's lists are
taken in pieces of LZ_F2_CAP hits, several chunks), a pattern with zeros to trim.

Per case: lzgpu_table_num_words and the exported last[] / prev[] equal the oracle's table (of the 28-bit seeds only
s14of22 and match14 export), HSPs, order and counters equal the oracle's on both strands, raw hits (extend=False) where
the case names them.  In process, and in two fresh child processes, fused scan path (LZGPU_FUSED_SCAN unset) and split
(=0), each under its own time limit; the first child that fails ends the series -- nothing more is started on the GPU after
a fault.  The children's arrays are compared with the oracle's, not with each other.

Further: heavy_blocks (fewer block bits than wanted: more chunks than blocks), self search, position filter and word-count
limit under 14of22, the window search with a spaced 14-bit seed and a 5-mer and its declines, and tables of seeds of
different weight in one process through save / load / export.  Needs an MI355X."""
import time

import numpy as np
import pytest

from oracle import lzo
from lastz_amd import lzgpu, seqio
import helpers as H
import seed_shape_cases as SC
import self_cases as S
import pos_filter_cases as P
import word_limit_cases as W

pytestmark = pytest.mark.gpu
CTB = lzo.upper_nuc_to_bits()
RUNS = [("fused", {}), ("split", {"LZGPU_FUSED_SCAN": "0"})]
PAIRS = [(key, name) for key, _ in RUNS for name in SC.CASES]


def _masked():
    return H.scoring()[1]


def _eq(got, want):
    return len(got) == len(want) and bool((got == want).all())


def _table_is(gpu, tab, export=True):
    pt = tab.pt.contents
    assert gpu.table_num_words() == pt.words_in_table
    if export:
        last, prev = gpu.table_export(int(pt.prev_entries))
        assert (last == np.ctypeslib.as_array(pt.last, shape=(int(pt.word_entries),))).all()
        assert (prev == np.ctypeslib.as_array(pt.prev, shape=(int(pt.prev_entries),))).all()


def _search_is(gpu, name, extend=True):
    c = SC.CASES[name]
    hs, sts = SC.oracle_search(lzo, name, _masked(), extend=extend)
    for k, q in enumerate(SC.queries(name)):
        gpu.counters_reset()
        got = gpu.seed_hit_search(_masked(), q=q, hsp_threshold=c["thr"], extend=extend)
        assert _eq(got, hs[k]), (name, k, extend, len(got), len(hs[k]))
        cn = gpu.counters()
        for x in SC.COUNTERS if extend else ("words", "raw_hits"):
            assert cn[x] == sts[k][x], (name, k, extend, x)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_table_and_search_equal_the_oracle(gpu, name):
    c = SC.CASES[name]
    t0 = time.perf_counter()
    gpu.set_hit_capacity(c["capacity"] or SC.WHOLE)
    try:
        gpu.table_prepare(SC.sequences(c["seq"])[0], gpu.seed(c["pattern"], c["trans"]), CTB, step=c["step"])
        _table_is(gpu, SC.table(lzo, name), export=c["export"])
        _search_is(gpu, name)
        if c["plain"]:
            _search_is(gpu, name, extend=False)
        if c["twin"]:                                                       # the untrimmed pattern's table and results
            gpu.table_prepare(SC.sequences(c["seq"])[0], gpu.seed(c["twin"], c["trans"]), CTB, step=c["step"])
            _table_is(gpu, SC.table(lzo, name))
            _search_is(gpu, name)
    finally:
        gpu.set_hit_capacity(SC.WHOLE)
    print("\n%s: %.2f s with the oracle's share" % (name, time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------- fresh processes, both scan paths

@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    out = H.run_gpu_children(tmp_path_factory.mktemp("seed_shapes"),
                             [(key, "seed_shape_cases", list(SC.CASES), env, 300, None) for key, env in RUNS])
    for key, _ in RUNS:
        print("\nseed shapes child %s" % key)
        for name in SC.CASES:
            for m in out[key][1][name]:
                print("  %-12s extend %-5s words %-7d modes %s  %6.3f s  %s" % (name, m["extend"], m["num_words"], m["scan_modes"], m["seconds"],
                      " ".join("%s=%d" % kv for kv in sorted(m["launches"].items()))))
    return out


@pytest.mark.parametrize("key,name", PAIRS)
def test_children_equal_the_oracle(runs, key, name):
    z, meta = runs[key]
    c = SC.CASES[name]
    assert [m["extend"] for m in meta[name]] == ([True, False] if c["plain"] else [True])
    for r, m in enumerate(meta[name]):
        hs, sts = SC.oracle_search(lzo, name, _masked(), extend=m["extend"])
        assert m["num_words"] == SC.table(lzo, name).pt.contents.words_in_table
        for k in range(2):
            assert _eq(z["%s/%d/%d" % (name, r, k)], hs[k]), (key, name, m["extend"], k)
        tot = SC.summed(sts)
        for x in SC.COUNTERS if m["extend"] else ("words", "raw_hits"):
            assert m["counters"][x] == tot[x], (key, name, m["extend"], x)
        la = m["launches"]
        if m["extend"]:                                                     # the path the child was started for
            assert (la.get("k_fill_hits", 0) == 0) == (key == "fused"), (key, name, la)
        if c["capacity"]:                                                   # several chunks
            assert la.get("k_settle2", 0) >= 3 or not m["extend"], (key, name, la)


# ---------------------------------------------------------------------------------------- further kernels under a heavy seed

def test_heavy_blocks(gpu):
    """s14of22_t2 on 300 kbp at hit capacity 2048: the 32-bit sort key has room for 3 block bits where the search wants 5,
    so there are more chunks than blocks (seed_shape_cases.heavy_reaches states it on the CPU)"""
    c = SC.CASES[SC.HEAVY["case"]]
    t, q = SC.sequences(SC.HEAVY["seq"])
    tab, hs, sts = SC.heavy_search(lzo, _masked())
    assert SC.heavy_reaches(lzo, _masked()) is None
    gpu.table_prepare(t, gpu.seed(c["pattern"], c["trans"]), CTB)
    assert gpu.table_num_words() == tab.pt.contents.words_in_table
    gpu.profile_enable(True)
    try:
        for k, qq in enumerate((q, seqio.revcomp(q))):
            gpu.set_hit_capacity(SC.HEAVY["capacity"])
            gpu.profile_reset(); gpu.counters_reset()
            got = gpu.seed_hit_search(_masked(), q=qq)
            cn, la = gpu.counters(), {n: v["launches"] for n, v in gpu.profile().items()}
            gpu.set_hit_capacity(SC.WHOLE)
            whole = gpu.seed_hit_search(_masked(), q=qq)
            assert _eq(got, hs[k]) and _eq(whole, hs[k]), k
            assert all(cn[x] == sts[k][x] for x in SC.COUNTERS), (cn, sts[k])
            print("\nheavy_blocks strand %d: %s" % (k, " ".join("%s=%d" % kv for kv in sorted(la.items()))))
            assert la.get("k_settle2", 0) > 8, la                           # more chunks than the 8 blocks
    finally:
        gpu.set_hit_capacity(SC.WHOLE); gpu.profile_enable(False)


@pytest.mark.parametrize("name", ["seed_t2", "multi_ragged"])
def test_self_search_under_a_heavy_seed(gpu, name):
    """lzgpu_seed_hit_search_self with 14of22 and two transitions, same and opposite strand: the 106 probes go through
    k_count_sorted_self's and k_fill_hits2<true>'s groups of 16"""
    v, seps, _ = S.sequence(name)
    sd = lzo.seed(SC.S14OF22, 2)
    tab = lzo.Table(v, sd)
    gpu.table_prepare(v, gpu.seed(SC.S14OF22, 2), CTB)
    raw = 0
    for same in (True, False):
        q = v if same else S.minus(v, seps)
        want, st = lzo.seed_hit_search(tab, q, _masked(), self_strand="same" if same else "opposite", sep1=seps or None, sep2=seps or None)
        gpu.counters_reset()
        got = gpu.seed_hit_search_self(_masked(), q=q, same_strand=same, sep1=seps or None, sep2=seps or None)
        assert _eq(got, want), (name, same, len(got), len(want))
        cn = gpu.counters()
        assert all(cn[x] == st[x] for x in SC.COUNTERS), (name, same, cn, st)
        raw += st["raw_hits"]
        assert len(want) > 0
    assert raw > 1000


def test_position_filter_under_a_heavy_seed(gpu):
    """lzgpu_seed_hit_search_within as tests/pos_filter_cases.py states it (the table of the words inside the target
    interval, over the intersected query interval), on its case probes_79 with 14of22 and two transitions"""
    c = dict(P.CASES["probes_79"], pattern=SC.S14OF22, trans=2)
    t, qs = P.queries("probes_79")
    sd = lzo.seed(c["pattern"], c["trans"])
    (ts, te), (q0, q1) = P.intersect(c, len(t), len(qs[0]), sd.length)
    tab = lzo.Table(t, sd, start=ts, end=te)
    gpu.table_prepare(t, gpu.seed(c["pattern"], c["trans"]), CTB)
    raw = 0
    for q in qs:
        want, st = lzo.seed_hit_search(tab, q, _masked(), start=q0, end=q1)
        gpu.counters_reset()
        got = gpu.seed_hit_search_within(_masked(), c["t_iv"], c["q_iv"], q=q)
        assert _eq(got, want), (len(got), len(want))
        cn = gpu.counters()
        assert all(cn[x] == st[x] for x in SC.COUNTERS), (cn, st)
        raw += st["raw_hits"]
    assert raw > 0


def test_word_count_limit_under_a_heavy_seed(gpu):
    """lzgpu_table_limit / lzgpu_table_find_limit over 2^28 words: rep20's 14of22 table (lists of 1 to 40 and more entries)
    against tests/word_limit_cases.py's statement on the oracle's table, searched with the probe cut out of its repeats"""
    t, q = W.seq("rep20"), W.seq("probe")
    sd = lzo.seed(SC.S14OF22, 1)
    tab = lzo.Table(t, sd)
    n = W.list_lengths(tab)
    lims = [1, 7, 39, 47, int(n.max()) + 1]                                 # between the lists of rep20's repeats (1, 2, 6-8, 39, 47, 189-279 entries)
    pt = tab.pt.contents                                                    # one oracle table for all limits: what limited() zeroes is put back
    last, some = np.ctypeslib.as_array(pt.last, shape=(int(pt.word_entries),)), np.flatnonzero(n)
    unlimited = last[some].copy()
    assert all((n == c).any() for c in (1, 7, 39, 47)) and int(n.max()) > 47
    gpu.table_prepare(t, gpu.seed(SC.S14OF22, 1), CTB)
    full = gpu.table_num_words()
    assert full == int(n.sum())
    dist = (lambda c, w: (c.astype(np.int64), w.astype(np.int64)))(*np.unique(n[n > 0], return_counts=True))
    count, words = gpu.table_count_distribution()
    assert (count == dist[0]).all() and (words == dist[1]).all()
    keeps = [W.keep_of(p) for p in W.GOLDEN_PERCENTS] + [0.999, 0.25, 0.97]
    want = [W.find_limit(None, k, dist) for k in keeps]
    assert [gpu.table_find_limit(k) for k in keeps] == want and len(set(want)) >= 2
    raws = set()
    try:
        for lim in lims + [0]:
            last[some], kept = unlimited, int(n.sum())
            pt.words_in_table = kept
            if lim:
                _, kept = W.limited(tab, lim, own=n)
            gpu.table_limit(lim)
            assert gpu.table_num_words() == kept, lim
            for qq in (q, seqio.revcomp(q)):
                hs, st = lzo.seed_hit_search(tab, qq, _masked())
                gpu.counters_reset()
                assert _eq(gpu.seed_hit_search(_masked(), q=qq), hs), lim
                cn = gpu.counters()
                assert all(cn[x] == st[x] for x in SC.COUNTERS), (lim, cn, st)
                raws.add(st["raw_hits"])
    finally:
        gpu.table_limit(0)
    assert len(raws) >= 6                                                   # every limit lets more hits in, on either strand


# ---------------------------------------------------------------------------------------- the window search's inner seeds

def _windows(t, q):
    """rectangles around twelve of the whole pair's HSPs (the pair's homologous blocks lie anywhere), with margins of 0 to
    3000 bases; the two ends of the sequences; a target piece shorter than any seed"""
    hs, _ = lzo.seed_hit_search(lzo.Table(t, lzo.seed()), q, _masked())
    rng = np.random.default_rng(12)
    wins = [(0, 20000, 0, 20000), (len(t) - 20480, 20480, len(q) - 20480, 20480), (40000, 3, 40000, 5000)]
    for h in hs[np.linspace(0, len(hs) - 1, 12).astype(int)]:
        m = rng.integers(0, 3000, 4)
        n = min(int(h["length"]), 14000)
        t0, q0 = max(0, int(h["pos1"]) - n - int(m[0])), max(0, int(h["pos2"]) - n - int(m[1]))
        wins.append((t0, min(len(t), int(h["pos1"]) + int(m[2])) - t0, q0, min(len(q), int(h["pos2"]) + int(m[3])) - q0))
    assert len(hs) >= 12 and all(tl <= 20480 and ql <= 20480 for _, tl, _, ql in wins)
    return wins


@pytest.mark.parametrize("pattern,thr", [("11010100111", 2200), ("11111", 3000)])
def test_window_search_with_other_inner_seeds(gpu, pattern, thr):
    """lzgpu_window_search with a spaced 14-bit seed and with a 5-mer (1024 words: 256 query positions have more hits than
    the kernel's buffer holds) on a few rectangles, each against the oracle run on the cut-out pieces"""
    t, q = H.load_case("synth200k")
    gpu.table_prepare(t, gpu.seed(), CTB)
    wins = _windows(t, q)
    isd, osd = gpu.seed(pattern, 0), lzo.seed(pattern, 0)
    got = gpu.window_search(_masked(), wins, isd, CTB, q=q, hsp_threshold=thr)
    total = 0
    for (t0, tl, q0, ql), g in zip(wins, got):
        want = np.zeros(0, dtype=lzgpu.HSP_DTYPE)
        if tl >= osd.length and ql >= osd.length:
            want, _ = lzo.seed_hit_search(lzo.Table(t[t0:t0 + tl], osd), q[q0:q0 + ql], _masked(), hsp_threshold=thr, entropic=False)
        assert _eq(g, want), (pattern, t0, tl, q0, ql, len(g), len(want))
        total += len(g)
    assert total > 20


def test_window_search_declines_heavier_seeds_and_transitions(gpu):
    t, q = H.load_case("synth200k")
    gpu.table_prepare(t, gpu.seed(), CTB)
    wins = _windows(t, q)[3:5]
    for pattern, trans in (("11111111", 0), ("1111111", 1), ("11010100111", 2)):
        with pytest.raises(lzgpu.NotHandled) as e:
            gpu.window_search(_masked(), wins, gpu.seed(pattern, trans), CTB, q=q)
        assert e.value.rc == 7                                              # LZGPU_NH_UNSUPPORTED
    isd, osd = gpu.seed("1111111", 0), lzo.seed("1111111", 0)               # and the library stays usable
    (t0, tl, q0, ql), g = wins[0], gpu.window_search(_masked(), wins[:1], isd, CTB, q=q)[0]
    want, _ = lzo.seed_hit_search(lzo.Table(t[t0:t0 + tl], osd), q[q0:q0 + ql], _masked(), entropic=False)
    assert _eq(g, want) and len(want) > 0


# ---------------------------------------------------------------------------------------- declines, and seeds of different weight

def test_a_one_base_word_is_declined_by_table_prepare(gpu):
    t, _ = SC.sequences("cut")
    for pattern, trans in SC.DECLINED_TABLES:
        with pytest.raises(lzgpu.NotHandled) as e:
            gpu.table_prepare(t, gpu.seed(pattern, trans), CTB)
        assert e.value.rc == 1                                              # LZGPU_NH_SEED
    for pattern, trans in SC.DECLINED_SEEDS:
        with pytest.raises(lzgpu.NotHandled):
            gpu.seed(pattern, trans)
    gpu.table_prepare(t, gpu.seed("1111", 1), CTB)                          # the library stays usable
    gpu.set_hit_capacity(50_000)
    try:
        _search_is(gpu, "light4_t1")
    finally:
        gpu.set_hit_capacity(SC.WHOLE)


@pytest.mark.parametrize("restart", [False, True], ids=["same-context", "shutdown-init"])
def test_seeds_of_different_weight_in_one_process(gpu, tmp_path, restart):
    """match14's table saved, an 8-mer's table prepared and searched, the file loaded: export and search are match14's
    (the binding sizes last[] by the resident table's geometry, not by the last seed prepared)"""
    t, q = SC.sequences("pair")
    f = tmp_path / "match14.lztab"
    gpu.table_prepare(t, gpu.seed("1" * 14, 0), CTB)
    gpu.table_save(f)
    light = lzo.Table(t, lzo.seed("11111111", 0))
    gpu.table_prepare(t, gpu.seed("11111111", 0), CTB)
    _table_is(gpu, light)
    want, _ = lzo.seed_hit_search(light, q, _masked())
    assert _eq(gpu.seed_hit_search(_masked(), q=q), want) and len(want) > 0
    if restart:
        gpu.shutdown(); gpu.init()
    gpu.table_load(f)
    assert gpu.table_geom().seed.weight_bits == 28
    _table_is(gpu, SC.table(lzo, "match14"))
    _search_is(gpu, "match14")
