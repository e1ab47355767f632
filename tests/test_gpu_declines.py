"""The declines the library takes after a search has begun -- LZGPU_NH_HITS_OVERFLOW (3: one query position has more raw
hits than a chunk holds), LZGPU_NH_HSP_OVERFLOW (4: more candidates than lzgpu_set_hsp_capacity's room, counted before
entropy) and LZGPU_NH_SCORE_CLASSES (2) -- on the pair of tests/window_cases.py (tests/test_window_cases.py states on the
CPU what the boundaries are).  A decline produces nothing, and the library is as good as before: with the capacities back
at their defaults the same search gives the oracle's HSPs, order and counters -- the plain search under every scan mode,
the self-comparison and the filtered search, after which a plain search is the plain oracle's (no clip stays behind).
Then one scripted sequence of searches, window searches under another matrix, a limited table and a fenced target in one
process, with the launches of k_build_wctx that the changes of table and target codes call for.  Needs an MI355X."""
import os
import time

import numpy as np
import pytest

from oracle import lzo
from lastz_amd import lzgpu
import window_cases as WC

pytestmark = pytest.mark.gpu
CTB = lzo.upper_nuc_to_bits()


@pytest.fixture()
def lib(gpu):
    """the decline pair's table; every setting a test may change is put back afterwards"""
    gpu.table_prepare(WC.decline_pair()[0], gpu.seed(), CTB)
    try:
        yield gpu
    finally:
        _defaults(gpu)
        gpu.table_limit(0)
        gpu.profile_enable(False)


def _defaults(gpu):
    gpu.set_hit_capacity(WC.HIT_CAPACITY_DEFAULT)
    gpu.set_hsp_capacity(WC.HSP_CAPACITY_DEFAULT)
    gpu.set_scan_mode(0)


def _call(gpu, kind, **kw):
    t, q = WC.decline_pair()
    if kind == "plain":
        return gpu.seed_hit_search(WC.masked(), q=q, **kw)
    if kind == "self":
        return gpu.seed_hit_search_self(WC.masked(), q=t, same_strand=True, **kw)
    return gpu.seed_hit_search_within(WC.masked(), WC.T_IV, WC.Q_IV, q=q, **kw)


def _is_the_oracles(gpu, kind, entropic):
    want, st = WC.oracle_of(kind, entropic=entropic)
    gpu.counters_reset()
    got = _call(gpu, kind, entropic=entropic)
    assert len(got) == len(want) and bool((got == want).all()), (kind, entropic, len(got), len(want))
    cn = gpu.counters()
    assert all(cn[x] == st[x] for x in WC.COUNTERS), (kind, entropic, cn, st)


def _declines(gpu, kind, rc, **kw):
    with pytest.raises(lzgpu.NotHandled) as e:
        _call(gpu, kind, **kw)
    assert e.value.rc == rc, (kind, e.value.rc)


def _launches(gpu, prefix):
    return sum(v["launches"] for k, v in gpu.profile().items() if k.startswith(prefix))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_hit_capacity_boundary(lib, mode):
    """capacity M, the most raw hits of one query position: searched, in many chunks; M - 1: declined, and the search
    after it is the oracle's"""
    M = WC.decline_reach()["M"]
    t0 = time.perf_counter()
    lib.set_scan_mode(mode)
    lib.set_hit_capacity(M)
    lib.profile_enable(True); lib.profile_reset()
    _is_the_oracles(lib, "plain", True)
    assert lib.last_scan_mode() == mode
    chunks = max(v["launches"] for k, v in lib.profile().items() if k.startswith("k_settle"))
    assert chunks >= WC.decline_reach()["over_1024"] >= 16                  # no two positions of more than M / 2 hits share a chunk
    lib.profile_enable(False)
    _is_the_oracles(lib, "plain", False)
    lib.set_hit_capacity(M - 1)
    _declines(lib, "plain", 3)
    _declines(lib, "plain", 3, entropic=False)
    lib.set_hit_capacity(WC.HIT_CAPACITY_DEFAULT)
    for entropic in (True, False):
        _is_the_oracles(lib, "plain", entropic)
    assert lib.last_scan_mode() == mode
    print("\nhit capacity boundary, scan mode %d: %.2f s" % (mode, time.perf_counter() - t0))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_hsp_capacity_boundary(lib, mode):
    """capacity C, the candidates before entropy: searched; C - 1: declined, with entropy too, whose final list is far
    shorter; the search after it is the oracle's"""
    r = WC.decline_reach()
    C = r["C"]
    lib.set_scan_mode(mode)
    lib.set_hsp_capacity(C)
    for entropic in (False, True):
        _is_the_oracles(lib, "plain", entropic)
    lib.set_hsp_capacity(C - 1)
    assert r["hsps"] < C - 1
    _declines(lib, "plain", 4, entropic=False)
    _declines(lib, "plain", 4, entropic=True)
    lib.set_hsp_capacity(WC.HSP_CAPACITY_DEFAULT)
    for entropic in (True, False):
        _is_the_oracles(lib, "plain", entropic)
    assert lib.last_scan_mode() == mode


@pytest.mark.parametrize("kind", ["self", "within"])
def test_declined_self_and_filtered_searches_leave_nothing_behind(lib, kind):
    for setter, value, default, rc in ((lib.set_hit_capacity, 1024, WC.HIT_CAPACITY_DEFAULT, 3),
                                       (lib.set_hsp_capacity, 16, WC.HSP_CAPACITY_DEFAULT, 4)):
        setter(value)
        _declines(lib, kind, rc)
        _declines(lib, "plain", rc)
        _declines(lib, kind, rc, entropic=False)
        setter(default)
        _is_the_oracles(lib, "plain", True)                                 # no clip of the declined search stays behind
        for entropic in (True, False):
            _is_the_oracles(lib, kind, entropic)
        setter(value)
        _declines(lib, kind, rc)
        setter(default)
        _is_the_oracles(lib, "plain", False)


def test_too_many_score_classes(lib):
    t, q = WC.decline_pair()
    many = WC.many_classes()
    isd = lib.seed(WC.INNER, 0)
    for _ in range(2):
        with pytest.raises(lzgpu.NotHandled) as e:
            lib.seed_hit_search(many, q=q)
        assert e.value.rc == 2
        _is_the_oracles(lib, "plain", True)
        with pytest.raises(lzgpu.NotHandled) as e:
            lib.window_search(many, WC.SCRIPT_WINDOWS, isd, CTB, q=q, hsp_threshold=WC.SCRIPT_THR)
        assert e.value.rc == 2
        got = lib.window_search(WC.masked(), WC.SCRIPT_WINDOWS, isd, CTB, q=q, hsp_threshold=WC.SCRIPT_THR)
        assert WC.differs(got, [WC.want(w, WC.SCRIPT_THR, seqs=(t, q)) for w in WC.SCRIPT_WINDOWS]) is None
        _is_the_oracles(lib, "plain", False)


def test_a_scripted_sequence_in_one_process(lib):
    """search, window search under `eight`, search, table limit, search, window search, two fences, filtered search, fences
    away, (one more search,) limit lifted, search: the oracle's at every step; k_build_wctx runs on the first fused search
    and on the fused search after the table (limit set, limit lifted) or the target's codes (a patch) changed, on no
    other.  The search of the fenced target is not fused (its NUL bytes take scan mode 1), so the search added after the
    fences' removal is the one that shows the patch's account."""
    t, q = WC.decline_pair()
    o = WC.script_oracle()
    m, eight, isd = WC.masked(), WC.eight(), lib.seed(WC.INNER, 0)
    fused = os.environ.get("LZGPU_FUSED_SCAN") != "0"
    at = np.flatnonzero(o["fenced"] != t)
    assert len(at) == 2
    built = []

    def search(want, within=None, mode0=True):
        hs, st = want
        lib.counters_reset(); lib.profile_reset()
        got = lib.seed_hit_search(m, q=q) if within is None else lib.seed_hit_search_within(m, within[0], within[1], q=q)
        assert len(got) == len(hs) and bool((got == hs).all()), (len(built), len(got), len(hs))
        cn = lib.counters()
        assert all(cn[x] == st[x] for x in WC.COUNTERS), (len(built), cn, st)
        assert (lib.last_scan_mode() == 0) == mode0, (len(built), lib.last_scan_mode())
        built.append(_launches(lib, "k_build_wctx"))

    def windows():
        lib.profile_reset()
        got = lib.window_search(eight, WC.SCRIPT_WINDOWS, isd, CTB, q=q, hsp_threshold=WC.SCRIPT_THR)
        assert WC.differs(got, o["windows"]) is None
        assert _launches(lib, "k_build_wctx") == 0 and _launches(lib, "k_window_search") >= 1

    lib.table_prepare(t, lib.seed(), CTB)                                   # a new table: nothing is built for it yet
    lib.profile_enable(True)
    patched = False
    try:
        search(o["plain"])                                                  # 1
        windows()                                                           # 2
        search(o["plain"])                                                  # 3
        lib.table_limit(WC.SCRIPT_LIMIT)                                    # 4
        search(o["limited"])                                                # 5
        windows()                                                           # 6
        lib.target_patch(at, o["fenced"][at]); patched = True               # 7
        search(o["within"], within=(o["t_iv"], o["q_iv"]), mode0=False)     # 8 (the fences are special bytes: masks, not fused)
        lib.target_patch(at, t[at]); patched = False                        # 9
        search(o["limited"])                                                # (between 9 and 10: fused again, on the patched codes' account)
        lib.table_limit(0)                                                  # 10
        search(o["plain"])                                                  # 11
    finally:
        if patched:
            lib.target_patch(at, t[at])
        lib.table_limit(0)
        lib.profile_enable(False)
    assert built == ([1, 0, 1, 0, 1, 1] if fused else [0] * 6), built
