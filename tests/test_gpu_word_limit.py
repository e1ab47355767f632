"""lzgpu_table_limit / lzgpu_table_find_limit (lastz --maxwordcount) against the oracle's search of a table limited from
outside (tests/word_limit_cases.py: limited(), find_limit(); pinned against the pristine binary by
tests/test_word_limit_oracle.py), on 10-40 kbp sequences with planted repeats:

  rep against itself and rep20 against rep under the limits c and c - 1 for the distinct list lengths c of the table, 1,
  and one above the longest list (= the unlimited search),
  the plain-hit processor (the rows list the limited table entry by entry, in list order),
  a 14-bit seed whose lists are nearly all longer than 1, a stepped table of a 12-of-12 seed, a table built on an interval,
  special bytes in the target (scan mode 1), hit capacity 4096 (a limited search of several chunks),
  a target of poly-A and AC runs only, from which limit 1 removes everything,
  a self-comparison and a position-filtered search on a limited table.

Per case, limit and strand the HSP arrays equal the oracle's, the five counters its sums and lzgpu_table_num_words() its
kept count; the last run of every case lifts the limit and must be the unlimited search.

The cases run in two child processes one after the other, LZGPU_FUSED_SCAN=1 (all cases) and =0 (seven of them): the
fused kernel reads wctx, which is rebuilt for the limited table.  Each child has its own time limit; the first that fails
ends the series -- nothing more is started on the GPU after a fault.  lzgpu_table_find_limit, what export / save keep
describing, what ends a limit and the state errors are checked in process.  Needs an MI355X."""
import numpy as np
import pytest

from oracle import lzo
from lastz_amd import lzgpu
import helpers as H
import word_limit_cases as W

pytestmark = pytest.mark.gpu
CTB = lzo.upper_nuc_to_bits()
RUNS = [("fused", list(W.CASES), "1"),
        ("split", W.SPLIT_CASES, "0")]
PAIRS = [(key, name) for key, cases, _ in RUNS for name in cases]


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    out = H.run_gpu_children(tmp_path_factory.mktemp("word_limit"),
                             [(key, "word_limit_cases", cases, {"LZGPU_FUSED_SCAN": fused}, 300, None) for key, cases, fused in RUNS])
    for key, cases, _ in RUNS:
        print("\nword limit child %s" % key)
        for name in cases:
            for m in out[key][1][name]:
                print("  %-10s limit %-4d words %-6d modes %s  %6.3f s  %s" % (name, m["limit"], m["num_words"], m["scan_modes"], m["seconds"],
                      " ".join("%s=%d" % kv for kv in sorted(m["launches"].items()))))
    return out


_oracle = {}


def oracle(name, limit):
    """one search of the oracle per case and limit, shared by the two children's tests"""
    if (name, limit) not in _oracle:
        _, masked = H.scoring()
        _oracle[name, limit] = W.oracle_search(lzo, name, masked, limit)
    return _oracle[name, limit]


@pytest.mark.parametrize("key,name", PAIRS)
def test_hsps_counters_and_word_counts_equal_the_oracle(runs, key, name):
    z, meta = runs[key]
    c = W.CASES[name]
    lims = W.limits(lzo, name) + [0]
    assert [m["limit"] for m in meta[name]] == lims
    unlimited = oracle(name, 0)
    for r, (m, lim) in enumerate(zip(meta[name], lims)):
        want, tot, kept = oracle(name, lim)
        assert m["num_words"] == kept, (key, name, lim)
        for k in range(2):
            got = z["%s/%d/%d" % (name, r, k)]
            assert len(got) == len(want[k]) and (got == want[k]).all(), (key, name, lim, k)
        for x in ("words", "raw_hits") if not c["extend"] else W.COUNTERS:
            assert m["counters"][x] == tot[x], (key, name, lim, x)
        if lim > int(W.lengths(lzo, name).max()):                           # above the longest list: nothing goes
            assert kept == unlimited[2] and tot == unlimited[1]
    assert unlimited[1]["raw_hits"] > 0


def test_the_cases_limit_what_they_say():
    """the expectations themselves: every list length is met from both sides, the limits bite, the empty table is empty"""
    for name in ("rep_rep", "rep20_rep"):
        n = W.lengths(lzo, name)
        lims = W.limits(lzo, name)
        distinct = sorted(set(n[n > 1].tolist()))
        assert len(distinct) >= 5 and 1 in lims and max(lims) > distinct[-1] and len(lims) <= 14
        assert sum(1 for c in distinct if c in lims and (c - 1) in lims) >= 4
        raw = [oracle(name, lim)[1]["raw_hits"] for lim in sorted(lims)]
        assert raw == sorted(raw) and len(set(raw)) >= 4                    # a higher limit lets more hits in
    assert (W.lengths(lzo, "seed_7") > 1).sum() > (W.lengths(lzo, "seed_7") == 1).sum() // 2
    assert oracle("empty", 1)[2] == 0 and oracle("empty", 1)[1]["raw_hits"] == 0 and oracle("empty", 0)[1]["raw_hits"] > 0
    assert oracle("chunks", 149)[1]["raw_hits"] > 3 * 4096                 # three chunks and more under the limit
    for name in ("self", "within", "interval", "repx", "seed_12s3", "plainhits"):
        lim = W.limits(lzo, name)[0]
        assert 0 < oracle(name, lim)[1]["raw_hits"] < oracle(name, 0)[1]["raw_hits"], name


@pytest.mark.parametrize("key,name", PAIRS)
def test_the_path_that_ran(runs, key, name):
    c = W.CASES[name]
    for m in runs[key][1][name]:
        la = m["launches"]
        assert m["scan_modes"] == [c["mode"]] * 2, (key, name, m)
        limits_something = m["limit"] and m["num_words"] < oracle(name, 0)[2]
        assert (la.get("k_limit_copy", 0) > 0) == bool(limits_something and m["num_words"]), (key, name, m)
        if key == "fused" and c["mode"] == 0 and c["extend"] and oracle(name, m["limit"])[1]["raw_hits"]:
            assert la.get("k_fill_hits", 0) == 0, (key, name, m)
            if limits_something:                                            # wctx is rebuilt for this table, once for the two strands
                assert la.get("k_build_wctx", 0) == 1, (key, name, m)
        elif oracle(name, m["limit"])[1]["raw_hits"]:
            assert la.get("k_fill_hits", 0) > 0 and la.get("k_build_wctx", 0) == 0, (key, name, m)
    if name == "chunks":
        assert runs[key][1][name][0]["launches"].get("k_settle2", 0) >= 3


# ---------------------------------------------------------------------------------------- in process

def _search_both(gpu, masked, q):
    return [gpu.seed_hit_search(masked, q=x) for x in (q, W.seqio.revcomp(q))]


def _same(a, b):
    return all(len(x) == len(y) and (x == y).all() for x, y in zip(a, b))


def test_find_limit_equals_the_reference_arithmetic(gpu):
    t = W.seq("rep20")
    gpu.table_prepare(t, gpu.seed(), CTB)
    tab = lzo.Table(t, lzo.seed())
    dist = W.distribution(tab)
    count, words = gpu.table_count_distribution()
    assert (count == dist[0]).all() and (words == dist[1]).all()
    on_boundary = W.boundary_keeps(dist)
    assert len(on_boundary) == 2
    keeps = [W.keep_of(p) for p in W.GOLDEN_PERCENTS] + on_boundary + [0.999, 0.001, 0.25, 0.97, 0.7]
    assert len(set(keeps)) == 10
    want = [W.find_limit(tab, k, dist) for k in keeps]
    assert [gpu.table_find_limit(k) for k in keeps] == want
    assert len(set(want)) >= 4
    gpu.table_limit(7)                                                      # ... on the unlimited table, also under a limit
    assert [gpu.table_find_limit(k) for k in keeps] == want
    gpu.table_limit(0)
    for name in ("seed_7", "seed_12s3", "interval"):                        # other weights, a step, an interval
        c = W.CASES[name]
        gpu.table_prepare(W.seq(c["t"]), gpu.seed(c["pattern"], c["trans"]), CTB, step=c["step"], start=c["start"], end=c["end"])
        tab = W.fresh_table(lzo, name)
        for k in (0.5, 0.8, 0.95):
            assert gpu.table_find_limit(k) == W.find_limit(tab, k), (name, k)


def test_export_and_save_describe_the_unlimited_table(gpu, tmp_path):
    _, masked = H.scoring()
    t, q = W.seq("rep20"), W.seq("rep")
    gpu.table_prepare(t, gpu.seed(), CTB)
    tab = lzo.Table(t, lzo.seed())
    pt = tab.pt.contents
    full = gpu.table_num_words()
    last0, prev0 = gpu.table_export(int(pt.prev_entries))
    assert (last0 == np.ctypeslib.as_array(pt.last, shape=(int(pt.word_entries),))).all()
    assert (prev0 == np.ctypeslib.as_array(pt.prev, shape=(int(pt.prev_entries),))).all()
    bufs0 = gpu.table_buffers()
    unlimited = _search_both(gpu, masked, q)
    gpu.table_limit(7)
    assert 0 < gpu.table_num_words() < full
    limited = _search_both(gpu, masked, q)
    assert not _same(limited, unlimited)
    last, prev = gpu.table_export(int(pt.prev_entries))
    assert (last == last0).all() and (prev == prev0).all()
    assert gpu.table_geom().num_words == full and gpu.table_buffers() == bufs0
    gpu.table_save(tmp_path / "t.lztab")
    gpu.table_limit(7)                                                      # the same limit again: nothing changes
    assert _same(_search_both(gpu, masked, q), limited)
    gpu.table_limit(39)                                                     # another limit starts from the unlimited table
    want = W.oracle_search(lzo, "rep20_rep", masked, 39)
    assert gpu.table_num_words() == want[2] and _same(_search_both(gpu, masked, q), want[0])
    gpu.table_load(tmp_path / "t.lztab")                                    # a table that is made ends the limit
    assert gpu.table_num_words() == full and _same(_search_both(gpu, masked, q), unlimited)


def test_what_ends_a_limit(gpu, tmp_path):
    _, masked = H.scoring()
    t, q = W.seq("rep20"), W.seq("rep")
    gpu.table_prepare(t, gpu.seed(), CTB)
    full = gpu.table_num_words()
    unlimited = _search_both(gpu, masked, q)

    def limit_and_search():
        gpu.table_limit(1)
        assert 0 < gpu.table_num_words() < full
        assert not _same(_search_both(gpu, masked, q), unlimited)

    def is_unlimited():
        assert gpu.table_num_words() == full and _same(_search_both(gpu, masked, q), unlimited)

    limit_and_search(); gpu.table_limit(0); is_unlimited()
    limit_and_search(); gpu.table_rebuild(); is_unlimited()
    limit_and_search(); gpu.table_prepare(t, gpu.seed(), CTB); is_unlimited()
    gpu.table_save(tmp_path / "t.lztab")
    limit_and_search(); gpu.table_load(tmp_path / "t.lztab"); is_unlimited()
    limit_and_search()                                                      # the bucket-owner kernels read the limited table too:
    want = W.oracle_search(lzo, "rep20_rep", masked, 1)[1]["raw_hits"]      # every raw hit of it has one owner
    raw = 0
    try:
        for owner in (0, 1, 2):
            gpu.set_bucket_owner(3, owner)
            gpu.counters_reset()
            _search_both(gpu, masked, q)
            raw += gpu.counters()["raw_hits"]
    finally:
        gpu.set_bucket_owner(1, 0)
    gpu.table_limit(0)
    assert raw == want and want > 0
    is_unlimited()


def test_without_a_table_both_calls_are_state_errors(gpu):
    gpu.target_upload(W.seq("rep20"))                                       # a target, no table
    with pytest.raises(lzgpu.LzGpuError, match="rc=-5"):                    # LZGPU_ERR_STATE
        gpu.table_limit(5)
    with pytest.raises(lzgpu.LzGpuError, match="rc=-5"):
        gpu.table_find_limit(0.5)
    with pytest.raises(lzgpu.LzGpuError, match="rc=-5"):
        gpu.table_count_distribution()
