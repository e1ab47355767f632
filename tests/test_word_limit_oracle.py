"""lastz --maxwordcount against the oracle, on the CPU: what the pristine binary printed (tests/golden/word_limit_*.segments
through word_limit_index.json, `--nogapped --format=segments`, recorded by tests/golden/make_word_limit_golden.py) is what
the oracle finds on a table that tests/word_limit_cases.py limited from outside -- last[w] = 0 for every word of more than
<n> positions -- and the limit the binary took for --maxwordcount=<p>% is the one find_limit() computes.  This pins the two
statements the GPU tests of lzgpu_table_limit / lzgpu_table_find_limit rely on.  Where oracle/_ref/lastz is present it is
run again."""
import sys

import pytest

from oracle import lzo
import helpers as H
import word_limit_cases as W

sys.path.insert(0, H.GOLDEN)
import make_word_limit_golden as M                  # noqa: E402

LIMITS = {"rep": W.GOLDEN_LIMITS, "probe": W.GOLDEN_PROBE_LIMITS}
RUNS = [(q, o) for q in LIMITS for o in M.options(q)]


def option_of(limit):
    return "--maxwordcount=%d" % limit if limit else None


def segments_text(name1, name2, rows):
    return "#name1\tstart1\tend1\tname2\tstart2\tend2\tstrand2\tscore\n" + "".join(
        "%s\t%d\t%d\t%s\t%d\t%d\t%s\t%d\n" % (name1, r[1], r[2], r[0], r[3], r[4], r[5], r[6]) for r in rows)


@pytest.fixture(scope="module")
def rep20_lengths():
    return W.list_lengths(lzo.Table(W.seq("rep20"), lzo.seed()))


def oracle_segments(query, limit, lengths):
    """rep20 against `query`, both strands, on the oracle's table limited to `limit` (0: not limited)"""
    _, masked = H.scoring()
    tab = lzo.Table(W.seq("rep20"), lzo.seed())
    if limit:
        W.limited(tab, limit, own=lengths)
    rows = []
    for strand, _, q in H.strands(W.seq(query)):
        hs, _ = lzo.seed_hit_search(tab, q, masked)
        rows += H.hsps_as_tsv_rows(query, strand, hs)
    return segments_text("rep20", query, rows)


@pytest.mark.parametrize("query,limit", [(q, n) for q in LIMITS for n in (0,) + LIMITS[q]])
def test_golden_is_the_oracles_search_of_the_limited_table(rep20_lengths, query, limit):
    assert oracle_segments(query, limit, rep20_lengths) == M.golden(query, option_of(limit))


def test_the_goldens_are_not_vacuous(rep20_lengths):
    longest = int(rep20_lengths.max())
    none = M.golden("rep", None)
    for n in W.GOLDEN_LIMITS:
        text = M.golden("rep", option_of(n))
        assert len(text.splitlines()) > 5, n
        assert (text != none) == (n < longest), n
    assert max(W.GOLDEN_LIMITS) > longest
    # rep20 against the probe: 1 < 7 < 8 < 39 < 47, each lets more lists in, and from 47 on nothing of the probe's is missing
    texts = [M.golden("probe", option_of(n)) for n in W.GOLDEN_PROBE_LIMITS]
    rows = [len(t.splitlines()) for t in texts]
    assert len(set(texts)) == len(texts) and rows == sorted(rows) and rows[0] < rows[1] < rows[3] < rows[4]
    assert len(texts[0].splitlines()) > 1 and texts[-1] == M.golden("probe", None)


def test_percent_form(rep20_lengths):
    """--maxwordcount=<p>%: find_limit() on the oracle's table names the limit whose search is the percent golden"""
    tab = lzo.Table(W.seq("rep20"), lzo.seed())
    dist = W.distribution(tab)
    found = [W.find_limit(tab, W.keep_of(p), dist) for p in W.GOLDEN_PERCENTS]
    assert len(set(found)) >= 3 and 1 in found, found
    assert any(dist[0][0] < n < dist[0][-1] for n in found), (found, dist[0])           # strictly inside the distribution
    for query in LIMITS:
        for p, n in zip(W.GOLDEN_PERCENTS, found):
            assert oracle_segments(query, n, rep20_lengths) == M.golden(query, "--maxwordcount=%s%%" % p), (query, p, n)
    assert len({M.golden("probe", "--maxwordcount=%s%%" % p) for p in W.GOLDEN_PERCENTS}) == 3      # each percentage its own rows


def test_find_limit_edges():
    """the arithmetic at its edges, on distributions written out by hand"""
    import numpy as np
    d = (np.array([1, 2, 10]), np.array([100, 10, 5]))                    # 100 + 20 + 50 = 170 positions
    assert W.find_limit(None, 0.5, d) == 1 and W.find_limit(None, 0.6, d) == 2           # ceil(102) - 100 = 2 <= 20
    assert W.find_limit(None, 0.75, d) == 10                               # 128 - 100 - 20 = 8 <= 50
    assert W.find_limit(None, 1e-9, d) == 1
    # each entry is compared with what is still to keep, not with the running sum
    assert W.find_limit(None, 0.6, (np.array([1, 2, 10]), np.array([90, 30, 5]))) == 2   # 120 - 90 = 30 <= 60
    assert W.find_limit(None, 0.6, (np.array([1, 2, 10]), np.array([90, 5, 10]))) == 10  # 120 - 90 - 10 = 20 <= 100
    # 2^32 positions wrap to 0 in unspos arithmetic: ceil(0 * keep) = 0, the first entry qualifies
    assert W.find_limit(None, 0.5, (np.array([1 << 16]), np.array([1 << 16]))) == 1 << 16


@pytest.mark.parametrize("query,option", RUNS)
def test_live_reference_run(tmp_path_factory, query, option):
    if lzo.ref_binary() is None:
        pytest.skip("oracle/_ref/lastz is not built here (the goldens above always run)")
    d = tmp_path_factory.getbasetemp() / "word_limit_inputs"
    if not d.exists():
        d.mkdir()
        M.write_inputs(d)
    assert M.run(option, d, query=query) == M.golden(query, option)
