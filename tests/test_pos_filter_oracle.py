"""lastz --chores against the oracle, on the CPU: what the pristine binary printed for the chores files under
tests/golden/ (chores_*.segments, `--nogapped --format=segments`) is what the oracle's restricted search finds
(tests/chores_golden.py says how the two correspond and why).  This pins the statement the GPU tests of
lzgpu_seed_hit_search_within rely on: a search under a position filter is the search of a table that holds only the
words inside the target interval, over the query interval.  Where oracle/_ref/lastz is present it is run again."""
import os

import pytest

from oracle import lzo
import helpers as H
import chores_golden as CG


def golden(name):
    return open(os.path.join(H.GOLDEN, name + ".segments")).read()


def test_the_chores_cover_what_they_should():
    assert CG.NAMES == ["chores_basic", "chores_edges"]
    basic = CG.read_chores("chores_basic")
    assert {s for c in basic for s in c[3]} == {"+", "-"} and any(c[3] == ("+", "-") for c in basic)      # both strands
    assert any(c[0] is not None and c[2] is None for c in basic)                                          # target only
    assert any(c[0] is None and c[2] is not None for c in basic)                                          # query only
    # no hits: the fifth chore of chores_basic contributes no row
    _, masked = H.scoring()
    per_chore = []
    for qname, strand, tf, qf, t_iv, q_iv in CG.searches("chores_basic"):
        per_chore.append(len(CG.oracle_hsps(tf, qf, t_iv, q_iv, masked)[0]))
    assert 0 in per_chore and sum(per_chore) == len(golden("chores_basic").splitlines()) - 1
    # edges: intervals that end on a seed window's last base and begin on a window's first base, each +- 1
    L = lzo.seed().length
    t, qs = CG.sequences()
    tab = lzo.Table(t, lzo.seed())
    hits, _ = lzo.seed_hit_search(tab, qs["pig3"], masked, mode=1)
    ends = {(int(h["pos1"]), int(h["pos2"])) for h in hits}
    edges = [(CG.resolve(c[0], len(t)), CG.resolve(c[2], len(qs["pig3"]))) for c in CG.read_chores("chores_edges")]
    assert ((4000, 5024), (18000, 18493)) in edges and (5024, 18493) in ends                  # ends ON the window's last base
    assert ((4000, 5023), (18000, 18493)) in edges and ((4000, 5024), (18000, 18492)) in edges
    assert ((4936, 6000), (18405, 19000)) in edges and (4936 + L, 18405 + L) in ends          # begins ON the window's first base
    assert ((4937, 6000), (18405, 19000)) in edges and ((4936, 6000), (18406, 19000)) in edges


@pytest.mark.parametrize("name", CG.NAMES)
def test_golden_is_the_oracles_restricted_search(name):
    want = golden(name)
    assert len(want.splitlines()) > 5
    assert CG.oracle_segments(name) == want


@pytest.mark.parametrize("name", CG.NAMES)
def test_live_reference_run(name):
    if lzo.ref_binary() is None:
        pytest.skip("oracle/_ref/lastz is not built here (the goldens above always run)")
    import sys
    sys.path.insert(0, H.GOLDEN)
    import make_chores_golden as M
    live = M.run(os.path.join(H.GOLDEN, name + ".chores"))
    assert live == golden(name)
    assert live == CG.oracle_segments(name)
