"""What the cases of tests/window_cases.py are built to reach, asserted on the oracle alone: a case that no longer meets
what it is for fails here, on the CPU, and not by quietly testing less on the GPU.  Also the comparison the GPU tests use
(window_cases.differs), shown to catch a dropped window, two swapped HSPs and a shifted duplicate."""
import numpy as np
import pytest

from oracle import lzo
import window_cases as WC


def test_many_reaches_what_it_is_for():
    wins, kinds = WC.many()
    t, q = WC.pair()
    n = len(wins)
    assert n == WC.N_MANY
    count = {k: kinds.count(k) for k in set(kinds)}
    print("\nmany: %s" % count)
    assert 8 <= count["big"] <= 20 and count["dup"] >= 8 and count["tiny"] >= 12
    assert 0.03 * n < count["heavy"] + count["heavy_part"] < 0.09 * n and count["heavy_part"] >= 10
    assert all(tl <= WC.LZ_WIN_MAXLEN and ql <= WC.LZ_WIN_MAXLEN and t0 >= 0 and q0 >= 0 and t0 + tl <= len(t) and q0 + ql <= len(q)
               for t0, tl, q0, ql in wins)
    # (a) whatever the grid, some block runs heavy -> small, small -> heavy and big -> small
    assert WC.transitions_missing(kinds, n // 3) == []
    # the kinds are what they are called
    for (t0, tl, q0, ql), kind in zip(wins, kinds):
        if kind in ("heavy", "heavy_part"):
            run_t = WC.longest_word_list(t[t0:t0 + tl])              # positions of the word AAAAAAA in the target piece
            run_q = ql - (int(np.flatnonzero(q[q0:q0 + ql] != WC.A).max()) + 1)     # the A the query piece ends with
            assert 200 <= run_q <= 300, (kind, ql, run_q)
            if kind == "heavy":
                assert run_t > WC.LZ_WIN_HITCAP                               # one list overflows the buffer: take == 0
            else:
                assert run_t <= WC.LZ_WIN_HITCAP < 2 * run_t                   # two lists together do: a partial take
        elif kind == "big":
            assert min(tl, ql) >= 15000
        elif kind == "small":
            assert 50 <= min(tl, ql) and max(tl, ql) <= 2000
        elif kind == "tiny":
            assert min(tl, ql) in (0, 3, WC.L - 1)
    assert {min(w[1], w[3]) for w, k in zip(wins, kinds) if k == "tiny"} == {0, 3, WC.L - 1}
    lo, hi = WC.expected("many", 600), WC.expected("many", 2200)
    # (b) more HSPs than the launcher's first room of a large call
    assert sum(len(x) for x in lo) > 64 * n
    # (c) homology in most small windows, and order is tested
    small = [k for k in range(n) if kinds[k] == "small"]
    assert sum(len(hi[k]) > 0 for k in small) > len(small) // 2
    assert sum(len(x) > 1 for x in hi) >= 100 and sum(len(x) > 1 for x in lo) >= 100
    assert sum(len(hi[k]) > 0 for k in range(n) if kinds[k] in ("heavy", "heavy_part")) > 0
    # (d) a duplicate equals its original
    for k in range(n):
        if kinds[k] == "dup":
            first = wins.index(wins[k])
            assert first < k
            for want in (lo, hi):
                assert len(want[k]) == len(want[first]) and (want[k] == want[first]).all()
    assert sum(len(hi[k]) > 0 for k in range(n) if kinds[k] == "dup") >= 3


def test_retry_small_reaches_the_retry():
    wins = WC.retry_small()
    assert len(wins) == 8 and WC.BIG_UNRELATED in wins
    assert sum(len(x) for x in WC.expected("retry_small", 600)) > max(64 * 8, 4096)
    assert 0 < sum(len(x) for x in WC.expected("retry_small", 3000)) < 4096


def test_edges_reach_the_edges():
    wins = WC.edges()
    ts, qs, n = WC.SAME
    for t0, tl, q0, ql in [WC.IDENTICAL] + WC.INSIDE:                    # strictly inside the identical stretch, shifted or not
        assert ts < t0 and t0 + 3 + tl < ts + n and qs < q0 and q0 + 3 + ql < qs + n
    assert WC.IDENTICAL[0] - ts == WC.IDENTICAL[2] - qs                   # ... the square one on its diagonal
    for thr in (600, 2200):
        want = WC.expected("edges", thr)
        full = want[wins.index(WC.IDENTICAL)]
        hit = full[full["length"] == WC.LZ_WIN_MAXLEN]
        assert len(hit) == 1 and int(hit["score"][0]) == WC.IDENTICAL_SCORE
        assert (int(hit["pos1"][0]), int(hit["pos2"][0])) == (WC.LZ_WIN_MAXLEN, WC.LZ_WIN_MAXLEN)      # diagEnd reaches 20480
        # inside a longer identical stretch the HSP runs from edge to edge of the window, whichever side is the shorter
        for w in WC.INSIDE:
            hs = want[wins.index(w)]
            d = (w[2] - WC.SAME[1]) - (w[0] - WC.SAME[0])             # the stretch's diagonal in window coordinates: pos1 - pos2
            lo1, hi1 = max(0, d), min(w[1], w[3] + d)
            edge = hs[(hs["pos1"] == hi1) & (hs["length"] == hi1 - lo1)]
            assert len(edge) == 1 and int(edge["pos1"][0]) - int(edge["pos2"][0]) == d, (w, d)
            assert hi1 - lo1 >= 12000
        # 60-base copies in opposite corners: diagonal indices pos1 - pos2 + q_len within 60 of 0 and of t_len + q_len
        t0, tl, q0, ql = WC.CORNERS60
        hs = want[wins.index(WC.CORNERS60)]
        dg = hs["pos1"].astype(np.int64) - hs["pos2"].astype(np.int64) + ql
        assert (dg == 60).sum() == 1 and (dg == tl + ql - 60).sum() == 1
        for s in (1, 2, 3):                                            # shifted: the copies are cut by the window's edge
            hs = want[wins.index(WC._shift(WC.CORNERS60, s))]
            dg = hs["pos1"].astype(np.int64) - hs["pos2"].astype(np.int64) + ql
            assert (dg == 60).sum() == 1 and (dg == tl + ql - 60).sum() == 1
            full = want[wins.index(WC._shift(WC.IDENTICAL, s))]
            assert (full["length"] == WC.LZ_WIN_MAXLEN).sum() == 1
    # 7-base copies in the very corners: the first and the last diagonal a window has, HSPs at threshold 600 only
    t0, tl, q0, ql = WC.CORNERS7
    hs = WC.expected("edges", 600)[wins.index(WC.CORNERS7)]
    ends = {(int(h["pos1"]), int(h["pos2"]), int(h["length"])) for h in hs}
    assert (WC.L, ql, WC.L) in ends and (tl, WC.L, WC.L) in ends


@pytest.mark.parametrize("pattern", list(WC.LIGHT))
def test_light_tables_find_homology(pattern):
    sd = lzo.seed(pattern, 0)
    wins = WC.light_windows(pattern)
    assert all(max(w[1], w[3]) <= WC.LIGHT[pattern] for w in wins) and sd.num_probes == 1 and sd.weight <= 14
    want = WC.expected("light_" + pattern, WC.LIGHT_THR)
    assert sum(len(x) > 0 for x in want) >= 4 and sum(len(x) for x in want) >= 8, [len(x) for x in want]
    if pattern in ("11", "111"):
        assert (1 << sd.weight) < WC.LZ_WIN_TPB                        # fewer words than the workgroup has lanes


def test_light_tables_weights():
    assert sorted(lzo.seed(p, 0).weight for p in WC.LIGHT) == [4, 6, 8, 10, 12, 14]


def test_the_comparison_catches_a_wrong_result():
    """the GPU tests' comparison, on the oracle's own lists with one defect each"""
    want = WC.expected("many", 2200)
    wins, kinds = WC.many()
    assert WC.differs([x.copy() for x in want], want) is None
    k = next(k for k, x in enumerate(want) if len(x) > 0)
    dropped = list(want); dropped[k] = WC.EMPTY
    assert WC.differs(dropped, want) == k
    k = next(k for k, x in enumerate(want) if len(x) > 1)
    swapped = list(want); swapped[k] = want[k].copy(); swapped[k][[0, 1]] = swapped[k][[1, 0]]
    assert WC.differs(swapped, want) == k
    k = next(k for k in range(len(want)) if kinds[k] == "dup" and len(want[k]) > 0)
    shifted = list(want); shifted[k] = want[k].copy(); shifted[k]["pos1"] += 1
    assert WC.differs(shifted, want) == k
    assert WC.differs(want[:-1], want) == -1


def test_decline_pair_reaches_the_declines():
    r = WC.decline_reach()
    print("\ndecline pair: %s" % r)
    assert r["over_1024"] >= 16 and r["M"] > 1024 and r["raw"] > 40 * r["M"]      # capacity M: many chunks
    assert r["C"] > 16 and r["hsps"] < r["C"] // 2                    # entropy leaves far fewer than the candidates
    for kind in ("self", "within"):
        k = WC.decline_reach(kind)
        print("%s: %s" % (kind, k))
        assert k["M"] > 1024 and k["C"] > 16                          # (the filtered search's HSPs all fall to entropy: it is compared without it too)
    # the plain search is neither the self nor the filtered one
    assert len(WC.oracle_of("plain")[0]) != len(WC.oracle_of("self")[0]) and r["raw"] != WC.decline_reach("within")["raw"]
    assert WC.row_classes(WC.many_classes()) > 32 >= WC.row_classes(WC.masked())
    assert WC.row_classes(WC.eight()) <= 32


def test_the_scripted_sequence_has_something_to_compare_at_every_step():
    o = WC.script_oracle()
    t, _ = WC.decline_pair()
    assert len(o["plain"][0]) > 20 and len(o["limited"][0]) > 20 and len(o["within"][0]) > 0
    assert o["limited"][1]["raw_hits"] < o["plain"][1]["raw_hits"]             # the limit takes the run of A's word away
    assert o["within"][1]["raw_hits"] < o["limited"][1]["raw_hits"]
    assert sum(len(x) for x in o["windows"]) > 5 and sum(len(x) > 0 for x in o["windows"]) >= 2
    at = np.flatnonzero(o["fenced"] != t)
    assert at.tolist() == [o["t_iv"][0] - 1, o["t_iv"][1]]
    # the windows' HSPs under `eight` are not HOXD70's: the matrix matters
    assert WC.differs([WC.want(w, WC.SCRIPT_THR, seqs=WC.decline_pair()) for w in WC.SCRIPT_WINDOWS], o["windows"]) is not None
