"""Dynamic masking of the position table (lastz --masking) on the CPU, over the cases of tests/table_mask_cases.py.

tests/emul/emul_mask.cpp runs the per-lane logic of the three masking kernels (lastz_amd/csrc/lz_mask.hpp, the functions
mask_kernels.hip compiles) as plain loops over the oracle's CSR table.  After every event of every case the result must be
the table the oracle BUILDS from the masked bytes, list order included (table_mask_cases.py says why that is the expected
value), and every case must reach what it is for.  CPU only."""
import numpy as np
import pytest

from oracle import lzo
import table_mask_cases as TM


def _run(name):
    """-> per event (wstart, wpos) after it, starting from the oracle's table of the unmasked target"""
    g = TM.geometry(name)
    ws, wp = TM.table(lzo, name, TM.target(name)).csr()
    out = [(ws, wp)]
    for widened, _ in TM.events(lzo, name):
        rc, ws, wp = TM.emul_mask(ws, wp, widened, g["L"], g["tlen"])
        assert rc == 0, (name, rc)
        out.append((ws, wp))
    return out


@pytest.mark.parametrize("name", list(TM.CASES))
def test_masked_table_is_the_table_of_the_masked_bytes(name):
    got = _run(name)
    want = TM.expected(lzo, name)
    assert len(got) == len(want) + 1
    for k, (_, tab) in enumerate(want):
        ws, wp = tab.csr()
        assert len(got[k + 1][1]) == len(wp), (name, k)
        assert (got[k + 1][0] == ws).all() and (got[k + 1][1] == wp).all(), (name, k)


def test_cases_reach_what_they_are_for():
    n = {name: [len(wp) for _, wp in _run(name)] for name in TM.CASES}
    print("\n", n)
    for name, v in n.items():
        assert v[0] > 0, name
        if name != "short":
            assert all(a > b for a, b in zip(v, v[1:])), (name, v)      # every event removes something
    assert n["short"][1] == n["short"][0] and n["short"][2] < n["short"][1]   # intervals shorter than L remove nothing
    assert n["whole"][1] == 0
    assert n["many"][1] > 0 and n["long"][1] > 0 and n["inside"][1] > 0
    # list_ends: the first, the last and a middle entry of one list of more than 50 go, and the list stays
    cores, ps = TM._list_cores(lzo, "list_ends", "ends")
    ws0, wp0 = TM.table(lzo, "list_ends", TM.target("list_ends")).csr()
    w = int(np.argmax(np.diff(ws0.astype(np.int64))))
    lst0 = wp0[ws0[w]: ws0[w + 1]]
    ws1, wp1 = _run("list_ends")[1]
    lst1 = wp1[ws1[w]: ws1[w + 1]]
    assert lst0[0] in ps and lst0[-1] in ps and not set(ps) & set(lst1.tolist()) and len(lst1) >= len(lst0) - 3 * 4
    assert lst1.tolist() == [p for p in lst0.tolist() if p in set(lst1.tolist())]              # order kept
    # list_empty: three lists of one entry become empty
    _, ps = TM._list_cores(lzo, "list_empty", "single")
    ws0, wp0 = TM.table(lzo, "list_empty", TM.target("list_empty")).csr()
    ws1, _ = _run("list_empty")[1]
    n0, n1 = np.diff(ws0.astype(np.int64)), np.diff(ws1.astype(np.int64))
    for p in ps:
        w = int(np.searchsorted(ws0, np.flatnonzero(wp0 == p)[0], side="right") - 1)
        assert n0[w] == 1 and n1[w] == 0
    # the clamps of the widening fire, and two_events' second event overlaps its first
    g = TM.geometry("clamps")
    wd = TM.events(lzo, "clamps")[0][0]
    assert wd[0][0] == 0 and wd[-1][1] == g["tlen"]
    (w1, _), (w2, _) = TM.events(lzo, "two_events")
    assert any(a < d and c < b for a, b in w1 for c, d in w2)
    assert len(TM.events(lzo, "many")[0][0]) == 3000 and all(20 <= e - s <= 60 for s, e in TM.events(lzo, "many")[0][0])


def test_bad_intervals_are_refused():
    ws, wp = TM.table(lzo, "clamps", TM.target("clamps")).csr()
    for iv in ([(10, 10)], [(20, 10)], [(0, 40001)], [(100, 200), (39999, 40001)]):
        assert TM.emul_mask(ws, wp, iv, 19, 40000)[0] == 1


def test_word_bits():
    """lz_mask_word_bits against the definition, through a pass over a table that holds every position once"""
    tlen = 200
    ws = np.array([0, tlen + 1], dtype=np.uint32)
    wp = np.arange(tlen, -1, -1, dtype=np.uint32)
    for s, e in ((0, 1), (0, 31), (0, 32), (1, 33), (30, 34), (31, 32), (63, 64), (0, 200), (5, 130), (64, 96), (95, 97), (199, 200)):
        rc, ws1, wp1 = TM.emul_mask(ws, wp, [(s, e)], 1, tlen)
        assert rc == 0
        assert wp1.tolist() == [p for p in wp.tolist() if not s + 1 <= p <= e], (s, e)
        assert ws1.tolist() == [0, len(wp1)]
