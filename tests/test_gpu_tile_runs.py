"""Hit tiles sorted by partition in place and phase B gathering its runs (k_partition<false> / k_partition<true> -> k_hist_scan ->
k_settle2, lastz_amd/csrc/lz_tile_runs.hpp) against the oracle: HSP arrays of both strands and the four counters, on

  small    a 3 kbp x 3 kbp pair: one partial tile
  tandem   251 x 'A' at the same offset of both sequences: 55 k hits, all of them in partitions 0 and 255, so a tile's
           run is longer than a settle tile (5376 records)
  sparse   a random 20,000 x 20,000 pair over the letters A and G: 77 tiles, 99 empty partitions, partitions whose
           records lie in the first or the last tile only, long scans and many SLOW records
  chunks   the same pair in chunks of at most 300,000 hits: runs and cursors restart per chunk, diagEnd carries over

through the fused path, and small + tandem through scan mode 1 and through the unfused path (LZGPU_FUSED_SCAN=0): every
partition kernel feeds the same settle kernel.  The profile proves the path: no launch under the label k_hist.

(On the GPU the cursor of a sorter wave moves by one block of 127 tiles at a time in test_gpu_fused_scan.py's and
test_gpu_seed.py's 2 Mbp pairs; a window that spans several blocks is tests/test_tile_runs.py's, on the CPU.)

Every setting runs in a fresh child process (LZGPU_FUSED_SCAN is read once) under its own time limit, one after the
other; the first child that fails ends the series -- nothing more is started on the GPU after a fault.  Needs an MI355X."""
import pytest

from oracle import lzo
import helpers as H
import tile_runs_cases as Ch

pytestmark = pytest.mark.gpu
TILE, S2_TILE = 16384, 5376
#          key       cases                                    scan mode  fused
RUNS = [("fused",   ["small", "tandem", "sparse", "chunks"],  0,         "1"),
        ("mode1",   ["small", "tandem"],                      1,         "1"),
        ("split",   ["small", "tandem"],                      0,         "0")]


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    out = H.run_gpu_children(tmp_path_factory.mktemp("tile_runs"),
                             [(key, "tile_runs_cases", cases, {"LZGPU_FUSED_SCAN": fused}, 300, mode) for key, cases, mode, fused in RUNS])
    return {key: (z, {name: m[0] for name, m in meta.items()}) for key, (z, meta) in out.items()}     # one run per case


@pytest.fixture(scope="module")
def oracle():
    """per pair: the oracle's HSP arrays of both strands and its counters summed over them (computed once)"""
    _, masked = H.scoring()
    out = {}
    for name in ("small", "tandem", "sparse"):
        t, q = Ch.PAIRS[name][0]()
        tab = lzo.Table(t, lzo.seed(H.DEFAULT_SEED, 1))
        hs, tot = [], dict.fromkeys(H.COUNTERS, 0)
        for _, _, qq in H.strands(q):
            h, st = lzo.seed_hit_search(tab, qq, masked)
            hs.append(h)
            for c in H.COUNTERS:
                tot[c] += st[c]
        out[name] = (hs, tot)
    out["chunks"] = out["sparse"]
    return out


@pytest.mark.parametrize("key,name", [(key, name) for key, cases, _, _ in RUNS for name in cases])
def test_hsps_and_counters_equal_the_oracle(runs, oracle, key, name):
    z, meta = runs[key]
    want, tot = oracle[name]
    for k in (0, 1):
        got = z["%s/0/%d" % (name, k)]
        assert len(got) == len(want[k]) and (got == want[k]).all(), (key, name, k)
    assert sum(len(h) for h in want) > 0
    for c in H.COUNTERS:
        assert meta[name]["counters"][c] == tot[c], (key, name, c)


def test_the_path_that_ran(runs):
    for key, cases, mode, fused in RUNS:
        meta = runs[key][1]
        for name in cases:
            la = meta[name]["launches"]
            assert meta[name]["scan_modes"] == [mode, mode], (key, name)
            assert "k_hist" not in la, (key, name, la)
            for k in ("k_partition", "k_hist_scan", "k_settle2"):
                assert la.get(k, 0) > 0, (key, name, k, la)
            assert (la.get("k_fill_hits", 0) == 0) == (fused == "1" and mode == 0), (key, name, la)


def test_cases_reach_what_they_are_for(runs):
    meta = runs["fused"][1]
    assert meta["small"]["counters"]["raw_hits"] < TILE
    assert meta["tandem"]["counters"]["raw_hits"] > 3 * TILE     # two partitions share four tiles: runs of > S2_TILE records
    assert 3 * TILE // 2 > S2_TILE
    assert meta["sparse"]["counters"]["raw_hits"] >= 70 * TILE
    assert meta["chunks"]["launches"]["k_settle2"] >= 4 > meta["sparse"]["launches"]["k_settle2"]
