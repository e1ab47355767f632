"""k_settle2's sorter waves naming each rank's run with the entry cursor (lastz_amd/csrc/lz_tile_runs.hpp: lz_tc_*, CPU tier:
tests/test_tile_cursor.py) against the oracle: HSP arrays of both strands and the four counters, through the fused path, on
tests/tile_cursor_cases.py's

  gap      a random 40,000 x 40,000 pair over the letters A and G: 5.07 M hits in 310 partition tiles, partitions with records
           at both ends of the chunk and up to 196 consecutive empty runs between them -- more than the 127 tiles of a
           cursor block, so a window moves the cursor while it is being located, over a block of empty runs
  chunks   the same pair in chunks of at most 2,000,000 hits: the cursors restart per chunk in the middle of the gap
  tandem   runs longer than a settle tile: many rounds without a run boundary

(k_settle_exact and k_settle_mismatch compile the same sorter text.  Their case tables, exact_cases.py and mismatch_cases.py,
are keyed by name with generators of their own and take no arbitrary pair, so `gap` does not run through them here; their
own tests, test_gpu_exact.py and test_gpu_mismatch.py, run that text.)

Every case runs in a fresh child process under its own time limit, one after the other; the first child that fails ends the
series -- nothing more is started on the GPU after a fault.  Needs an MI355X."""
import pytest

from oracle import lzo
import helpers as H
import tile_cursor_cases as Cc

pytestmark = pytest.mark.gpu
CASES = ["gap", "chunks", "tandem"]
BLOCK = 128                                                  # lz_tile_runs.hpp: LZ_TR_BLOCK


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    out = H.run_gpu_children(tmp_path_factory.mktemp("tile_cursor"),
                             [(name, "tile_cursor_cases", [name], {"LZGPU_FUSED_SCAN": "1"}, 300, 0) for name in CASES])
    return {name: (z, meta[name][0]) for name, (z, meta) in out.items()}


@pytest.fixture(scope="module")
def oracle():
    """per pair: the oracle's HSP arrays of both strands and its counters summed over them (computed once)"""
    _, masked = H.scoring()
    out = {}
    for name in ("gap", "tandem"):
        t, q = Cc.PAIRS[name][0]()
        tab = lzo.Table(t, lzo.seed(H.DEFAULT_SEED, 1))
        hs, tot = [], dict.fromkeys(H.COUNTERS, 0)
        for _, _, qq in H.strands(q):
            h, st = lzo.seed_hit_search(tab, qq, masked)
            hs.append(h)
            for c in H.COUNTERS:
                tot[c] += st[c]
        out[name] = (hs, tot)
    out["chunks"] = out["gap"]
    return out


@pytest.mark.parametrize("name", CASES)
def test_hsps_and_counters_equal_the_oracle(runs, oracle, name):
    z, meta = runs[name]
    want, tot = oracle[name]
    for k in (0, 1):
        got = z["%s/0/%d" % (name, k)]
        assert len(got) == len(want[k]) and (got == want[k]).all(), (name, k)
    assert sum(len(h) for h in want) > 0
    for c in H.COUNTERS:
        assert meta["counters"][c] == tot[c], (name, c)


def test_the_path_that_ran(runs):
    for name in CASES:
        meta = runs[name][1]
        la = meta["launches"]
        assert meta["scan_modes"] == [0, 0], name
        assert la.get("k_fill_hits", 0) == 0 and "k_hist" not in la, (name, la)
        for k in ("k_partition", "k_hist_scan", "k_settle2"):
            assert la.get(k, 0) > 0, (name, k, la)


def test_the_gap_is_there(runs, oracle):
    """the partition bytes of the gap pair's hits, recomputed: as many hits as the search counted, all of them on the forward
    strand, and a partition with more consecutive empty tiles between two of its runs than a cursor block covers"""
    bins = Cc.gap_partition_bytes()
    assert len(bins) == runs["gap"][1]["counters"]["raw_hits"] == oracle["gap"][1]["raw_hits"]
    assert Cc.longest_gap(bins) >= BLOCK
    assert runs["chunks"][1]["launches"]["k_settle2"] >= 3 > runs["gap"][1]["launches"]["k_settle2"]
