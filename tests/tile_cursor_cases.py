"""The pairs of tests/test_gpu_tile_cursor.py (run by tests/gpu_child.py) and of tests/test_tile_cursor.py's last case.

  gap      random sequences over A and G only, 40,000 x 40,000, drawn as tile_runs_cases.sparse_pair draws them: 5.07 M hits =
           310 partition tiles, all on the forward strand, by query position on the diagonals -39,981 .. 39,981.  A partition
           byte (bits 8..15 of the diagonal) comes round every 65,536 diagonals, so partitions 100..155 hold two bands of
           diagonals, one met in the first tiles and one in the last, and nothing in up to 196 consecutive tiles between them:
           more than the 127 tiles of a cursor block, so a sorter wave moves its cursor inside a window, over blocks of empty runs
  chunks   the same pair in chunks of at most 2,000,000 hits: the cursors restart per chunk in the middle of the gap
  tandem   tile_runs_cases' tandem: runs longer than a settle tile, so most rounds meet no run boundary at all"""
import numpy as np

import helpers as H
import tile_runs_cases as Ch

GAP_LEN = 40_000
CHUNK_CAPACITY = 2_000_000
TILE = 16384                                                 # lz_tile_runs.hpp: LZ_PP_TILE_HOST


def gap_pair():
    rng = np.random.default_rng(23)
    ag = np.frombuffer(b"AG", dtype=np.uint8)
    return ag[rng.integers(0, 2, GAP_LEN)].copy(), ag[rng.integers(0, 2, GAP_LEN)].copy()


def _words(s, ones):
    """per start position: the seed's twelve positions as bits (A = 0, G = 1)"""
    bit = (s == ord("G")).astype(np.int64)
    n = len(s) - ones[-1]
    w = np.zeros(n, dtype=np.int64)
    for k in ones:
        w = (w << 1) | bit[k:k + n]
    return w


def gap_partition_bytes():
    """the partition byte of every raw hit of the gap pair's forward strand, by query position (inside one query position:
    equal words first, then the twelve single flips, target positions ascending): two words hit if they are equal or one
    A/G flip (a transition) apart over the seed's twelve positions"""
    t, q = gap_pair()
    ones = [k for k, c in enumerate(H.DEFAULT_SEED) if c == "1"]
    assert len(ones) == 12
    wt, wq = _words(t, ones), _words(q, ones)
    order = np.argsort(wt, kind="stable")                     # target positions by word
    start = np.searchsorted(wt[order], np.arange(4097))
    pos1, pos2, rank = [], [], []
    for v, flip in enumerate([0] + [1 << k for k in range(12)]):
        w = wq ^ flip
        cnt = start[w + 1] - start[w]
        j = np.repeat(np.arange(len(wq)), cnt)
        off = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        pos1.append(order[np.repeat(start[w], cnt) + off]); pos2.append(j); rank.append(np.full(len(j), v))
    pos1, pos2, rank = np.concatenate(pos1), np.concatenate(pos2), np.concatenate(rank)
    o = np.lexsort((pos1, rank, pos2))
    return (((pos1[o] - pos2[o]) >> 8) & 255).astype(np.uint8)


def longest_gap(bins):
    """over the partitions: the most consecutive partition tiles without a record between two tiles that hold some"""
    nt = (len(bins) + TILE - 1) // TILE
    tile = np.arange(len(bins)) // TILE
    holds = np.zeros((256, nt), dtype=bool)
    holds[bins, tile] = True
    best = 0
    for p in range(256):
        at = np.flatnonzero(holds[p])
        if len(at) > 1:
            best = max(best, int(np.diff(at).max()) - 1)
    return best


PAIRS = {"gap": (gap_pair, None), "chunks": (gap_pair, CHUNK_CAPACITY), "tandem": (Ch.tandem_pair, None)}


def run(g, name):
    make, capacity = PAIRS[name]
    t, q = make()
    _, masked = H.scoring()
    g.table_prepare(t, g.seed(H.DEFAULT_SEED, 1), Ch.CTB)
    if capacity:
        g.set_hit_capacity(capacity)
    try:
        yield H.search_strands(g, lambda qq: g.seed_hit_search(masked, q=qq), [qq for _, _, qq in H.strands(q)])
    finally:
        if capacity:
            g.set_hit_capacity(1 << 28)
