"""The pairs of tests/test_gpu_tile_runs.py, run by tests/gpu_child.py under the scan mode on its command line and whatever
LZGPU_FUSED_SCAN the parent put into its environment."""
import numpy as np

from lastz_amd import seqio
from oracle import lzo
import helpers as H

CTB = lzo.upper_nuc_to_bits()
SPARSE_LEN = 20_000
CHUNK_CAPACITY = 300_000


def small_pair():
    """3 kbp x 3 kbp: far fewer hits than one partition tile (16384)"""
    return seqio.synth_pair(3_000, 3_000, seed=21)


def tandem_pair():
    """251 x 'A' at the same offset of both sequences: 233 x 233 word pairs hit, on the diagonals -232 .. 232, so every one
    of them lies in partition 0 or 255 (bits 8..15 of the diagonal): four tiles, each with runs of thousands of records --
    longer than a settle tile (5376)"""
    t, q = seqio.synth_pair(3_000, 3_000, seed=22)
    t = t.copy(); q = q.copy()
    t[1_000:1_251] = ord("A"); q[1_000:1_251] = ord("A")
    return t, q


def sparse_pair():
    """random sequences over A and G only, default seed with one transition: 13 of 4096 word pairs hit, 1.27 M hits = 77
    tiles on the forward strand (none on the other), in discovery order = by query position, on the diagonals
    -19,981 .. 19,981: partitions 0..78 and 178..255 hold records, 99 hold none, and those at the edge of the range
    (77, 78, 178) have records only in the first or the last tiles, none in the 76 others.  A mismatch is a transition
    (-31 against matches of 91..100): scans run long, many records take the SLOW path"""
    rng = np.random.default_rng(23)
    ag = np.frombuffer(b"AG", dtype=np.uint8)
    return ag[rng.integers(0, 2, SPARSE_LEN)].copy(), ag[rng.integers(0, 2, SPARSE_LEN)].copy()


PAIRS = {"small": (small_pair, None), "tandem": (tandem_pair, None), "sparse": (sparse_pair, None), "chunks": (sparse_pair, CHUNK_CAPACITY)}


def run(g, name):
    make, capacity = PAIRS[name]
    t, q = make()
    _, masked = H.scoring()
    g.table_prepare(t, g.seed(H.DEFAULT_SEED, 1), CTB)
    if capacity:
        g.set_hit_capacity(capacity)
    try:
        yield H.search_strands(g, lambda qq: g.seed_hit_search(masked, q=qq), [qq for _, _, qq in H.strands(q)])
    finally:
        if capacity:
            g.set_hit_capacity(1 << 28)
