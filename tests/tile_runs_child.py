"""Child process of tests/test_gpu_tile_runs.py: runs the cases below under the scan mode given on the command line and
whatever LZGPU_FUSED_SCAN the parent put into the environment (read once per process) and saves, per case, the HSP
arrays of both strands, the counters, the scan mode and the launches the profile saw.

    python tests/tile_runs_child.py OUT.npz MIN_SCAN_MODE CASE [CASE ...]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from lastz_amd import lzgpu, seqio                 # noqa: E402
from oracle import lzo                              # noqa: E402
import helpers as H                                 # noqa: E402

CTB = lzo.upper_nuc_to_bits()
COUNTERS = ("words", "raw_hits", "extensions", "bp_extended")
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


def run_case(g, name):
    make, capacity = PAIRS[name]
    t, q = make()
    _, masked = H.scoring()
    g.table_prepare(t, g.seed(H.DEFAULT_SEED, 1), CTB)
    if capacity:
        g.set_hit_capacity(capacity)
    try:
        return [g.seed_hit_search(masked, q=qq) for _, _, qq in H.strands(q)]
    finally:
        if capacity:
            g.set_hit_capacity(1 << 28)


def main():
    out, mode, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    g = lzgpu.Lib(); g.init()
    g.profile_enable(True)
    g.set_scan_mode(mode)
    res, meta = {}, {}
    for name in names:
        g.profile_reset(); g.counters_reset()
        hs = run_case(g, name)
        c = g.counters()
        for k, h in enumerate(hs):
            res["%s.%d" % (name, k)] = h
        meta[name] = {"counters": {k: c[k] for k in COUNTERS}, "scan_mode": g.last_scan_mode(),
                      "launches": {k: v["launches"] for k, v in g.profile().items()}}
    g.shutdown()
    np.savez(out, meta=np.array(json.dumps(meta)), **res)
    print("tile runs child ok")


if __name__ == "__main__":
    main()
