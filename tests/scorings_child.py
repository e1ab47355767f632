"""Child process of tests/test_gpu_scorings.py: runs seed-stage rows of tests/scorings.py under the scan mode given on the
command line and whatever LZGPU_FUSED_SCAN the parent put into the environment (read once per process) and saves, per case,
the HSP arrays of both strands, the counters, the scan mode and the launches the profile saw.

    python tests/scorings_child.py OUT.npz MIN_SCAN_MODE CASE [CASE ...]

CASE is a row's name, with `.s` for its variant with special bytes or `.c` for the run in chunks of at most CHUNK_CAPACITY hits.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from lastz_amd import lzgpu                         # noqa: E402
from oracle import lzo                              # noqa: E402
import helpers as H                                 # noqa: E402
import scorings as S                                # noqa: E402

CTB = lzo.upper_nuc_to_bits()
COUNTERS = ("words", "raw_hits", "extensions", "bp_extended")
CHUNK_CAPACITY = 20_000


def split_case(case):
    name, _, variant = case.partition(".")
    return name, variant == "s", variant == "c"


def run_case(g, case):
    name, specials, chunks = split_case(case)
    t, q, masked, kw, _ = S.seed_case(name, gpu=True, specials=specials)
    g.table_prepare(t, g.seed(H.DEFAULT_SEED, 1), CTB)
    if chunks:
        g.set_hit_capacity(CHUNK_CAPACITY)
    try:
        hs, modes = [], []
        for _, _, qq in H.strands(q):
            hs.append(g.seed_hit_search(masked, q=qq, **kw)); modes.append(g.last_scan_mode())
        return hs, modes
    finally:
        if chunks:
            g.set_hit_capacity(1 << 28)


def main():
    out, mode, cases = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    t0 = time.time()
    g = lzgpu.Lib(); g.init()
    g.profile_enable(True)
    g.set_scan_mode(mode)
    res, meta = {}, {}
    for case in cases:
        g.profile_reset(); g.counters_reset()
        hs, modes = run_case(g, case)
        c = g.counters()
        for k, h in enumerate(hs):
            res["%s/%d" % (case, k)] = h
        meta[case] = {"counters": {k: c[k] for k in COUNTERS}, "scan_modes": modes,
                      "launches": {k: v["launches"] for k, v in g.profile().items()}}
    g.shutdown()
    meta["seconds"] = time.time() - t0
    np.savez(out, meta=np.array(json.dumps(meta)), **res)
    print("scorings child ok")


if __name__ == "__main__":
    main()
