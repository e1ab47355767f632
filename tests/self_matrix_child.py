"""Child process of tests/test_gpu_self_matrix.py: runs the named cases of tests/self_cases.py through
lzgpu_seed_hit_search_self under whatever LZGPU_FUSED_SCAN the parent put into the environment (read once per process)
and saves, per case and per run of it (a chunked case runs once per hit capacity), the HSP arrays of each strand, the
five counters, the scan mode and the launches the profile saw, and the run's wall time.

    python tests/self_matrix_child.py OUT.npz CASE [CASE ...]
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
import self_cases as S                              # noqa: E402

CTB = lzo.upper_nuc_to_bits()
WHOLE = 1 << 28                                     # the hit capacity that chunks nothing here


def run_case(g, name, capacity):
    c = S.CASES[name]
    v, seps, _ = S.sequence(name)
    _, masked = H.scoring()
    g.set_scan_mode(c["force_mode"])
    g.set_hit_capacity(capacity or WHOLE)
    try:
        g.table_prepare(v, g.seed(c["pattern"], c["trans"]), CTB, step=c["step"])
        return [g.seed_hit_search_self(masked, q=v if strand == "+" else S.minus(v, seps), same_strand=(strand == "+"),
                                       band_width=c["band"], sep1=seps or None, sep2=seps or None, xdrop=c["xdrop"],
                                       hsp_threshold=c["hsp_threshold"], entropic=c["entropic"], extend=c["extend"])
                for strand in c["strands"]]
    finally:
        g.set_hit_capacity(WHOLE)
        g.set_scan_mode(0)


def main():
    out, names = sys.argv[1], sys.argv[2:]
    g = lzgpu.Lib(); g.init()
    g.profile_enable(True)
    res, meta = {}, {}
    for name in names:
        meta[name] = []
        for r, capacity in enumerate(S.CASES[name]["capacities"]):
            g.profile_reset(); g.counters_reset()
            t0 = time.perf_counter()
            hs = run_case(g, name, capacity)
            wall = time.perf_counter() - t0
            c = g.counters()
            for k, h in enumerate(hs):
                res["%s.%d.%d" % (name, r, k)] = h
            meta[name].append({"capacity": capacity, "counters": {k: c[k] for k in S.COUNTERS}, "scan_mode": g.last_scan_mode(),
                               "launches": {k: v["launches"] for k, v in g.profile().items()}, "seconds": round(wall, 3)})
    g.shutdown()
    np.savez(out, meta=np.array(json.dumps(meta)), **res)
    print("self matrix child ok")


if __name__ == "__main__":
    main()
