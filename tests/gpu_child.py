"""The child process of the GPU tests that vary a process setting of the library (LZGPU_FUSED_SCAN, LZGPU_TASK_REGION_CAP:
read once per process, so each setting needs a process of its own; tests/helpers.py: run_gpu_children starts them).

    python tests/gpu_child.py OUT.npz CASES_MODULE [--scan-mode N] CASE [CASE ...]

CASES_MODULE (fused_scan_cases, tile_runs_cases, scorings, self_cases) has run(g, case), a generator of the case's runs: each
does its searches when asked for and gives {"hsps": one array per strand, "scan_modes": one per strand} (helpers.search_strands),
with "capacity" where the case runs under several hit capacities.  Saved: the arrays as CASE/RUN/STRAND, and as `meta`
{CASE: [per run {"counters", "scan_modes", "launches", "seconds"[, "capacity"]}]} -- the module's COUNTERS, else the four common ones."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from lastz_amd import lzgpu                         # noqa: E402
import helpers as H                                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out"); ap.add_argument("module"); ap.add_argument("--scan-mode", type=int); ap.add_argument("cases", nargs="+")
    a = ap.parse_args()
    mod = importlib.import_module(a.module)
    counters = getattr(mod, "COUNTERS", H.COUNTERS)
    g = lzgpu.Lib(); g.init()
    g.profile_enable(True)
    if a.scan_mode is not None:
        g.set_scan_mode(a.scan_mode)
    res, meta = {}, {}
    for case in a.cases:
        meta[case] = []
        g.profile_reset(); g.counters_reset()
        t0 = time.perf_counter()
        for run in mod.run(g, case):                # (a run's searches happen inside the generator: between two yields)
            wall = time.perf_counter() - t0
            c = g.counters()
            for k, h in enumerate(run.pop("hsps")):
                res["%s/%d/%d" % (case, len(meta[case]), k)] = h
            meta[case].append(dict(run, counters={k: c[k] for k in counters}, seconds=round(wall, 3),
                                   launches={k: v["launches"] for k, v in g.profile().items()}))
            g.profile_reset(); g.counters_reset()
            t0 = time.perf_counter()
    g.shutdown()
    np.savez(a.out, meta=np.array(json.dumps(meta)), **res)
    print("gpu child ok")


if __name__ == "__main__":
    main()
