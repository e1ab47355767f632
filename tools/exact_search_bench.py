"""What an exact-match search (lastz --exact=50, lzgpu_seed_hit_search_exact) costs per kernel, beside the X-drop search of
the same pair in the same process:

    python tools/exact_search_bench.py [--tlen 50000000] [--qlen 50000000] [--length 50] [--split] [--out FILE.json]

The pair is bench.py's (seqio.synth_pair(tlen, qlen, seed=1000)) under the default 12-of-19 seed.  Per search kind: one
untimed search, then ONE warm step -- both strands, the query strands resident in slots -- with lzgpu_profile_enable on:
every kernel's launches and milliseconds, the wall clock of the step, HSPs and raw hits.  The X-drop step runs the path the
benchmark runs (the fused scan kernel); --split (a process started with LZGPU_FUSED_SCAN=0) times the two-kernel path,
whose k_scan_hits and k_settle2 stand where k_scan_exact and k_settle_exact do.  One JSON object on stdout, and in --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lastz_amd import lzgpu, seqio                  # noqa: E402
from oracle import lzo                              # noqa: E402  (lastz's default scoring matrix only, as bench.py takes it)


def nuc_to_bits(lower):
    t = np.full(256, -1, dtype=np.int8)
    for k, ch in enumerate(b"ACGT"):
        t[ch] = k
        if lower:
            t[ch + 32] = k
    return t


def step(lib, search):
    """one profiled step over both resident strands -> the figures"""
    lib.profile_reset(); lib.counters_reset()
    t0 = time.perf_counter()
    n = sum(len(search(slot)) for slot in (0, 1))
    wall = (time.perf_counter() - t0) * 1e3
    cn = lib.counters()
    kernels = {k: {"launches": v["launches"], "ms": round(v["ms"], 3)} for k, v in sorted(lib.profile().items()) if v["launches"]}
    return {"wall_ms": round(wall, 2), "hsps": n, "raw_hits": cn["raw_hits"], "kernel_ms": round(sum(v["ms"] for v in kernels.values()), 2), "kernels": kernels}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tlen", type=int, default=50_000_000)
    ap.add_argument("--qlen", type=int, default=50_000_000)
    ap.add_argument("--length", type=int, default=50)
    ap.add_argument("--split", action="store_true", help="expect the two-kernel X-drop path (start the process with LZGPU_FUSED_SCAN=0)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.split and os.environ.get("LZGPU_FUSED_SCAN") != "0":
        sys.exit("--split: start this process with LZGPU_FUSED_SCAN=0")
    lib = lzgpu.Lib()
    lib.init(0)
    t, q = seqio.synth_pair(a.tlen, a.qlen, seed=1000)
    lib.table_prepare(t, lib.seed(), nuc_to_bits(False))
    lib.query_upload(0, q); lib.query_upload(1, seqio.revcomp(q))
    masked, mb = lzo.hoxd70_scoring()[1], nuc_to_bits(True)
    kinds = {"exact": lambda slot: lib.seed_hit_search_exact(mb, a.length, slot=slot),
             "xdrop": lambda slot: lib.seed_hit_search(masked, slot=slot)}
    out = {"tlen": a.tlen, "qlen": a.qlen, "length": a.length, "xdrop_path": "two kernels" if a.split else "fused"}
    lib.profile_enable(True)
    for kind in ("exact", "xdrop", "exact", "xdrop"):               # (the second round is the warm one: every buffer has its size)
        for slot in (0, 1):
            kinds[kind](slot)
        out[kind] = step(lib, kinds[kind])
    lib.shutdown()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")
