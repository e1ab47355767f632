"""What a seed-hit filter (lastz --filter=2,15, lzgpu_set_hit_filter) costs per kernel, beside the unfiltered X-drop search of
the same pair in the same process:

    python tools/filter_search_bench.py [--tlen 50000000] [--qlen 50000000] [--matches 15] [--transversions 2] [--out FILE.json]

The pair is bench.py's (seqio.synth_pair(tlen, qlen, seed=1000)) under the default 12-of-19 seed, the filter the whole window's
(tests/filter_cases.py, whole_2_15).  Per search kind: one untimed search, then ONE warm step -- both strands, the query strands
resident in slots -- with lzgpu_profile_enable on: every kernel's launches and milliseconds, the wall clock of the step, HSPs,
raw hits and the hits the filter dropped.  The filtered step runs the two-kernel path (a filter needs the key stream between
k_fill_hits and k_scan_hits), the unfiltered one the path the benchmark runs (the fused scan kernel).  `filter_ms_per_chunk`:
k_filter_mark + k_filter_move + the scan of the block counts, per launch of k_fill_hits, beside k_fill_hits' and k_scan_hits'
own.  One JSON object on stdout, and in --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lastz_amd import lzgpu, seqio                  # noqa: E402
from oracle import lzo                              # noqa: E402  (lastz's default scoring matrix only, as bench.py takes it)
from exact_search_bench import nuc_to_bits, step    # noqa: E402


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tlen", type=int, default=50_000_000)
    ap.add_argument("--qlen", type=int, default=50_000_000)
    ap.add_argument("--matches", type=int, default=15)
    ap.add_argument("--transversions", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = lzgpu.Lib()
    lib.init(0)
    t, q = seqio.synth_pair(a.tlen, a.qlen, seed=1000)
    sd = lib.seed()
    lib.table_prepare(t, sd, nuc_to_bits(False))
    lib.query_upload(0, q); lib.query_upload(1, seqio.revcomp(q))
    masked, mb = lzo.hoxd70_scoring()[1], nuc_to_bits(True)
    out = {"tlen": a.tlen, "qlen": a.qlen, "filter": "--filter=%d,%d" % (a.transversions, a.matches)}
    lib.profile_enable(True)
    for kind in ("filtered", "xdrop") * 2:                          # (the second round is the warm one: every buffer has its size)
        if kind == "filtered":
            lib.set_hit_filter(mb, a.matches, a.transversions, (1 << 19) - 1)
        try:
            dropped = 0
            for slot in (0, 1):
                lib.seed_hit_search(masked, slot=slot)
                dropped += lib.last_filter_dropped()
            out[kind] = step(lib, lambda slot: lib.seed_hit_search(masked, slot=slot))
            out[kind]["dropped"] = dropped
        finally:
            lib.set_hit_filter(None)
    k = out["filtered"]["kernels"]
    chunks = k["k_fill_hits"]["launches"]
    out["chunks"] = chunks
    out["filter_ms_per_chunk"] = round((k["k_filter_mark"]["ms"] + k["k_filter_move"]["ms"] + k["rocprim_scan_filter"]["ms"]) / chunks, 3)
    out["k_filter_mark_ms_per_chunk"] = round(k["k_filter_mark"]["ms"] / chunks, 3)
    out["k_filter_move_ms_per_chunk"] = round(k["k_filter_move"]["ms"] / chunks, 3)
    out["k_fill_hits_ms_per_chunk"] = round(k["k_fill_hits"]["ms"] / chunks, 3)
    out["k_scan_hits_ms_per_chunk"] = round(k["k_scan_hits"]["ms"] / chunks, 3)
    out["xdrop_path"] = "two kernels" if "k_fill_hits" in out["xdrop"]["kernels"] else "fused"
    lib.shutdown()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")
