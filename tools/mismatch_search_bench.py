"""What an N-mismatch search (lastz --mismatch=2,50, lzgpu_seed_hit_search_mismatch) costs per kernel, beside the exact-match
search (--exact=50) and the X-drop search of the same pair in the same process:

    python tools/mismatch_search_bench.py [--tlen 50000000] [--qlen 50000000] [--count 2] [--length 50] [--out FILE.json]

The pair is bench.py's (seqio.synth_pair(tlen, qlen, seed=1000)) under the default 12-of-19 seed.  Per search kind: one
untimed search, then ONE warm step -- both strands, the query strands resident in slots -- with lzgpu_profile_enable on:
every kernel's launches and milliseconds, the wall clock of the step, HSPs and raw hits.  k_scan_mismatch and
k_settle_mismatch stand where k_scan_exact and k_settle_exact do; the X-drop step runs the path the process is on (the
benchmark's fused scan kernel unless it was started with LZGPU_FUSED_SCAN=0; `xdrop_path` says which, from the kernels that
ran).  One JSON object on stdout, and in --out."""
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
    ap.add_argument("--count", type=int, default=2)
    ap.add_argument("--length", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = lzgpu.Lib()
    lib.init(0)
    t, q = seqio.synth_pair(a.tlen, a.qlen, seed=1000)
    lib.table_prepare(t, lib.seed(), nuc_to_bits(False))
    lib.query_upload(0, q); lib.query_upload(1, seqio.revcomp(q))
    masked, mb = lzo.hoxd70_scoring()[1], nuc_to_bits(True)
    kinds = {"mismatch": lambda slot: lib.seed_hit_search_mismatch(mb, a.count, a.length, slot=slot),
             "exact": lambda slot: lib.seed_hit_search_exact(mb, a.length, slot=slot),
             "xdrop": lambda slot: lib.seed_hit_search(masked, slot=slot)}
    out = {"tlen": a.tlen, "qlen": a.qlen, "count": a.count, "length": a.length}
    lib.profile_enable(True)
    for kind in ("mismatch", "exact", "xdrop") * 2:                  # (the second round is the warm one: every buffer has its size)
        for slot in (0, 1):
            kinds[kind](slot)
        out[kind] = step(lib, kinds[kind])
    out["xdrop_path"] = "two kernels" if "k_fill_hits" in out["xdrop"]["kernels"] else "fused"      # (from the kernels that ran: the fused scan enumerates by itself)
    lib.shutdown()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")
