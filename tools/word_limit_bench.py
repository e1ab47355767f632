"""What the word-count limit costs on the device (lzgpu_table_limit, lzgpu_table_find_limit), beside the calls it stands
next to in a lastz run: lzgpu_table_rebuild, and lzgpu_table_export -- the first half of the route a percentage took before
(the table copied to the host, then walked there on one core).

    python tools/word_limit_bench.py [--tlen 50000000] [--reps 5] [--out FILE.json]

Two targets of --tlen bases under the default 12-of-19 seed: `bench`, bench.py's (uniform random: lists of about three
entries, so limits of 10 and more remove next to nothing), and `repeats`, the same with a tenth of it overwritten by
copies of 300-base units, 20, 200 and 2000 copies of each (lists up to a few thousand entries).  Every figure is the
median of --reps calls, each ended by the library's own synchronisation, in this one process; the limit is lifted
(untimed) before every timed lzgpu_table_limit.  One JSON object per target on stdout, and in --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lastz_amd import lzgpu, seqio                  # noqa: E402

LIMITS = (10, 100, 1000)
KEEPS = (0.5, 0.9, 0.99)


def upper_nuc_to_bits():
    t = np.full(256, -1, dtype=np.int8)
    for k, ch in enumerate(b"ACGT"):
        t[ch] = k
    return t


def with_repeats(t, seed=7):
    """a tenth of t overwritten by runs of copies of random 300-base units: 20, 200 and 2000 copies, in turn"""
    rng = np.random.default_rng(seed)
    t = t.copy()
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    budget, at, k = len(t) // 10, len(t) // 20, 0
    while budget > 0 and at < len(t) - 700_000:
        copies = (20, 200, 2000)[k % 3]
        n = min(300 * copies, budget)
        t[at:at + n] = np.tile(acgt[rng.integers(0, 4, 300)], copies)[:n]
        budget -= n; at += n + 100_000; k += 1
    return t


def median_ms(fn, reps, before=None):
    out = []
    for _ in range(reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(out)[len(out) // 2], 3)


def measure(g, name, t, reps):
    g.table_prepare(t, g.seed(), upper_nuc_to_bits())
    full = g.table_num_words()
    count, words = g.table_count_distribution()
    rec = {"target": name, "tlen": len(t), "table_entries": full, "distinct_list_lengths": len(count), "longest_list": int(count[-1]),
           "table_rebuild_ms": median_ms(g.table_rebuild, reps), "table_limit": {}, "table_find_limit": {}}
    for lim in LIMITS:
        ms = median_ms(lambda: g.table_limit(lim), reps, before=lambda: g.table_limit(0))
        rec["table_limit"][str(lim)] = {"ms": ms, "entries_kept": g.table_num_words()}
    rec["table_limit_lift_ms"] = median_ms(lambda: g.table_limit(0), reps, before=lambda: g.table_limit(LIMITS[0]))
    for keep in KEEPS:
        rec["table_find_limit"][str(keep)] = {"ms": median_ms(lambda: g.table_find_limit(keep), reps), "limit": g.table_find_limit(keep)}
    prev_entries = 1 + len(t)                               # start 0, step 1 (src/pos_table.c:1065)
    rec["table_export_ms"] = median_ms(lambda: g.table_export(prev_entries), reps)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tlen", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = lzgpu.Lib(); g.init()
    t, _ = seqio.synth_pair(a.tlen, 64, seed=1000)          # bench.py's target
    recs = []
    for name, seq in (("bench", t), ("repeats", with_repeats(t))):
        recs.append(measure(g, name, seq, a.reps))
        print(json.dumps(recs[-1]), flush=True)
    g.shutdown()
    if a.out:
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
