#!/usr/bin/env python3
"""Two ways to run a chores list on the GPU, timed on the bench pair (seqio.synth_pair(50 Mbp, 50 Mbp, seed=1000)) with 100
chores of 1 Mbp x 1 Mbp, plus strand:

  route 1  the table of the whole target, built once; per chore lzgpu_seed_hit_search_within (the lists clipped on the device)
  route 2  per chore lzgpu_table_prepare on the chore's target interval + lzgpu_seed_hit_search over its query interval

    python tools/pos_filter_chores.py [--rounds 3] [--chores 100] [--out profiles/pos_filter_chores_series.json]

Both routes find the same seed hits (the search of a table that holds only the words inside the target interval: DESIGN.md §1,
"Position filter"); the script checks that their HSP lists are equal chore by chore.  The routes run in alternating fresh
child processes, one at a time, each under its own time limit; a child that fails ends the series.  The figure of a
process is the wall time of its loop over the chores, after one untimed chore (the query is resident in both routes;
route 1's one table build is reported beside it, not inside it)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIDE = 1_000_000


def chores(n, tlen, qlen):
    rng = np.random.default_rng(7)
    return [(int(a), int(b)) for a, b in zip(rng.integers(0, tlen - SIDE, n), rng.integers(0, qlen - SIDE, n))]


def child(route, n, pair_file, out):
    from lastz_amd import lzgpu
    from oracle import lzo                                      # (the scoring matrix and the byte map only)
    z = np.load(pair_file)
    t, q = z["t"], z["q"]
    _, masked = lzo.hoxd70_scoring()
    ctb = lzo.upper_nuc_to_bits()
    g = lzgpu.Lib(); g.init(0)
    sd = g.seed()
    g.query_upload(0, q)
    build_s = 0.0
    if route == 1:
        t0 = time.perf_counter(); g.table_prepare(t, sd, ctb); build_s = time.perf_counter() - t0

    def one(ts, qs):
        if route == 1:
            return g.seed_hit_search_within(masked, (ts, ts + SIDE), (qs, qs + SIDE), slot=0)
        g.table_prepare(t, sd, ctb, start=ts, end=ts + SIDE)
        return g.seed_hit_search(masked, slot=0, start=qs, end=qs + SIDE)

    work = chores(n, len(t), len(q))
    one(*work[0])
    res, per = [], []
    t0 = time.perf_counter()
    for ts, qs in work:
        t1 = time.perf_counter(); res.append(one(ts, qs)); per.append(time.perf_counter() - t1)
    loop_s = time.perf_counter() - t0
    g.shutdown()
    np.savez(out, meta=np.array(json.dumps({"route": route, "loop_s": loop_s, "table_build_s": build_s, "chores": n,
                                            "per_chore_ms_median": 1e3 * float(np.median(per)), "hsps": int(sum(len(r) for r in res))})),
             **{"h%d" % k: r for k, r in enumerate(res)})
    print("chores child ok")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--chores", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pos_filter_chores_series.json"))
    ap.add_argument("--tmp", default="/tmp/pos_filter_chores")
    ap.add_argument("--child", nargs=3, metavar=("ROUTE", "PAIR", "OUT"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(int(a.child[0]), a.chores, a.child[1], a.child[2])
    from lastz_amd import seqio
    os.makedirs(a.tmp, exist_ok=True)
    pair_file = os.path.join(a.tmp, "pair.npz")
    t, q = seqio.synth_pair(50_000_000, 50_000_000, seed=1000)
    np.savez(pair_file, t=t, q=q)
    series = {1: [], 2: []}
    first = {}
    for r in range(a.rounds):
        for route in (1, 2):
            out = os.path.join(a.tmp, "r%d_%d.npz" % (route, r))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--chores", str(a.chores), "--child", str(route), pair_file, out],
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0 or "chores child ok" not in p.stdout:
                sys.exit("route %d, round %d failed (exit %s): %s" % (route, r, p.returncode, p.stderr[-2000:]))
            z = np.load(out)
            m = json.loads(str(z["meta"]))
            series[route].append(m)
            hs = [z["h%d" % k] for k in range(a.chores)]
            if route not in first:
                first[route] = hs
            print("round %d route %d: %.3f s for %d chores (median %.2f ms each), table build %.3f s, %d HSPs" %
                  (r, route, m["loop_s"], a.chores, m["per_chore_ms_median"], m["table_build_s"], m["hsps"]), flush=True)
    same = all(len(x) == len(y) and (x == y).all() for x, y in zip(first[1], first[2]))
    doc = {"what": "100 chores of 1 Mbp x 1 Mbp (plus strand) on the 50 Mbp bench pair, alternating fresh processes on one MI355X: tools/pos_filter_chores.py",
           "route_1": "lzgpu_seed_hit_search_within per chore, one table of the whole target", "route_2": "lzgpu_table_prepare on the target interval + lzgpu_seed_hit_search per chore",
           "hsp_lists_equal": bool(same), "series": {"route_1": series[1], "route_2": series[2]}}
    json.dump(doc, open(a.out, "w"), indent=1)
    print("HSP lists equal:", same, "->", a.out)
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
