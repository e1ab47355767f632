"""Cost of dynamic-masking events on a 50 Mbp target (profiles/mask_event_50m.json; DESIGN.md section 1, "Dynamic masking"):

    python tools/mask_event_bench.py [out.json]

Three events in one process -- 1 run of 2000 bases (the process's first call: it also loads the kernels), 40 runs of 300,
3000 runs of 60 -- each as the binding sends it: one lzgpu_table_mask, the 'x' bytes with one lzgpu_target_update per group
of intervals that lie within 64 KiB of each other (and, for comparison, with one per interval), then a search.  Kernel times
are the library's own timer (lzgpu_profile_get), wall times include the calls' synchronisations."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                   # noqa: E402
from lastz_amd import lzgpu, seqio                   # noqa: E402
from oracle import lzo                               # noqa: E402

GAP = 65536


def groups(widened):
    out = []
    for s, e in sorted(widened):
        if out and s <= out[-1][1] + GAP:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def main(path):
    lib = lzgpu.Lib(); lib.init(0)
    t, q = seqio.synth_pair(50_000_000, 20_000, seed=3)
    _, masked = lzo.hoxd70_scoring()
    lib.table_prepare(t, lib.seed(), lzo.upper_nuc_to_bits())
    lib.seed_hit_search(masked, q=q)                 # warm: buffers grown
    rng = np.random.default_rng(1)
    res = {"target_bases": len(t), "entries_before": lib.table_num_words(), "events": [],
           "note": "one process on one MI355X; kernel_ms from the library's kernel timer; the first event also loads the kernels; "
                   "the search after an event runs scan mode 1 (the target holds 'x'), so k_build_wctx does not run"}
    for n, length in ((1, 2000), (40, 300), (3000, 60)):
        starts = np.sort(rng.integers(0, len(t) - length - 40, n))
        cores = [(int(s), int(s) + length) for s in starts]
        widened = [(max(0, s - 18), min(len(t), e + 18)) for s, e in cores]
        for s, e in cores:
            t[s:e] = ord("x")
        lib.profile_reset(); lib.profile_enable(True)
        w0 = time.perf_counter()
        lib.table_mask(widened)
        w1 = time.perf_counter()
        g = groups(widened)
        for s, e in g:
            lib.target_update(s, t[s:e])
        w2 = time.perf_counter()
        for s, e in widened:
            lib.target_update(s, t[s:e])
        w3 = time.perf_counter()
        lib.seed_hit_search(masked, q=q)
        w4 = time.perf_counter()
        prof = lib.profile(); lib.profile_enable(False)
        keep = {k: v for k, v in prof.items() if v["launches"] and k.startswith(("k_mask", "rocprim_scan_mask", "k_build_wctx", "k_encode", "k_pack2", "k_overlap"))}
        res["events"].append({"intervals": n, "core_bases": length, "entries_after": lib.table_num_words(),
                              "copies_grouped": len(g), "bytes_grouped": sum(e - s for s, e in g),
                              "wall_ms": {"table_mask": 1e3 * (w1 - w0), "target_update_grouped": 1e3 * (w2 - w1),
                                          "target_update_per_interval": 1e3 * (w3 - w2), "next_search_20kb_query": 1e3 * (w4 - w3)},
                              "kernel_ms": keep})
        print(json.dumps(res["events"][-1]))
    lib.shutdown()
    json.dump(res, open(path, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mask_event_50m.json"))
