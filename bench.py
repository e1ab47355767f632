#!/usr/bin/env python3
"""bench.py -- BASELINE.json metric on MI355X: Gbp of target aligned per second (whole job).

N = 1 (the driver's bench line): workload = BASELINE.json configs[1]: synthetic 50 Mbp target vs 50 Mbp query, default
12-of-19 seed with one transition, --nogapped (the HSP kernel path), both strands.  A step = one complete pass of the
hot path over the batch, inputs already resident in HBM: position-table build from the resident target (B1), then
seed-hit search + X-drop extension of the + strand and of the - strand of the query (B2), HSPs delivered to the host in
the reference's order.  A plain run does only that: set-up, warm-up, the timed steps, --dump-outputs DIR (the HSP lists of the
last timed step, one .npy per strand and field, float64), the line.  Its `roofline` is the dominant kernel's algorithmic bytes /
HIP-event time of the timed steps, `traffic` a replay of the committed PMC table.  With --full the same process adds, outside `value`:
  roofline  k_scan_hits: algorithmic bytes / HIP-event time; `traffic` from THIS run's own rocprofv3 PMC passes (FETCH_SIZE and WRITE_SIZE,
            one pass each over a child process that runs one step), calibrated with the factors tools/fetch_calib.sh measured on known
            byte counts (profiles/fetch_size_calibration.json); --no-pmc replays the committed table instead and says so
  gapped    configs[2]: the same pair through the Y-drop DP (B3, --ydrop=9430): GCUPS, k_ydrop time, its HBM evidence (`roofline`, with PMC
            traffic) and the ceiling it is graded against (`roofline_int_alu`), DP cpu_baseline
  parity    SHA-256 of the HSP list, of the alignments the batch DP returned written out as a LAV (lastz_amd/lav.py), and of the LAV the
            lastz CLI bound to this library writes for this exact pair, against the fingerprints of the pristine reference's output
            (tests/golden/bench50m.sha.json, made by tests/golden/make_bench_sha.py: 2 x 40 minutes of CPU); the batch's alignments
            against the CLI's LAV field by field -- and the CLI's wall clock
  chain     N2: lzgpu_reduce_to_chain_batch (host code) on the pair's HSPs, both strands side by side; one after the other; beside a gapped batch
  cli       the bound lastz on the pair, four runs back to back (first after this process freed its device memory, median, minimum) and
            one after a pause (the definition rounds 1-3 quoted)
  north_star  the same legs on BASELINE.json's north-star pair (200 Mbp x 200 Mbp): seed stage (1 warm-up + 3 timed steps: mean, min,
            median), its own PMC passes, gapped batch, chain clock, one CLI run, parity against tests/golden/bench200m.sha.json
            (--no-north-star skips it)
  content   the seed stage on the same pair with 40 % soft-masked bases + N runs, and with sparse IUPAC codes (scan mode 1)
  cpu_baseline  the pristine reference binary on the box's host cores: 1 core (lastz is single-threaded) and the whole
            host (one process per core over query units, the reference's own scale-out model), on a bounded sample SCALED to the bench
            size (`scaled_sample`), with the reference's full-size wall on this pair (clocked once, on another box) beside it

N > 1 (one process per GPU, torch.distributed / RCCL): workload = BASELINE.json configs[3] in its shape: 200 Mbp target
against 15 query sequences x 2 strands = 30 units, LPT-sharded over the ranks (strong scaling: the job is fixed), the
position table built on rank 0 and broadcast over RCCL/xGMI once per job; every rank searches its units AND runs their gapped
stage (--ydrop=9430) on a second host thread and stream beside the next units' searches, the finished units going down in batches
(lzgpu_gapped_extend_batch; --chain: their HSPs chained first, configs[4]'s shape); HSP lists and alignment digests
gathered and merged on rank 0 in the reference's order.  A step = the whole job.  Before any work every rank checks that its library is
on the device of its LOCAL_RANK and that device 0 was left alone by the others (device_selfcheck).  At configs[3]'s own sizes unit 0 is
the north-star query and its HSP list is checked against the reference's fingerprint inside the line (north_star_unit).
(--q-unit-len / --q-units / --tlen-multi scale it for smoke runs; --bucket-owners splits every unit's search over the ranks by
hashed-diagonal ownership; --force-multi runs this code path on one rank: the N = 1 point of the curve; its cpu_baseline needs --full;
--dump-outputs writes every unit's merged HSP list on rank 0.)

One JSON line on rank 0 (driver contract); extra objects with --full: cpu_baseline, gapped, chain, parity, cli, north_star, content.
"""
import argparse
import collections
import csv
import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec (6.3 TB/s achievable)
# the Y-drop DP's honest ceiling is the integer ALU -- ~12 integer operations per cell on 256 CUs x 64 lanes at
# 2.4 GHz = 3.28 T cells/s -- not the HBM roofline (1 traceback byte per cell)
INT_ALU_PEAK_GCELLS = 256 * 64 * 2.4 / 12.0 * 1.0          # 3276.8 G cells/s
HSP_FMT = "--format=general-:name2,start1,end1,start2,end2,strand2,score"


class _DevMem:
    """raw device pointer -> torch tensor view (zero copy) via __cuda_array_interface__"""
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


_REAL_STDOUT = None


def claim_stdout():
    """The driver's contract is ONE JSON line on stdout.  Native libraries write there too (gloo's "[Gloo] Rank 0 is connected ..." went
    out ahead of the line in round 5): fd 1 is pointed at stderr for the life of the process and emit() writes the line to the
    descriptor that WAS stdout."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.dup(1)
        os.dup2(2, 1)


def emit(obj):
    line = (json.dumps(obj) + "\n").encode()
    sys.stdout.flush()
    os.write(_REAL_STDOUT if _REAL_STDOUT is not None else 1, line)


def _kernel_short(name):
    n = name.split("(")[0]
    if "radix_sort" in n or "onesweep" in n or "histogram" in n:
        return "rocprim:radix_sort"
    if "rocprim" in n:
        return "rocprim:other"
    return n.replace("void ", "").split("<")[0]


def pmc_calibration():
    """counted -> moved bytes, per access pattern, from tools/fetch_calib.sh's run on this hardware (profiles/fetch_size_calibration.json:
    FETCH_SIZE / WRITE_SIZE of kernels whose byte counts are known by construction).  The scan kernel's fetches are 16-byte gathers, two
    per 64-byte line (k_gather16x2); its stores 4-byte non-temporal streams.  Without the file: no correction is claimed."""
    fn = os.path.join(ROOT, "profiles", "fetch_size_calibration.json")
    if not os.path.exists(fn):
        return None
    c = json.load(open(fn))
    try:
        return {"fetch_gather16": c["k_gather16x2"]["factor_fetch"], "fetch_stream16": c["k_stream16"]["factor_fetch"],
                "fetch_stream8_nt": c["k_stream8_nt"]["factor_fetch"], "write_store4_nt": c["k_store4_nt"]["factor_write"],
                "write_store8_nt": c["k_store8_nt"]["factor_write"], "source": "profiles/fetch_size_calibration.json (tools/fetch_calib.sh)"}
    except (KeyError, TypeError):
        return None


def pmc_replay(kernel):
    """HBM-side bytes per launch of `kernel` from the newest COMMITTED PMC table (profiles/*pmc_fetch_write.csv): the fall-back when
    the live passes are not possible (no rocprofv3, --no-pmc); labelled as a replay in the line"""
    import re
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_fetch_write.csv")),
                   key=lambda f: ([int(x) for x in re.findall(r"\d+", os.path.basename(f))], os.path.basename(f)))
    for fn in reversed(files):
        for line in open(fn).read().split("\n")[1:]:
            f = line.split(",")
            if len(f) >= 4 and f[0] == kernel:
                return {"fetch": float(f[2]) * 1024.0, "write": float(f[3]) * 1024.0, "launches": int(f[1]),
                        "source": "replay of profiles/" + os.path.basename(fn) + " (not this run)"}
    return None


def pmc_live(child_args, timeout_s=240):
    """FETCH_SIZE and WRITE_SIZE of every kernel of ONE step of this workload, collected NOW on this box: two rocprofv3 passes
    (--pmc <counter> --kernel-trace, nothing else: the two counters do not fit one pass) over a child process that runs one seed-stage
    step and the gapped batch on the same pair (bench.py --pmc-child).  Counter units are KiB (MI355X_MICROARCH.md).
    -> {kernel: {"fetch": bytes per launch, "write": ..., "launches": n, "fetch_total", "write_total"}} or None"""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None
    out = {}
    d = tempfile.mkdtemp(prefix="lzbench_pmc_", dir="/tmp")
    try:
        for cnt, key in (("FETCH_SIZE", "fetch"), ("WRITE_SIZE", "write")):
            od = os.path.join(d, cnt)
            cmd = [exe, "--pmc", cnt, "--kernel-trace", "--output-format", "csv", "-d", od, "--", sys.executable, os.path.abspath(__file__), "--pmc-child"] + child_args
            try:
                subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s, cwd="/tmp", env={**os.environ, "TMPDIR": "/tmp"})
            except (subprocess.TimeoutExpired, OSError):
                return None
            tot, n = collections.defaultdict(float), collections.Counter()
            for f in glob.glob(os.path.join(od, "**", "*counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if r.get("Counter_Name") == cnt:
                        k = _kernel_short(r["Kernel_Name"])
                        tot[k] += float(r["Counter_Value"]) * 1024.0; n[k] += 1
            if not n:
                return None
            for k in n:
                e = out.setdefault(k, {})
                e[key] = tot[k] / n[k]; e[key + "_total"] = tot[k]; e["launches"] = n[k]
        # a third pass: wave-instructions issued per kernel (VALU / SALU / LDS), for "instructions per DP row" and "per raw hit";
        # the byte counters above stand without it
        od = os.path.join(d, "SQ_INSTS")
        names = ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS")
        cmd = [exe, "--pmc"] + list(names) + ["--kernel-trace", "--output-format", "csv", "-d", od, "--", sys.executable, os.path.abspath(__file__), "--pmc-child"] + child_args
        try:
            subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s, cwd="/tmp", env={**os.environ, "TMPDIR": "/tmp"})
            for f in glob.glob(os.path.join(od, "**", "*counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if r.get("Counter_Name") in names:
                        e = out.setdefault(_kernel_short(r["Kernel_Name"]), {})
                        key = r["Counter_Name"].lower() + "_total"
                        e[key] = e.get(key, 0.0) + float(r["Counter_Value"])
        except (subprocess.TimeoutExpired, OSError):
            pass
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return out


def traffic_fields(kernel, pmc, gather=True, stream_bytes=0.0):
    """the roofline object's traffic keys for `kernel`: live PMC (this run) if there is one, else the committed table, else null.
    traffic = bytes per launch as counted (FETCH_SIZE + WRITE_SIZE); traffic_calibrated = the same with the factors measured for this
    kernel's access patterns on known byte counts (pmc_calibration): on gfx950 a coalesced stream is counted at HALF its bytes whether its
    loads are 16 or 8 bytes wide (factor 2.00), a 16-byte gather at the 64-byte line it moves (0.98-1.00), stores as they are (1.00).  So
    the guide's x2 applies to the kernel's coalesced key stream (`stream_bytes` per launch, known: 8 bytes per hit) and NOT to its window
    gathers -- round 4's blanket x2 implied 7 TB/s."""
    src = None
    e = (pmc or {}).get(kernel) or (pmc or {}).get(kernel + "2")          # (k_fill_hits2 is timed as k_fill_hits)
    if e and "fetch" in e and "write" in e:
        src = "live: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE passes over a child process of this run (one step)"
    else:
        e = pmc_replay(kernel)
        if e:
            src = e["source"]
    if not e:
        return {"traffic": None, "traffic_counted": None, "traffic_calibrated": None, "traffic_source": None}
    cal = pmc_calibration()
    counted = e["fetch"] + e["write"]
    calibrated = None
    if cal:
        ff = cal["fetch_gather16"] if gather else cal["fetch_stream16"]
        fw = cal["write_store4_nt"] if gather else cal["write_store8_nt"]
        fs = cal["fetch_stream8_nt"]
        if ff and fw and fs:
            counted_stream = min(stream_bytes / fs, e["fetch"])          # what the counter shows of the coalesced stream
            calibrated = (e["fetch"] - counted_stream) * ff + counted_stream * fs + e["write"] * fw
    return {"traffic": calibrated if calibrated is not None else counted, "traffic_counted": counted, "traffic_calibrated": calibrated,
            "traffic_fetch_counted": e["fetch"], "traffic_write_counted": e["write"], "traffic_launches_in_pmc_pass": e.get("launches"),
            "traffic_calibration": cal, "traffic_source": src}


def scoring():
    """lastz default scoring (HOXD70; lower case / N / X penalised in the HSP stage), built here without the oracle:
    src/dna_utilities.c:137-148,215-300,497-552 -> (sub, masked, charToBits)"""
    ctb = np.full(256, -1, dtype=np.int8)
    for i, ch in enumerate(b"ACGT"):
        ctb[ch] = i
    sub = np.full((256, 256), -100, dtype=np.int32)
    sub[0, :] = -107374182; sub[:, 0] = -107374182
    for ch in b"Xx":
        sub[ch, :] = -1000; sub[:, ch] = -1000
    hox = [[91, -114, -31, -123], [-114, 100, -125, -31], [-31, -125, 100, -114], [-123, -31, -114, 91]]
    for i, r in enumerate(b"ACGT"):
        for j, c in enumerate(b"ACGT"):
            for rr in (r, r + 32):
                for cc in (c, c + 32):
                    sub[rr, cc] = hox[i][j]
    masked = sub.copy()
    for ch in b"acgtNnX":
        masked[ch, 1:] = -1000
    for ch in b"acgtNnX":
        masked[1:, ch] = -1000
    return sub, masked, ctb


def _ref_clocks(ref, tf, qf, gapped, st):
    t0 = time.time()
    p = subprocess.run([ref, tf, qf, "--ydrop=9430" if gapped else "--nogapped", "--stats=" + st],
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    wall = time.time() - t0
    clocks = {}
    for line in p.stderr.split("\n"):
        if ":" in line:
            k, v = line.rsplit(":", 1)
            try:
                clocks[k.strip()] = float(v.split()[0])
            except (ValueError, IndexError):
                pass
    dp_cells = None
    if gapped and os.path.exists(st):
        for line in open(st):
            if "DP cells visited" in line:
                dp_cells = int(line.split(":")[1].replace(",", ""))
    return clocks, wall, dp_cells


def physical_cores():
    """physical cores this process may run on (SMT siblings counted once)"""
    cpus = os.sched_getaffinity(0)
    seen = set()
    for c in cpus:
        try:
            sib = open("/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list" % c).read().strip()
        except OSError:
            sib = str(c)
        seen.add(sib)
    return max(len(seen), 1)


def cpu_quota():
    """CPUs' worth of run time the container's cgroup grants this process (cpu.max of cgroup v2, cfs quota / period of v1), or None: a box of the
    pool shows 256 hardware threads and an affinity mask of all of them, but `1600000 100000` in cpu.max -- sixteen CPUs -- and that, not the
    128 physical cores, is what "the whole host" can mean for a baseline run there (rounds 3-5 labelled it 128 cores)"""
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else float(q) / float(p)
    except (OSError, ValueError):
        pass
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()); p = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else q / p
    except (OSError, ValueError):
        return None


def cpu_baseline(t, q, qlen_bench, sample_bp, gapped=False, whole_host=True):
    """The pristine reference (oracle/_ref/lastz_stats, built from /root/reference in the build container and shipped
    with the snapshot) on a bounded sample of the same workload: 1 core (lastz is single-threaded), then the whole
    host -- one process per core, each on its own query sample against the same target sample (the reference's
    scale-out model).  Falls back to the oracle port if the binary is absent."""
    from lastz_amd import seqio
    ts, qs = t[:sample_bp], q[:sample_bp]
    ref = os.path.join(ROOT, "oracle", "_ref", "lastz_stats")
    bp2 = float(len(ts)) * float(len(qs)) * 2.0
    if not os.path.exists(ref):
        from oracle import lzo
        _, masked = lzo.hoxd70_scoring()
        t0 = time.time()
        tab = lzo.Table(ts, lzo.seed())
        for qq in (qs, seqio.revcomp(qs)):
            lzo.seed_hit_search(tab, qq, masked)
        sec = time.time() - t0
        return {"value": bp2 / sec / (2.0 * qlen_bench) / 1e9, "unit": "Gbp/s", "cores": 1, "kind": "port",
                "sample": f"first {len(ts)} bp x first {len(qs)} bp, both strands, oracle port ({sec:.2f} s)", "bp2_per_s": bp2 / sec}
    with tempfile.TemporaryDirectory() as d:
        tf, qf, st = os.path.join(d, "t.fa"), os.path.join(d, "q.fa"), os.path.join(d, "st.txt")
        seqio.write_fasta(tf, [("target", ts)]); seqio.write_fasta(qf, [("query", qs)])
        # with --gapped the same run also yields the DP stage's clock and cell count (the table and search
        # clocks do not depend on what follows them)
        clocks, wall, dp_cells = _ref_clocks(ref, tf, qf, gapped, st)
        sec = clocks.get("seed position table", 0.0) + clocks.get("seed hit search", 0.0)
        if sec <= 0:
            sec = wall
        detail = {"seed_position_table_s": clocks.get("seed position table"),
                  "seed_hit_search_s": clocks.get("seed hit search"), "process_wall_s": round(wall, 3)}
        if gapped and dp_cells and clocks.get("gapped extension"):
            detail["gapped"] = {"dp_cells": dp_cells, "gapped_extension_s": clocks["gapped extension"],
                                "gcups": dp_cells / clocks["gapped extension"] / 1e9, "cores": 1}
        host = None
        if whole_host:
            # every physical core runs the --nogapped pipeline on its own query sample (consecutive windows of the bench
            # query) against a smaller target sample: the processes share the memory system, which is what bounds them
            phys, quota = physical_cores(), cpu_quota()
            cores = phys if quota is None else max(1, min(phys, int(quota + 0.5)))     # one process per CPU this container may actually use
            hs = max(sample_bp // 2, 1000)
            hbp2 = float(hs) * float(hs) * 2.0
            th = os.path.join(d, "th.fa")
            seqio.write_fasta(th, [("target", t[:hs])])
            for k in range(cores):
                lo = (k * hs) % max(len(q) - hs, 1)
                seqio.write_fasta(os.path.join(d, "q%d.fa" % k), [("query", q[lo:lo + hs])])
            procs, t0 = [], time.time()
            for k in range(cores):
                procs.append(subprocess.Popen([ref, th, os.path.join(d, "q%d.fa" % k), "--nogapped"],
                                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL))
            for p in procs:
                p.wait()
            hw = time.time() - t0
            rate = cores * hbp2 / hw
            host = {"value": rate / (2.0 * qlen_bench) / 1e9, "unit": "Gbp/s", "cores": cores, "wall_s": round(hw, 2),
                    "host_physical_cores": phys, "cgroup_cpu_quota": quota,
                    "bp2_per_s": rate, "sample": f"{cores} concurrent reference processes (one per CPU the container's cgroup grants this run: quota {quota}, "
                                                 f"{phys} physical cores on the host), each first {hs} bp of target x "
                                                 f"its own {hs} bp window of the query, --nogapped, whole-process wall time"}
    rate_bp2 = bp2 / sec
    # seed work is proportional to Tlen*Qlen: the CPU rate in the metric's unit AT THE BENCH WORKLOAD's query size
    out = {"value": rate_bp2 / (2.0 * qlen_bench) / 1e9, "unit": "Gbp/s", "cores": 1, "kind": "reference",
           "sample": f"first {len(ts)} bp of target x first {len(qs)} bp of query, both strands, "
                     f"{'--ydrop=9430 run, seed-stage clocks' if gapped else '--nogapped'} ({sec:.2f} s of table+search CPU time); "
                     f"scaled by Tlen*Qlen to the bench query size",
           "bp2_per_s": rate_bp2, **detail}
    if host:
        out["whole_host"] = host
    return out


def gather_ceiling(footprint_bytes):
    """TB/s of random 64-byte lines this memory system delivers when every CU gathers inside `footprint_bytes` (the access pattern of
    k_scan_hits' target windows: one random line per raw hit), measured with tools/ub/gather_rate.hip on this hardware and committed as
    profiles/gather_ceiling.json -- the streaming HBM peak is not reachable by a gather.  -> (GB/s, region MiB, source) or None"""
    fn = os.path.join(ROOT, "profiles", "gather_ceiling.json")
    if not os.path.exists(fn):
        return None
    c = json.load(open(fn))
    regs = sorted(c["regions"], key=lambda r: r["mib"])
    pick = next((r for r in regs if r["mib"] * (1 << 20) >= footprint_bytes), regs[-1])
    return pick["lines_TBps_pair"] * 1e3, pick["mib"], c["source"]


def seed_roofline(prof, cnt, K, num_probes, dt, pmc=None, tlen=None):
    """`roofline` object of the seed stage's dominant kernel from the library's HIP-event timer and work counters.
    Algorithmic bytes per step, SURVEY.md 8(d): B_seed = W*(1+4V) + 8H + 4E + X, split over the kernels that do each
    part: the table probes and chain links (count, fill), the bases the X-drop scans touch (phase A = k_scan_hits),
    the diagEnd read / write per hit / extension (phase B = k_settle)."""
    W, Hh, E, X = (cnt[k] / K for k in ("words", "raw_hits", "extensions", "bp_extended"))
    V = num_probes
    alg = {"k_count_hits": W * (1 + 4 * V), "k_fill_hits": 4 * Hh, "k_scan_hits": X, "k_settle2": 4 * Hh + 4 * E}
    b_seed = W * (1 + 4 * V) + 8 * Hh + 4 * E + X
    kern_ms = {k: v["ms"] / K for k, v in prof.items()}
    dom = max((k for k in kern_ms if k in alg), key=lambda k: kern_ms[k], default=None)
    if not dom or not prof[dom]["launches"] or not prof[dom]["ms"]:
        return None
    launches = prof[dom]["launches"] / K
    avg_ms = prof[dom]["ms"] / max(prof[dom]["launches"], 1)
    ach = alg[dom] / launches / (avg_ms * 1e-3) / 1e9
    extra = {}
    if dom == "k_scan_hits" and tlen:
        # what the kernel is actually up against (profiles/r06_k_scan_hits_what_bounds_it.txt): one random 64-byte line of the target's
        # half-overlapping 2-bit blocks (tlen / 2 bytes) per raw hit, against the gather rate the same box reaches on that footprint
        gc = gather_ceiling(tlen / 2.0)
        if gc:
            lines_gbs = 64.0 * Hh / launches / (avg_ms * 1e-3) / 1e9
            extra = {"gather_lines_GBs": lines_gbs, "gather_ceiling_GBs": gc[0], "gather_ceiling_footprint_mib": gc[1], "gather_ceiling_source": gc[2],
                     "frac_of_gather_ceiling": lines_gbs / gc[0]}
    return {"bound": "hbm", "kernel": dom, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": ach / HBM_PEAK_GBS, **extra, **traffic_fields(dom, pmc, stream_bytes=(8.0 * Hh / launches) if dom == "k_scan_hits" else 0.0),
            "algorithmic_bytes_per_launch": alg[dom] / launches, "avg_launch_ms": avg_ms,
            "launches_per_step": launches,
            # whole seed stage against the same roofline, on wall time
            "stage": {"b_seed_bytes_per_step": b_seed, "wall_ms_per_step": dt / K * 1e3,
                      "sum_kernel_ms_per_step": sum(kern_ms.values()),
                      "frac_of_hbm_peak": b_seed / (dt / K) / 1e9 / HBM_PEAK_GBS}}


def hsp_rows_sha(hsps_by_strand):
    """sha256 of the rows `lastz --nogapped --format=general-:name2,start1,end1,start2,end2,strand2,score` prints"""
    h = hashlib.sha256()
    n = 0
    for strand, hs in zip("+-", hsps_by_strand):
        s1 = (hs["pos1"].astype(np.int64) - hs["length"] + 1); e1 = hs["pos1"].astype(np.int64)
        s2 = (hs["pos2"].astype(np.int64) - hs["length"] + 1); e2 = hs["pos2"].astype(np.int64)
        sc = hs["score"].astype(np.int64)
        lines = ["query\t%d\t%d\t%d\t%d\t%s\t%d\n" % (a, b, c, d, strand, e) for a, b, c, d, e in zip(s1, e1, s2, e2, sc)]
        h.update("".join(lines).encode()); n += len(lines)
    return h.hexdigest(), n


DUMP_BUDGET_BYTES = 60_000_000          # --dump-outputs: the arrays' bytes in all (the .npy headers stay well inside 64 MB with them)
HSP_FIELDS = ("pos1", "pos2", "length", "score")


def dump_hsps(dirname, lists):
    """--dump-outputs: HSP lists as a caller of the timed path receives them, [(name, array of lzgpu.HSP_DTYPE)] ->
    DIR/<name>_<field>.npy (float64: exact for the 32-bit fields) and DIR/<name>_rows.npy (the list's full length).  A list longer
    than its share of the budget is written as a fixed, seeded sample of its rows, in list order."""
    os.makedirs(dirname, exist_ok=True)
    cap = (DUMP_BUDGET_BYTES // max(len(lists), 1) - 8) // (8 * len(HSP_FIELDS))
    for name, hs in lists:
        rows = hs
        if len(hs) > cap:
            rows = hs[np.sort(np.random.default_rng(1000).choice(len(hs), cap, replace=False))]
        np.save(os.path.join(dirname, name + "_rows.npy"), np.array([len(hs)], dtype=np.float64))
        for f in HSP_FIELDS:
            np.save(os.path.join(dirname, "%s_%s.npy" % (name, f)), rows[f].astype(np.float64))


def lav_fingerprint(text):
    lines = text.split("\n")
    for i, ln in enumerate(lines):
        if ln.startswith("d {"):
            del lines[i + 1]
            break
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def setup_dist(torch, force_multi=False):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    dist = None
    if world > 1 or force_multi:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:                                  # --force-multi: the N > 1 code path with one rank (the yardstick of the two-rank tests)
            backend = os.environ.get("LZ_BENCH_BACKEND", "nccl")
            rdv = tempfile.NamedTemporaryFile(prefix="lzbench_rdv_", delete=False); rdv.close(); os.unlink(rdv.name)
            kw = {"device_id": torch.device("cuda", local)} if backend == "nccl" else {}
            dist.init_process_group(backend, init_method="file://" + rdv.name, rank=0, world_size=1, **kw)
            return world, rank, local, dist
        # "nccl" is RCCL on ROCm.  LZ_BENCH_BACKEND=gloo exists only to exercise this code path with two
        # ranks on a one-GPU box (RCCL refuses two ranks on the same device); it is not a measured mode.
        backend = os.environ.get("LZ_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    return world, rank, local, dist


def bcast_table(torch, dist, lib, rank, local):
    """the three table buffers of rank 0 into the other ranks' allocations (zero copy over RCCL; staged for gloo)"""
    from lastz_amd import shard
    transport = "rccl" if dist.get_backend() == "nccl" else dist.get_backend() + " (host-staged)"
    for ptr, nbytes in lib.table_buffers():
        if nbytes == 0:
            continue
        if dist.get_backend() == "nccl":
            tt = torch.as_tensor(_DevMem(ptr, nbytes), device=torch.device("cuda", local))
            shard.broadcast_buffers(dist, [tt], src=0)
        else:
            stage = torch.empty(nbytes, dtype=torch.uint8, device=torch.device("cuda", local))
            if rank == 0:
                lib.device_copy(stage.data_ptr(), ptr, nbytes)
            host = stage.cpu()
            dist.broadcast(host, src=0)
            if rank != 0:
                stage.copy_(host)
                torch.cuda.synchronize()
                lib.device_copy(ptr, stage.data_ptr(), nbytes)
    torch.cuda.synchronize()
    return transport


def hsps_to_segs(lzgpu, hs, ident):
    """HSPs as the reporter delivers them (end positions) -> anchor segments (src/segment.h: start positions)"""
    sg = np.zeros(len(hs), dtype=lzgpu.SEG_DTYPE)
    sg["pos1"] = hs["pos1"] - hs["length"]; sg["pos2"] = hs["pos2"] - hs["length"]
    sg["length"] = hs["length"]; sg["s"] = hs["score"]; sg["id"] = ident
    return sg


def measure_pair(torch, lib, lzgpu, target, query, steps, warmup, do_gapped):
    """B1 + B2 (+ the B3 leg) of one (target, query) pair on the resident library: warm-up, `steps` timed steps
    (a step = table rebuild + both strands' searches), then optionally the gapped stage of the same pair.
    -> (record, [HSPs of the + strand, of the - strand])"""
    from lastz_amd import seqio
    sub, masked, ctb = scoring()
    sd = lib.seed("1110100110010101111", 1)
    lib.table_prepare(target, sd, ctb)
    lib.query_upload(0, query)
    lib.query_upload(1, seqio.revcomp(query))
    last = [None, None]

    def step():
        lib.table_rebuild()
        for slot in (0, 1):
            last[slot] = lib.seed_hit_search(masked, slot=slot)

    for _ in range(warmup):
        step()
    lib.profile_enable(True); lib.profile_reset(); lib.counters_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    marks = [t0]
    for _ in range(steps):
        step()
        marks.append(time.perf_counter())               # (a search returns its HSPs: the step is complete when it returns)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    lib.profile_enable(False)
    prof, cnt = lib.profile(), lib.counters()
    K = max(steps, 1)
    tlen, qlen = len(target), len(query)
    step_ms = sorted((b - a) * 1e3 for a, b in zip(marks, marks[1:]))
    rec = {"ms_per_step": dt / K * 1e3, "ms_per_step_min": step_ms[0] if step_ms else None, "ms_per_step_median": step_ms[len(step_ms) // 2] if step_ms else None,
           "value": (tlen / 1e9) / (dt / K), "steps": steps, "warmup": warmup,
           "bp2_per_s": float(tlen) * float(qlen) * 2.0 / (dt / K), "scan_mode": lib.last_scan_mode(),
           "hsps": int(len(last[0]) + len(last[1])),
           "counters_per_step": {k: cnt[k] / K for k in ("words", "raw_hits", "extensions", "bp_extended")},
           "kernel_ms_per_step": {k: v["ms"] / K for k, v in prof.items()},
           "roofline": seed_roofline(prof, cnt, K, sd.num_probes, dt, tlen=tlen)}
    # k_scan_hits against the same roofline whichever kernel dominates (the content legs: byte-code scans)
    if "k_scan_hits" in prof and prof["k_scan_hits"]["launches"]:
        ms = prof["k_scan_hits"]["ms"] / prof["k_scan_hits"]["launches"]
        rec["k_scan_hits"] = {"avg_launch_ms": ms, "frac": cnt["bp_extended"] / prof["k_scan_hits"]["launches"] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
    if not do_gapped:
        return rec, last
    segs = [hsps_to_segs(lzgpu, h, rev) for rev, h in enumerate(last)]
    # ---- N2, --chain: the pair's HSPs chained (a host routine, in the reference and here: src/chain.c:497).  The two strands'
    # problems are independent: lzgpu_reduce_to_chain_batch runs them side by side (host_s); one after the other for comparison
    c0 = time.perf_counter()
    kept1 = [lib.reduce_to_chain(sg)[0] for sg in segs]
    c1 = time.perf_counter()
    kept = [k for k, _ in lib.reduce_to_chain_batch(segs)]
    c2 = time.perf_counter()
    assert all((a_ == b_).all() for a_, b_ in zip(kept, kept1))
    rec["chain"] = {"call": "lzgpu_reduce_to_chain_batch, both strands side by side (host_s); one lzgpu_reduce_to_chain per strand (host_s_one_after_the_other); default penalties (--chain)",
                    "host_s": c2 - c1, "host_s_one_after_the_other": c1 - c0,
                    "anchors": int(len(segs[0]) + len(segs[1])), "kept": int(len(kept[0]) + len(kept[1])),
                    "device": "none (host routine: n dependent steps, each a pruned 2-d tree search of ~0.3 us; DESIGN.md 5 has the estimate of the device alternatives)"}
    # ---- the gapped stage of the same pair (configs[2]: --ydrop=9430)
    probs = lambda: [dict(anchors=segs[slot].copy(), slot=slot, ydrop=9430) for slot in (0, 1)]
    lib.gapped_extend_batch(sub, probs())                                       # warm-up (allocations)
    # strand by strand, as the reference's host loop calls the stage (src/lastz.c:3401-3419) ...
    torch.cuda.synchronize()
    s0 = time.perf_counter()
    for slot in (0, 1):
        lib.gapped_extend(sub, segs[slot].copy(), slot=slot, ydrop=9430)
    torch.cuda.synchronize()
    sdt = time.perf_counter() - s0
    # ... and both strands as one batch (lzgpu_gapped_extend_batch): the same alignments, the launches shared, so
    # that one strand's launch does not sit out the other strand's longest DP
    # (three calls: a call is ~60 ms of which ~20 are host threads -- one sample is at the mercy of whatever else the box does;
    # wall_s is the median, the kernel times and counters are the last call's)
    lib.profile_enable(True)
    gdts = []
    wake = os.environ.get("LZ_BENCH_WAKE", "1") != "0"
    tick = torch.zeros(1 << 20, device="cuda") if wake else None

    def touch_device():
        # A GPU that has idled since the previous call (tens of ms of Python between two calls here) answers its first command after 17-35 ms on
        # this pool (`wall_s_calls` of rounds 5-6: 58-62 ms calls with 77-99 ms ones among them, kernel time identical; LZGPU_HOSTPROF puts the
        # extra time in the first stream synchronisation of the call).  A pipeline that calls the stage back to back never sees that, so the
        # timed calls start from a device that has just run something -- LZ_BENCH_WAKE=0 shows the cold figures.
        if wake:
            for _ in range(8):
                tick.add_(1.0)
        torch.cuda.synchronize()

    for _ in range(3):
        lib.profile_reset(); lib.counters_reset(); lib.dp_longest(reset=True)
        touch_device()
        g0 = time.perf_counter()
        res = lib.gapped_extend_batch(sub, probs())
        torch.cuda.synchronize()
        gdts.append(time.perf_counter() - g0)
    gdt = sorted(gdts)[1]
    nblocks = sum(len(al) for al, _ in res)
    gpr, gc = lib.profile(), lib.counters()
    lib.profile_enable(False)
    # the chain of another query beside this batch (the N > 1 job's B3 thread does exactly this): wall the chaining ADDS
    # (three samples like wall_s: a single call is at the mercy of whatever else the box does -- round 5's driver line had one 77 ms call among
    # 61-62 ms ones in wall_s_calls and a single "beside" sample of +23 ms; the figure is median(beside) - median(alone), all samples in the line)
    bdts = []
    for _ in range(3):
        th = threading.Thread(target=lambda: lib.reduce_to_chain_batch(segs))
        touch_device()
        b0 = time.perf_counter()
        th.start()
        lib.gapped_extend_batch(sub, probs())
        th.join()
        torch.cuda.synchronize()
        bdts.append(time.perf_counter() - b0)
    rec["chain"]["added_wall_s_beside_a_gapped_batch"] = max(sorted(bdts)[1] - gdt, 0.0)
    rec["chain"]["wall_s_calls_beside_a_gapped_batch"] = bdts
    # (the DP kernel has two builds: k_ydrop -- four waves per DP -- and k_ydrop_n -- two waves, 16-bit sweep row --, picked per launch)
    kparts = {k: gpr[k] for k in ("k_ydrop", "k_ydrop_n") if k in gpr}
    kms = {"ms": sum(v["ms"] for v in kparts.values()), "launches": sum(v["launches"] for v in kparts.values())}
    kname = max(kparts, key=lambda k: kparts[k]["ms"]) if kparts else "k_ydrop"          # the build that did most of the call's work
    dpl = lib.dp_longest()
    cells_per_s = (gc["dp_cells"] / (kms["ms"] * 1e-3)) if kms["ms"] else None
    rec["gapped"] = {"wall_s": gdt, "wall_s_min": min(gdts), "wall_s_calls": gdts, "wall_s_strand_by_strand": sdt,
                     "call": "lzgpu_gapped_extend_batch, both strands as one batch (wall_s: the median of three calls, wall_s_calls); one lzgpu_gapped_extend per strand (wall_s_strand_by_strand)",
                     "anchors": int(len(segs[0]) + len(segs[1])), "alignments": nblocks,
                     "anchors_extended": gc["anchors_extended"], "dp_launched": gc["gapped_extensions"], "dp_rows_launched": gc.get("dp_rows"),
                     "dp_cells_reference": gc["dp_cells"], "gcups_wall": gc["dp_cells"] / gdt / 1e9,
                     "k_ydrop_ms": kms["ms"], "k_ydrop_launches": kms["launches"],
                     "k_ydrop_builds": {k: {"ms": v["ms"], "launches": v["launches"]} for k, v in kparts.items()},
                     # a launch lasts as long as its longest DP: shader cycles per row of that DP
                     "longest_dp": {"rows": dpl["rows"], "cells": dpl["cells"],
                                    "cycles_per_row": (dpl["sweep_ticks"] / dpl["rows"]) if dpl["rows"] else None,
                                    "traceback_cycles": dpl["traceback_ticks"]},
                     "kernel_ms": {k: v["ms"] for k, v in gpr.items() if v["ms"]},
                     # algorithmic bytes of the DP, SURVEY 8(d): 1 traceback byte per visited cell -- reported as evidence; the
                     # kernel is GRADED against the integer-ALU ceiling of the same section (roofline_int_alu)
                     "roofline": {"bound": "hbm", "kernel": kname,
                                  "achieved": (cells_per_s / 1e9) if cells_per_s else None,
                                  "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "frac": (cells_per_s / 1e9 / HBM_PEAK_GBS) if cells_per_s else None,
                                  "algorithmic_bytes": gc["dp_cells"], "traffic": None},
                     "roofline_int_alu": {"bound": "int_alu", "kernel": kname, "achieved": (cells_per_s / 1e9) if cells_per_s else None,
                                          "peak": INT_ALU_PEAK_GCELLS, "unit": "Gcells/s",
                                          "frac": (cells_per_s / 1e9 / INT_ALU_PEAK_GCELLS) if cells_per_s else None,
                                          "peak_definition": "SURVEY.md 8(d): ~12 integer operations per DP cell on 256 CUs x 64 lanes x 2.4 GHz"}}
    rec["_gapped_result"] = res
    return rec, last


def attach_traffic(rec, pmc):
    """the PMC bytes of this run's own passes (pmc_live) into the roofline objects of a measure_pair record"""
    if rec.get("roofline"):
        r = rec["roofline"]
        hits_per_launch = rec["counters_per_step"]["raw_hits"] / max(r["launches_per_step"], 1.0)
        r.update(traffic_fields(r["kernel"], pmc, stream_bytes=8.0 * hits_per_launch if r["kernel"] == "k_scan_hits" else 0.0))
        if r.get("traffic"):
            r["traffic_over_algorithmic"] = r["traffic"] / r["algorithmic_bytes_per_launch"]
            r["traffic_GBs"] = r["traffic"] / (r["avg_launch_ms"] * 1e-3) / 1e9
        e = (pmc or {}).get(r["kernel"]) or {}
        if e.get("sq_insts_valu_total") and rec["counters_per_step"]["raw_hits"]:
            # wave-instructions of the dominant kernel per 64 raw hits (one lane per hit): live PMC, the child's one step
            per = 64.0 / rec["counters_per_step"]["raw_hits"]
            r["insts_per_64_hits"] = {k: e.get("sq_insts_%s_total" % k, 0.0) * per for k in ("valu", "salu", "lds")}
    g = rec.get("gapped")
    if g:
        es = [(pmc or {}).get(k) for k in ("k_ydrop", "k_ydrop_n")]
        rows = g.get("dp_rows_launched")
        iv = sum((x or {}).get("sq_insts_valu_total", 0.0) for x in es)
        if rows and iv:
            # VALU / SALU / LDS wave-instructions of the batch's k_ydrop* launches per DP row swept (live PMC: the child's batch = this one)
            g["valu_per_row"] = iv / rows
            g["salu_per_row"] = sum((x or {}).get("sq_insts_salu_total", 0.0) for x in es) / rows
            g["lds_per_row"] = sum((x or {}).get("sq_insts_lds_total", 0.0) for x in es) / rows
        es = [x for x in es if x and "fetch_total" in x and "write_total" in x]
        e = {k: sum(x[k] for x in es) for k in ("fetch_total", "write_total", "launches")} if es else None
        if e:
            # the batch call's k_ydrop launches together (achieved is cells of the call / kernel time of the call)
            g["roofline"].update({"traffic": e["fetch_total"] + e["write_total"], "traffic_fetch_counted": e["fetch_total"], "traffic_write_counted": e["write_total"],
                                  "traffic_launches_in_pmc_pass": e["launches"],
                                  "traffic_source": "live: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE passes over a child process of this run (one gapped batch: every k_ydrop launch of it)"})
        else:
            r = pmc_replay("k_ydrop")
            if r:
                g["roofline"].update({"traffic": (r["fetch"] + r["write"]) * r["launches"], "traffic_source": r["source"] + ", all its k_ydrop launches"})


def cli_leg(seqio, target, query, runs=3, settle_s=0.0):
    """The lastz CLI bound to this library (reference host code + integration/lzgpu_shim.c + liblzgpu.so) on a pair:
    wall clocks of `runs` + 1 stand-alone processes, back to back, and the LAV of the last one.  The first run starts
    right after this process let go of its device buffers (the driver clears what a process frees before it hands it
    out again: a run that starts meanwhile waits in its first large hipMalloc) -- reported on its own; `wall_s` is the
    median of the others.  -> (record, LAV text or None)"""
    gpu_bin = os.path.join(ROOT, "integration", "_build", "lastz_gpu")
    if not os.path.exists(gpu_bin):
        return None, None
    with tempfile.TemporaryDirectory() as d:
        tf, qf = os.path.join(d, "t.fa"), os.path.join(d, "q.fa")
        seqio.write_fasta(tf, [("target", target)]); seqio.write_fasta(qf, [("query", query)])
        walls, out, rc = [], None, 0
        for _ in range(runs + 1):
            c0 = time.time()
            p = subprocess.run([gpu_bin, "t.fa", "q.fa", "--ydrop=9430"], capture_output=True, text=True, cwd=d)
            walls.append(round(time.time() - c0, 3))
            rc = rc or p.returncode
            out = p.stdout
        rest = sorted(walls[1:])
        settled = None
        if settle_s:                                             # round 3's definition of the CLI wall: ONE run after a pause (keep both)
            time.sleep(settle_s)
            c0 = time.time()
            subprocess.run([gpu_bin, "t.fa", "q.fa", "--ydrop=9430"], capture_output=True, text=True, cwd=d)
            settled = round(time.time() - c0, 3)
        rec = {"command": "integration/_build/lastz_gpu t.fa q.fa --ydrop=9430 (reference host code + integration/lzgpu_shim.c + liblzgpu.so)",
               "wall_s": rest[len(rest) // 2], "wall_s_min": rest[0], "wall_s_first_after_free": walls[0], "runs_s": walls,
               "wall_s_definition": "median of the %d runs that follow the first; the first starts right after this process freed its device buffers" % runs,
               "wall_s_after_settle": settled,
               "wall_s_after_settle_definition": ("one more run after a %.0f s pause: rounds 1-3 quoted this" % settle_s) if settle_s else None,
               "rc": rc, "lav_blocks": out.count("\na {") if out else 0}
        return rec, (out if rc == 0 else None)


def golden(name, tlen, qlen):
    gp = os.path.join(ROOT, "tests", "golden", name)
    if os.path.exists(gp):
        g = json.load(open(gp))
        if g["tlen"] == tlen and g["qlen"] == qlen and g["seed"] == 1000:
            return g
    return None


def soft_masked(seq, seed, frac=0.40, n_frac=0.005):
    """`frac` of the bases in lower case (runs of 0.2 - 8 kbp: a soft-masked assembly) and `n_frac` in runs of N"""
    rng = np.random.default_rng(seed)
    s = seq.copy()
    n = len(s)
    mean = 4100.0
    k = max(int(n * frac / mean), 1)
    for st, ln in zip(rng.integers(0, n, k), rng.integers(200, 8000, k)):
        s[st:st + ln] |= 0x20
    k = max(int(n * n_frac / 2500.0), 1)
    for st, ln in zip(rng.integers(0, n, k), rng.integers(100, 5000, k)):
        s[st:st + ln] = ord("N")
    return s


def sparse_iupac(seq, seed, rate=1e-4):
    rng = np.random.default_rng(seed)
    s = seq.copy()
    idx = rng.integers(0, len(s), max(int(len(s) * rate), 1))
    s[idx] = np.frombuffer(b"RYKMSW", dtype=np.uint8)[rng.integers(0, 6, len(idx))]
    return s


def pmc_child(a, lib):
    """bench.py --pmc-child: what pmc_live profiles -- one seed-stage step and one gapped batch of the pair in --pair-file, nothing else"""
    from lastz_amd import lzgpu, seqio
    z = np.load(a.pair_file)
    target, query = z["t"], z["q"]
    sub, masked, ctb = scoring()
    lib.table_prepare(target, lib.seed("1110100110010101111", 1), ctb)
    lib.query_upload(0, query); lib.query_upload(1, seqio.revcomp(query))
    lib.table_rebuild()
    last = [lib.seed_hit_search(masked, slot=slot) for slot in (0, 1)]
    if not a.no_gapped:
        lib.gapped_extend_batch(sub, [dict(anchors=hsps_to_segs(lzgpu, last[slot], slot), slot=slot, ydrop=9430) for slot in (0, 1)])


def pmc_of_pair(a, target, query, timeout_s):
    """this run's own PMC passes over the pair (pmc_live), the pair handed to the child through a file"""
    if a.no_pmc:
        return None
    shm = "/dev/shm" if os.path.isdir("/dev/shm") else "/tmp"
    fn = os.path.join(shm, "lzbench_pair_%d.npz" % os.getpid())
    try:
        np.savez(fn, t=target, q=query)
        return pmc_live(["--pair-file", fn] + (["--no-gapped"] if a.no_gapped else []), timeout_s)
    finally:
        if os.path.exists(fn):
            os.unlink(fn)


def run_single(a, torch, lib):
    from lastz_amd import lzgpu, seqio, lav as lavmod
    target, query = seqio.synth_pair(a.tlen, a.qlen, seed=1000)
    rec, last = measure_pair(torch, lib, lzgpu, target, query, a.steps, a.warmup, a.full and not a.no_gapped)
    if a.dump_outputs:
        dump_hsps(a.dump_outputs, [("hsp_plus", last[0]), ("hsp_minus", last[1])])
    head = {"metric": "Gbp-of-target aligned/sec (whole job, --nogapped HSP path, both strands)",
            "value": rec["value"], "unit": "Gbp/s", "n_gpus": 1, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": rec["ms_per_step"], "ms_per_step_min": rec["ms_per_step_min"], "ms_per_step_median": rec["ms_per_step_median"],
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "s32", "data": "synthetic",
            "config": {"workload": ("BASELINE.json north_star size: " if a.north_star else "BASELINE.json configs[1]: ") +
                                   "synthetic %d bp target vs %d bp query, 12-of-19 seed + 1 transition, "
                                   "--nogapped, both strands" % (a.tlen, a.qlen),
                       "tlen": a.tlen, "qlen": a.qlen, "scan_mode": rec["scan_mode"]},
            "bp2_per_s": rec["bp2_per_s"], "hsps": rec["hsps"],
            "counters_per_step": rec["counters_per_step"],
            "kernel_ms_per_step": rec["kernel_ms_per_step"], "roofline": rec["roofline"]}
    if not a.full:
        emit(head)
        return
    batch_res = rec.pop("_gapped_result", None)
    attach_traffic(rec, pmc_of_pair(a, target, query, 240 if a.tlen <= 60_000_000 else 480))
    gold = golden("bench200m.sha.json" if a.north_star else "bench50m.sha.json", a.tlen, a.qlen)

    # ---- parity of the timed path's output: the reference's HSP list for this exact pair
    parity = {}
    sha, nrows = hsp_rows_sha(last)
    parity["hsp_rows"] = nrows; parity["hsp_sha"] = sha
    parity["hsp_sha_ok"] = (sha == gold["hsp_sha"]) if gold else None
    parity["reference"] = ("tests/golden/%s (pristine lastz 1.04.58 on this pair)" % ("bench200m.sha.json" if a.north_star else "bench50m.sha.json")) if gold else None
    gapped = rec.get("gapped")
    sub_unmasked = scoring()[0]
    if gapped is not None:
        gapped["workload"] = "BASELINE.json configs[2]: same pair, gapped stage, --ydrop=9430, both strands"
        if gold:
            gapped["alignments_ok"] = (gapped["alignments"] == gold["lav_blocks"])
        # The bytes of the call gcups_wall is quoted for (VERDICT r4 #3d): the alignments lzgpu_gapped_extend_batch RETURNED, written out
        # as the reference writes a LAV (lastz_amd/lav.py: every score, begin, end, gap-free piece and identity column, in order) and
        # fingerprinted like the file the pristine reference wrote for this pair -- no CLI, no count
        if batch_res is not None:
            parity["batch_lav_sha"] = lavmod.fingerprint(lavmod.render(target, [query, seqio.revcomp(query)], batch_res, sub_unmasked))
            parity["batch_lav_sha_ok"] = (parity["batch_lav_sha"] == gold["lav_sha"]) if gold else None

    # ---- the non-ideal content (scan modes 1 and 2) on the same pair, perf only (parity: tests/test_gpu_seed.py)
    content = None
    if not a.no_content and not a.north_star:
        content = {}
        for name, f in (("soft_masked_40pct_plus_N_runs", soft_masked), ("sparse_iupac_1e-4", sparse_iupac)):
            r2, _ = measure_pair(torch, lib, lzgpu, f(target, 11), f(query, 12), 2, 1, False)
            content[name] = {k: r2[k] for k in ("ms_per_step", "scan_mode", "hsps", "k_scan_hits")}
            content[name]["kernel_ms_per_step"] = {k: round(v, 2) for k, v in r2["kernel_ms_per_step"].items() if v > 1.0}
            content[name]["raw_hits_per_step"] = r2["counters_per_step"]["raw_hits"]

    # ---- the size BASELINE.json's north_star quotes its targets on, inside the default line
    ns = None
    ns_res = None
    if not a.no_north_star and not a.north_star:
        nt, nq = seqio.synth_pair(200_000_000, 200_000_000, seed=1000)
        r3, l3 = measure_pair(torch, lib, lzgpu, nt, nq, 3, 1, True)
        ns_res = r3.pop("_gapped_result", None)
        attach_traffic(r3, pmc_of_pair(a, nt, nq, 480))       # its own passes at its own size (VERDICT r4 #3c)
        g2 = golden("bench200m.sha.json", len(nt), len(nq))
        sha3, rows3 = hsp_rows_sha(l3)
        ns = {"workload": "BASELINE.json north_star size: synthetic 200000000 bp target vs 200000000 bp query, 12-of-19 seed + 1 transition, both strands; "
                          "1 warm-up + 3 timed steps of the seed stage (ms_per_step = their mean; min and median beside it), then the gapped stage (--ydrop=9430) as one batch",
              **{k: r3[k] for k in ("ms_per_step", "ms_per_step_min", "ms_per_step_median", "value", "bp2_per_s", "hsps", "scan_mode", "counters_per_step", "kernel_ms_per_step", "roofline", "gapped", "chain")},
              "parity": {"hsp_rows": rows3, "hsp_sha": sha3, "hsp_sha_ok": (sha3 == g2["hsp_sha"]) if g2 else None,
                         "alignments_ok": (r3["gapped"]["alignments"] == g2["lav_blocks"]) if g2 else None,
                         "batch_lav_sha_ok": (lavmod.fingerprint(lavmod.render(nt, [nq, seqio.revcomp(nq)], ns_res, sub_unmasked)) == g2["lav_sha"]) if (g2 and ns_res is not None) else None,
                         "reference": "tests/golden/bench200m.sha.json (pristine lastz 1.04.58 on this pair, tests/golden/make_bench200m_sha.py)" if g2 else
                                      "no reference fingerprint committed for this pair: counts cross-checked between the library path and the bound CLI only"}}

    # ---- the lastz CLI bound to this library on the same pair(s): wall clocks + the LAV's fingerprint.  The CLI is a
    # process of its own: this one first lets go of its device buffers (~60 GiB of chunk buffers and DP arenas).
    # The LAV it writes is pinned to the pristine reference's by SHA-256; the alignments lzgpu_gapped_extend_batch returned above --
    # the call `gapped.gcups_wall` is quoted for -- are compared with that LAV FIELD BY FIELD (score, begin, end, every gap-free
    # piece of every block, in order), not by count (VERDICT r4 #3d).
    cli = None
    if not a.no_cli:
        lib.shutdown()
        cli, lav = cli_leg(seqio, target, query, settle_s=5.0)
        if cli is not None and lav is not None:
            fp = lav_fingerprint(lav)
            parity["lav_sha"] = fp
            parity["lav_sha_ok"] = (fp == gold["lav_sha"]) if gold else None
            if batch_res is not None:
                parity["batch_alignments_vs_cli_lav"] = lavmod.compare(batch_res, lav)
            if gold and "reference_wall_s" in gold:
                cli["reference_wall_s_1core"] = gold["reference_wall_s"]["gapped"]
                cli["speedup_vs_reference_cli"] = gold["reference_wall_s"]["gapped"] / cli["wall_s"]
                if cli.get("wall_s_after_settle"):
                    cli["speedup_vs_reference_cli_after_settle"] = gold["reference_wall_s"]["gapped"] / cli["wall_s_after_settle"]
                cli["speedup_vs_reference_cli_first_after_free"] = gold["reference_wall_s"]["gapped"] / cli["wall_s_first_after_free"]
        if ns is not None:
            c2, lav2 = cli_leg(seqio, nt, nq, runs=1)
            if c2 is not None:
                ns["cli"] = c2
                if lav2 is not None:
                    fp2 = lav_fingerprint(lav2)
                    ns["parity"]["lav_sha"] = fp2
                    ns["parity"]["lav_sha_ok"] = (fp2 == g2["lav_sha"]) if g2 else None
                    ns["parity"]["cli_blocks_equal_library_alignments"] = (c2["lav_blocks"] == ns["gapped"]["alignments"])
                    if ns_res is not None:
                        ns["parity"]["batch_alignments_vs_cli_lav"] = lavmod.compare(ns_res, lav2)

    out = {**head, "parity": parity}
    if gapped is not None:
        out["gapped"] = gapped
    if "chain" in rec:
        out["chain"] = rec["chain"]
    if cli is not None:
        out["cli"] = cli
    if ns is not None:
        out["north_star"] = ns
    if content is not None:
        out["content"] = content
    if not a.no_cpu_baseline:
        cb = cpu_baseline(target, query, a.qlen, min(a.cpu_sample, a.tlen, a.qlen), gapped=gapped is not None, whole_host=not a.no_whole_host)
        # which number is which (VERDICT r4 #3e): `value` above is a SCALED SAMPLE (clocked here, on this host); the pristine reference's
        # wall on the full-size pair was clocked once, on the build container's CPU, when the golden fingerprints were made
        cb["scaled_sample"] = True
        if gold and "reference_wall_s" in gold:
            cb["full_size_reference"] = {"wall_s_nogapped": gold["reference_wall_s"]["nogapped"], "wall_s_gapped": gold["reference_wall_s"]["gapped"], "cores": 1,
                                         "value": (a.tlen / 1e9) / gold["reference_wall_s"]["nogapped"], "unit": "Gbp/s",
                                         "clocked": "once, on the build container's CPU (another box), by tests/golden/make_bench_sha.py: whole-process wall of the pristine binary on this exact pair",
                                         "speedup_of_this_line_over_it": rec["value"] / ((a.tlen / 1e9) / gold["reference_wall_s"]["nogapped"])}
        if gapped is not None and "gapped" in cb:
            gapped["cpu_baseline"] = cb.pop("gapped")
            gapped["speedup_vs_cpu_1core"] = gapped["gcups_wall"] / gapped["cpu_baseline"]["gcups"]
            if ns is not None:
                ns["gapped"]["speedup_vs_cpu_1core"] = ns["gapped"]["gcups_wall"] / gapped["cpu_baseline"]["gcups"]
        out["cpu_baseline"] = cb
        out["speedup_vs_cpu_1core"] = rec["value"] / cb["value"] if cb["value"] else None
        if "whole_host" in cb:
            out["speedup_vs_cpu_whole_host"] = rec["value"] / cb["whole_host"]["value"]
    # LAST key of the line (the driver stores the tail of it): configs[2]'s DP figures and the north-star pair's headline numbers
    c2 = {}
    if gapped is not None:
        c2.update({"gcups_wall": gapped["gcups_wall"], "k_ydrop_ms": gapped["k_ydrop_ms"], "frac_hbm": gapped["roofline"]["frac"],
                   "frac_int_alu": gapped["roofline_int_alu"]["frac"], "valu_per_row": gapped.get("valu_per_row"),
                   "alignments_ok": gapped.get("alignments_ok"), "batch_lav_sha_ok": parity.get("batch_lav_sha_ok")})
    chain_keys = ("host_s", "device", "device_s", "added_wall_s_beside_a_gapped_batch")
    if "chain" in rec:
        c2["chain"] = {k: rec["chain"].get(k) for k in chain_keys}
    if ns is not None:
        c2["north_star"] = {"ms_per_step": ns["ms_per_step"], "roofline_frac": ns["roofline"]["frac"], "frac_of_gather_ceiling": ns["roofline"].get("frac_of_gather_ceiling"),
                            "hsp_sha_ok": ns["parity"]["hsp_sha_ok"],
                            "gcups_wall": ns["gapped"]["gcups_wall"], "k_ydrop_ms": ns["gapped"]["k_ydrop_ms"],
                            "valu_per_row": ns["gapped"].get("valu_per_row"),
                            "chain": {k: ns["chain"].get(k) for k in chain_keys}}
    c2["seed"] = {"ms_per_step": rec["ms_per_step"], "roofline_frac": rec["roofline"]["frac"], "frac_of_gather_ceiling": rec["roofline"].get("frac_of_gather_ceiling"),
                  "hsp_sha_ok": parity.get("hsp_sha_ok")}
    out["configs2"] = c2
    emit(out)


def init_with_selfcheck(torch, dist, lib, world, rank, local):
    """Brings the library up on every rank and checks, before any work, what a wrong device binding would break silently (ADVICE r3's
    fix; the test of it skips on a one-GPU box -- VERDICT r4 #5c): (1) every rank's library is bound to device LOCAL_RANK;
    (2) the ranks > 0 did not touch device 0: rank 0 reads its own device's free memory, stays idle while the others initialise the
    library and upload a sequence, and reads it again -- a context or a buffer of another process on device 0 shows as a drop.
    Fails loudly (every rank raises); with ranks that share a device by design (more ranks than devices: the two-rank tests on one GPU)
    only (1) is checked.  -> the record that goes into the bench line"""
    ndev = max(torch.cuda.device_count(), 1)
    shared = world > ndev
    dist.barrier()                                          # (the communicator's own buffers are allocated by the first collective: before the reading)
    free_a = None
    if rank == 0:
        lib.init(local)
        torch.cuda.synchronize()
        free_a = torch.cuda.mem_get_info(local)[0]
    dist.barrier()
    if rank != 0:
        lib.init(local)
        lib.query_upload(1 << 20, np.full(1 << 20, ord("A"), dtype=np.uint8))      # an allocation + a kernel on the rank's device
    dist.barrier()
    moved = None
    if rank == 0:
        moved = int(free_a - torch.cuda.mem_get_info(local)[0])
    info = [None] * world
    dist.all_gather_object(info, {"rank": rank, "local_rank": local, "lzgpu_device_index": int(lib.device_index())})
    bad = [e for e in info if e["lzgpu_device_index"] != e["local_rank"]]
    mv = [moved]
    dist.broadcast_object_list(mv, src=0)
    # (what a rank's library on the wrong device would take: a HIP context and its sequence / chunk buffers, gigabytes; RCCL may map a few
    # tens of MiB of peer buffers on device 0 meanwhile: the figure is reported, the run stops above 512 MiB)
    rec = {"ranks": info, "devices_visible": ndev, "ranks_share_a_device": shared, "device0_free_bytes_moved_while_other_ranks_initialised": mv[0],
           "ok": not bad and (shared or world == 1 or mv[0] is None or mv[0] < (512 << 20))}
    if not rec["ok"]:
        raise RuntimeError("bench.py --gpus %d: device binding self-check failed: %r" % (world, rec))
    return rec


def align_digest(al, op):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(al[["beg1", "beg2", "end1", "end2", "s"]]).tobytes()); h.update(np.ascontiguousarray(op).tobytes())
    return h.hexdigest()


def run_multi(a, torch, lib, world, rank, local, dist, selfcheck=None):
    """configs[3] shape: one target, 15 query sequences x 2 strands sharded over the ranks, table broadcast once per job;
    every unit is searched (B2) and gapped-extended (B3), B3 of unit k beside B2 of unit k+1."""
    import threading
    from lastz_amd import lzgpu, seqio, shard
    sub, masked, ctb = scoring()
    tlen, nu, ulen = a.tlen_multi, a.q_units, a.q_unit_len
    # At configs[3]'s own sizes (200 Mbp target, 200 Mbp units) the target is the north-star pair's and unit 0 its query: the pristine
    # reference's fingerprint of that pair's HSP list (tests/golden/bench200m.sha.json) is then checked INSIDE this job's line
    ns_unit = (tlen == 200_000_000 and ulen == 200_000_000)
    q_ns = None
    if ns_unit:
        target, q_ns = seqio.synth_pair(tlen, ulen, seed=1000)
    else:
        target, _ = seqio.synth_pair(tlen, 64, seed=3000)
    units_all = [(i, s) for i in range(nu) for s in (0, 1)]
    # Fewer units than GPUs (one long query on a node): (sequence, strand) sharding leaves GPUs idle; B2 then shards
    # INSIDE every unit by hashed-diagonal ownership (every rank enumerates, each extends its buckets)
    # and the unit's HSP parts meet on one rank for B3.  With more units than GPUs whole units win: the enumeration
    # (count + fill, a quarter of a search) would be repeated on every rank.
    owners = a.bucket_owners == "always" or (a.bucket_owners == "auto" and len(units_all) < world)
    if owners:
        plan = [[u for k, u in enumerate(units_all) if k % world == r] for r in range(world)]     # who runs B3 of a unit
        mine_search = units_all
    else:
        plan = shard.plan_units([ulen] * nu, world)
        mine_search = plan[rank]
    mine = plan[rank]
    slots = {}
    for qi in sorted({qi for qi, _ in mine_search}):        # this rank's query sequences, homologous to the same target
        q = q_ns if (ns_unit and qi == 0) else seqio.synth_query(target, ulen, seed=3100 + qi)
        for strand in (0, 1):
            if (qi, strand) in mine_search:
                slot = 2 * qi + strand
                lib.query_upload(slot, q if strand == 0 else seqio.revcomp(q))
                slots[(qi, strand)] = slot
        del q
    sd = lib.seed("1110100110010101111", 1)
    if rank == 0:
        lib.table_prepare(target, sd, ctb)
    gb = [bytes(lib.table_geom()) if rank == 0 else None]
    dist.broadcast_object_list(gb, src=0)
    if rank != 0:
        lib.table_adopt(lzgpu.TableGeom.from_buffer_copy(gb[0]))
    if owners:
        lib.set_bucket_owner(world, rank)
    dev = torch.device("cuda", local)
    use_cuda = dist.get_backend() == "nccl"
    merged = [None]; aligned = [None]; transport = [None]
    phase = {"table_build": 0.0, "table_broadcast": 0.0, "search_and_gapped": 0.0, "gather_merge": 0.0}
    busy = {"search_s": 0.0, "gapped_s": 0.0, "chain_s": 0.0, "dp_cells": 0, "b3_batches": 0}
    timeline = []

    def lap(name, t):
        torch.cuda.synchronize()
        now = time.perf_counter(); phase[name] += now - t
        return now

    def step():
        t = time.perf_counter()
        t_step = t
        if rank == 0:
            lib.table_rebuild()
        t = lap("table_build", t)
        transport[0] = bcast_table(torch, dist, lib, rank, local)
        if rank != 0:
            lib.table_commit()
        t = lap("table_broadcast", t)
        del timeline[:]
        res, ali = {}, {}
        # B3 on a second host thread and the library's B3 stream: the units whose search is done wait in a queue and go down TOGETHER
        # (lzgpu_gapped_extend_batch: the DPs of a batch share their launches -- 170-180 GCUPS against 110-145 for one
        # lzgpu_gapped_extend per unit).  A batch is at least the two strands of a sequence unless the search is over.  With --chain the
        # thread first chains the units' HSPs (lzgpu_reduce_to_chain_batch: host code, beside the next unit's search) and extends the chains.
        pending = collections.deque(); cv = threading.Condition(); search_over = [False]; b3_err = []

        def b3_loop():
            try:
                while True:
                    with cv:
                        while len(pending) < 2 and not search_over[0]:
                            cv.wait()
                        if not pending:
                            return
                        batch = [pending.popleft() for _ in range(len(pending))]
                    g0 = time.perf_counter()
                    c0 = lib.counters()["dp_cells"]
                    segs = [hsps_to_segs(lzgpu, hs, u[1]) for u, hs in batch]
                    if a.chain:
                        k0 = time.perf_counter()
                        segs = [sg[kept] for sg, (kept, _) in zip(segs, lib.reduce_to_chain_batch(segs))]
                        busy["chain_s"] += time.perf_counter() - k0
                    out = lib.gapped_extend_batch(sub, [dict(anchors=sg, slot=slots[u], ydrop=9430) for (u, _), sg in zip(batch, segs)])
                    g1 = time.perf_counter()
                    for (u, _), (al, op) in zip(batch, out):
                        ali[u] = (len(al), align_digest(al, op))
                    busy["gapped_s"] += g1 - g0; busy["dp_cells"] += lib.counters()["dp_cells"] - c0; busy["b3_batches"] += 1
                    timeline.append(([list(u) for u, _ in batch], "gapped", round(g0 - t_step, 4), round(g1 - t_step, 4)))
            except Exception as e:                              # (a failure on the thread must fail the step, not hang it)
                b3_err.append(e)

        worker = None
        if not a.no_gapped:
            worker = threading.Thread(target=b3_loop)
            worker.start()
        for u in mine_search:
            s0 = time.perf_counter()
            hs = lib.seed_hit_search(masked, slot=slots[u])
            s1 = time.perf_counter()
            busy["search_s"] += s1 - s0
            timeline.append((list(u), "search", round(s0 - t_step, 4), round(s1 - t_step, 4)))
            if owners:                                      # the unit's parts -> the rank that runs its B3, in discovery order
                dst = units_all.index(u) % world
                parts = [None] * world if rank == dst else None
                dist.gather_object((hs, lib.last_hsp_order(len(hs))), parts, dst=dst)
                if rank != dst:
                    continue
                hs = shard.merge_bucket_owners(parts)
            res[u] = hs
            if worker is not None:
                with cv:
                    pending.append((u, hs)); cv.notify()
        if worker is not None:
            with cv:
                search_over[0] = True; cv.notify()
            worker.join()
            if b3_err:
                raise b3_err[0]
        t = lap("search_and_gapped", t)
        # HSP lists (and the alignments' digests) to rank 0: sizes, then one padded gather; merged in file order, + before -
        flat = np.concatenate([res[u].view(np.uint8) for u in mine]) if mine and sum(len(res[u]) for u in mine) else np.zeros(0, np.uint8)
        sizes = [None] * world
        dist.all_gather_object(sizes, [(u, len(res[u]), ali.get(u)) for u in mine])
        nbytes = [sum(n for _, n, _ in s) * 16 for s in sizes]
        cap = max(max(nbytes), 16)
        buf = torch.zeros(cap, dtype=torch.uint8, device=dev if use_cuda else "cpu")
        if len(flat):
            buf[:len(flat)] = torch.from_numpy(flat).to(buf.device)
        outl = [torch.empty_like(buf) for _ in range(world)] if rank == 0 else None
        dist.gather(buf, outl, dst=0)
        if rank == 0:
            per_rank, per_rank_al = [], []
            for r in range(world):
                arr = outl[r][:nbytes[r]].cpu().numpy().view(lzgpu.HSP_DTYPE)
                d, da, o = {}, {}, 0
                for u, n, al in sizes[r]:
                    d[tuple(u)] = arr[o:o + n]; o += n
                    da[tuple(u)] = al
                per_rank.append(d); per_rank_al.append(da)
            merged[0] = shard.merge_units(per_rank)
            aligned[0] = shard.merge_units(per_rank_al)
        lap("gather_merge", t)

    def fence():
        dist.barrier()
        torch.cuda.synchronize()

    # A step is the whole job (30 units): seconds, not milliseconds.  The step counts the driver asks for are kept
    # unless warm-up + timed steps would run past --time-budget-s; then rank 0 decides on fewer (never fewer than
    # one timed step) from the first warm-up step's duration and every rank follows; the JSON line reports both.
    steps, warmup = max(a.steps, 1), a.warmup
    fence(); w0 = time.perf_counter()
    step()                                              # warm-up step 0 (also the probe for the budget)
    fence(); first = time.perf_counter() - w0
    plan_steps = [steps, max(warmup - 1, 0)]
    if rank == 0 and first * (steps + warmup) > a.time_budget_s:
        plan_steps = [max(1, min(steps, int(a.time_budget_s / first) - 1)), 0]
    dist.broadcast_object_list(plan_steps, src=0)
    steps_run, more_warm = plan_steps
    for _ in range(more_warm):
        step()
    for k in phase:
        phase[k] = 0.0
    busy.update(search_s=0.0, gapped_s=0.0, chain_s=0.0, dp_cells=0, b3_batches=0)
    lib.profile_enable(True); lib.profile_reset(); lib.counters_reset()
    fence()
    t0 = time.perf_counter()
    for _ in range(steps_run):
        step()
    fence()
    dt = time.perf_counter() - t0
    tt = torch.tensor([dt], dtype=torch.float64, device=dev if use_cuda else "cpu")
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    dt = float(tt.item())
    lib.profile_enable(False)
    prof, cnt = lib.profile(), lib.counters()
    K = steps_run
    per_rank_busy = [None] * world
    dist.all_gather_object(per_rank_busy, {"rank": rank, "units": len(mine_search), "search_s": busy["search_s"] / K, "gapped_s": busy["gapped_s"] / K, "chain_s_inside_gapped_s": busy["chain_s"] / K, "b3_batches": busy["b3_batches"] / K,
                                           "gapped_gcups": (busy["dp_cells"] / (busy["gapped_s"] - busy["chain_s"]) / 1e9) if busy["gapped_s"] > busy["chain_s"] else None,
                                           "search_and_gapped_wall_s": phase["search_and_gapped"] / K})
    if rank == 0:
        if a.dump_outputs and merged[0] is not None:
            dump_hsps(a.dump_outputs, [("hsp_q%d_%s" % (qi, "minus" if strand else "plus"), hs) for (qi, strand), hs in merged[0]])
        kern_ms = {k: v["ms"] / K for k, v in prof.items()}
        cb = None
        if a.full and not a.no_cpu_baseline:                # the pristine reference on one host core, bounded sample of the same shape
            qs = seqio.synth_query(target[:a.cpu_sample], min(a.cpu_sample, ulen), seed=3100)
            cb = cpu_baseline(target, qs, a.qlen, min(a.cpu_sample, tlen, len(qs)), gapped=False, whole_host=False)
        nh = sum(len(v) for _, v in merged[0]) if merged[0] else 0
        assert merged[0] is None or [u for u, _ in merged[0]] == units_all
        al_n = al_sha = None
        if not a.no_gapped and aligned[0]:
            assert [u for u, _ in aligned[0]] == units_all
            al_n = sum(v[0] for _, v in aligned[0])
            al_sha = hashlib.sha256("".join(v[1] for _, v in aligned[0]).encode()).hexdigest()
        # unit 0 = the north-star query (at configs[3]'s own sizes): its two strands' HSP lists against the pristine reference's fingerprint
        ns_check = None
        if ns_unit and merged[0]:
            md = dict(merged[0])
            sha0, rows0 = hsp_rows_sha([md[(0, 0)], md[(0, 1)]])
            g2 = golden("bench200m.sha.json", tlen, ulen)
            ns_check = {"unit": 0, "hsp_rows": rows0, "hsp_sha": sha0, "hsp_sha_ok": (sha0 == g2["hsp_sha"]) if g2 else None,
                        "reference": "tests/golden/bench200m.sha.json (pristine lastz 1.04.58 on the north-star pair = this job's target and unit 0)"}
        step_s = dt / K
        tb = (phase["table_build"] + phase["table_broadcast"]) / K
        out = {"metric": "Gbp-of-target aligned/sec (whole job, both strands: HSP search + gapped stage)" if not a.no_gapped else
                         "Gbp-of-target aligned/sec (whole job, --nogapped HSP path, both strands)",
               # the N = 1 line quotes Gbp of target aligned per second against a query of a.qlen bases (configs[1]);
               # here the target meets nu * ulen bases of query per step: the same quantity, i.e. the same
               # bp^2 / s rate, is Tlen * (nu * ulen / a.qlen) / t -- so that the per-N values are comparable
               "value": (tlen / 1e9) * (float(nu) * float(ulen) / float(a.qlen)) / step_s, "unit": "Gbp/s", "n_gpus": world,
               "steps": steps_run, "warmup": 1 + more_warm, "steps_requested": a.steps, "warmup_requested": a.warmup,
               "ms_per_step": step_s * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
               "dtype": "s32", "data": "synthetic",
               "config": {"workload": "BASELINE.json configs[3] shape: synthetic %d bp target vs %d query sequences x %d bp "
                                      "(= %d bp), 12-of-19 seed + 1 transition, both strands%s; a step = the whole job"
                                      % (tlen, nu, ulen, nu * ulen, ", --nogapped" if a.no_gapped else ", gapped stage (--ydrop=9430) of every unit"),
                          "tlen": tlen, "q_units": nu, "q_unit_len": ulen,
                          "value_definition": "Gbp of target aligned per second, normalised to the %d bp query of the N = 1 line "
                                              "(configs[1]): Tlen * (total query bases / %d) / t; target_passes_gbp_per_s is the "
                                              "unnormalised count (q_units * Tlen / t).  The N = 1 line's step is one 50 Mbp pair "
                                              "without the gapped stage: a different workload, not the N = 1 point of this curve "
                                              "(bench.py --gpus 1 --force-multi is)" % (a.qlen, a.qlen),
                          "parallelism": ("%d (sequence x strand) units, every one searched by all %d GPUs (hashed-diagonal ownership inside "
                                          "the unit), B3 of a unit on rank (unit index mod %d)" % (2 * nu, world, world)) if owners else
                                         ("%d (sequence x strand) units LPT-sharded over %d GPUs" % (2 * nu, world)) +
                                         ", position table built on rank 0 and broadcast over RCCL/xGMI once per job, the gapped stage of unit k on a "
                                         "second stream beside the search of unit k+1, HSP lists + alignment digests merged on rank 0"},
               "bp2_per_s": float(tlen) * float(nu) * float(ulen) * 2.0 / step_s,
               "target_passes_gbp_per_s": float(nu) * (tlen / 1e9) / step_s,
               "hsps_merged": int(nh), "alignments": al_n, "alignments_sha": al_sha, "chain": bool(a.chain),
               "device_selfcheck": selfcheck, "north_star_unit": ns_check,
               "units_per_rank": [len(p) for p in plan], "bucket_owners": owners,
               # how the table reached the ranks ("rccl": torch.distributed's nccl backend = RCCL, device buffers in place), and how even the
               # longest-first deal of the units is: the busiest rank's query bases over the mean (1.0 = perfectly even; the job is as long as that rank)
               "table_transport": transport[0], "table_bytes": int(sum(nb for _, nb in lib.table_buffers())),
               "lpt_imbalance": (max(len(p) for p in plan) / (sum(len(p) for p in plan) / float(world))) if sum(len(p) for p in plan) else None,
               # rank 0's clocks of the parts of a step (the table is built and broadcast once per job = once per step)
               "phase_ms_per_step_rank0": {k: v / K * 1e3 for k, v in phase.items()},
               "table_build_and_broadcast_share_of_step": tb / step_s,
               # B3 beside B2: a rank's wall for its units against the sum of the two stages' busy times
               "per_rank": per_rank_busy,
               "overlap": {"rank0_search_busy_s": per_rank_busy[0]["search_s"], "rank0_gapped_busy_s": per_rank_busy[0]["gapped_s"],
                           "rank0_wall_s": per_rank_busy[0]["search_and_gapped_wall_s"],
                           "rank0_wall_over_sum": per_rank_busy[0]["search_and_gapped_wall_s"] / max(per_rank_busy[0]["search_s"] + per_rank_busy[0]["gapped_s"], 1e-9)},
               "timeline_rank0_last_step": sorted(timeline, key=lambda e: e[2]),
               "kernel_ms_per_step_rank0": kern_ms,
               "roofline": seed_roofline(prof, cnt, K, sd.num_probes, dt, tlen=tlen),      # rank 0's launches of the dominant kernel
               "cpu_baseline": cb}
        emit(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tlen", type=int, default=50_000_000)
    ap.add_argument("--qlen", type=int, default=50_000_000)
    ap.add_argument("--full", action="store_true", help="everything beside the headline figure: N = 1: the gapped, chain, parity, PMC, content, "
                                                        "north-star, CLI and CPU-baseline legs; N > 1: the CPU baseline.  The --no-* options "
                                                        "below trim a --full run")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the HSP lists of the last one as DIR/<name>.npy (float64, at most 64 MB in all)")
    ap.add_argument("--cpu-sample", type=int, default=5_000_000)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-whole-host", action="store_true", help="cpu_baseline: the 1-core figure only")
    ap.add_argument("--no-gapped", action="store_true", help="skip the gapped stage (N = 1: the configs[2] leg of --full; N > 1: B3 of every unit)")
    ap.add_argument("--no-cli", action="store_true", help="skip the lastz CLI runs (wall clocks + LAV fingerprint)")
    ap.add_argument("--no-north-star", action="store_true", help="N = 1: skip the 200 Mbp x 200 Mbp object of the --full line")
    ap.add_argument("--no-content", action="store_true", help="N = 1: skip the soft-masked / IUPAC legs (scan modes 1 and 2)")
    ap.add_argument("--gapped", action="store_true", help="(default now; kept for old command lines)")
    ap.add_argument("--tlen-multi", type=int, default=200_000_000, help="N > 1: target length (configs[3]: 200 Mbp)")
    ap.add_argument("--q-units", type=int, default=15, help="N > 1: query sequences (configs[3]: 15)")
    ap.add_argument("--q-unit-len", type=int, default=200_000_000, help="N > 1: bases per query sequence (configs[3]: 200 Mbp)")
    ap.add_argument("--bucket-owners", choices=("auto", "always", "never"), default="auto",
                    help="N > 1: shard B2 inside every unit by hashed-diagonal ownership (auto: when there are fewer units than GPUs)")
    ap.add_argument("--chain", action="store_true", help="N > 1: --chain in front of the gapped stage (configs[4]'s shape): every unit's HSPs chained on the B3 thread, the chain extended")
    ap.add_argument("--force-multi", action="store_true", help="run the N > 1 code path with whatever WORLD_SIZE is (1 included)")
    ap.add_argument("--north-star", action="store_true", help="the whole N = 1 line at BASELINE.json's north_star size (200 Mbp x 200 Mbp; no CLI leg, "
                                                              "1-core CPU baseline only); the --full line carries the same pair as its north_star object")
    ap.add_argument("--no-pmc", action="store_true", help="N = 1: no live rocprofv3 PMC passes (FETCH_SIZE / WRITE_SIZE over a child process); roofline.traffic then replays the committed table")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--pair-file", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--time-budget-s", type=float, default=420.0, help="N > 1: warm-up + timed steps are cut to fit (a step is the whole 3 Gbp job)")
    a = ap.parse_args()
    if a.north_star:
        a.tlen = a.qlen = 200_000_000
        a.no_cli = True; a.no_whole_host = True

    if a.pmc_child:                                # (profiled by pmc_live: no torch, no process group -- the library alone)
        from lastz_amd import lzgpu
        lib = lzgpu.Lib()
        lib.init(int(os.environ.get("LOCAL_RANK", "0")))
        pmc_child(a, lib)
        lib.shutdown()
        return
    claim_stdout()
    import torch                                   # before liblzgpu.so: one HIP runtime per process
    world, rank, local, dist = setup_dist(torch, a.force_multi)
    from lastz_amd import lzgpu
    lib = lzgpu.Lib()
    if dist is None:
        lib.init(local)
        run_single(a, torch, lib)
    else:
        selfcheck = init_with_selfcheck(torch, dist, lib, world, rank, local)
        run_multi(a, torch, lib, world, rank, local, dist, selfcheck)
    lib.shutdown()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
