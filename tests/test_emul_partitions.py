"""The gapped stage on partitioned sequences, CPU tier: every case of tests/partition_cases.py through the product's host pass
(lz_gapped_host.cpp: partition_limits, add_jobs, trivial_alignments, holds_trivial_candidate) and the product's one-sided DP
(lz_dp_dev.hpp) executed lane by lane (tests/emul/emul_gapped.cpp), against the oracle: alignments, edit scripts, their order,
the DP cells visited and the decline code -- in the default build and in the two-wave / 16-bit-row build."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lastz_amd import lzgpu
import helpers as H
import partition_cases as P
from test_emul_gapped import ARGTYPES

NH_IDENTICAL = 6


def bind(so):
    lib = C.CDLL(so)
    lib.emul_gapped_extend.argtypes = ARGTYPES
    lib.emul_gapped_partitions.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_int]
    lib.emul_gapped_row16_runs.restype = C.c_uint64
    return lib


@pytest.fixture(scope="module")
def L():
    return bind(H.build_emul())


def emul_problem(L, pr, sub, window=1024):
    """one problem of a case through the emulator -> (return code, alignments, ops, stats)"""
    kw = pr["kw"]
    L.emul_gapped_options(int(kw.get("all_bounds", False)), int(kw.get("no_trim", False)))
    s1, s2 = (np.ascontiguousarray([] if x is None else x, dtype=np.uint32) for x in (pr["sep1"], pr["sep2"]))
    L.emul_gapped_partitions(s1.ctypes.data, len(s1), s2.ctypes.data, len(s2), int(kw["strands_differ"]), int(kw.get("inhibit_trivial", False)))
    try:
        t = np.ascontiguousarray(np.append(pr["t"], 0).astype(np.uint8)); q = np.ascontiguousarray(np.append(pr["q"], 0).astype(np.uint8))
        segs = np.ascontiguousarray(pr["segs"].view(lzgpu.SEG_DTYPE).copy())
        out = C.c_void_p(); n = C.c_uint64(); ops = C.c_void_p(); nops = C.c_uint64()
        rc = L.emul_gapped_extend(t.ctypes.data, len(t) - 1, q.ctypes.data, len(q) - 1, sub.ctypes.data, kw.get("gap_open", 400), kw.get("gap_extend", 30),
                                  9400, kw.get("score_thresh", 3000), 0, segs.ctypes.data, len(segs), int(pr["reduce"]), window, 0,
                                  C.byref(out), C.byref(n), C.byref(ops), C.byref(nops))
    finally:
        L.emul_gapped_partitions(None, 0, None, 0, 0, 0)
        L.emul_gapped_options(0, 0)
    if rc:
        return rc, None, None, None
    al = np.zeros(n.value, dtype=lzgpu.ALIGN_DTYPE); op = np.zeros(nops.value, dtype=np.uint32)
    if n.value:
        C.memmove(al.ctypes.data, out, n.value * al.itemsize)
    if nops.value:
        C.memmove(op.ctypes.data, ops, nops.value * 4)
    st = (C.c_uint64 * 8)(); L.emul_gapped_stats(st)
    return 0, al, op, dict(zip(("anchors", "anchors_extended", "dp_runs", "dp_cells", "rounds", "reruns", "retries", "wide_runs"), st))


def check_case(L, name, window=1024):
    """-> the emulator's statistics summed over the strands"""
    c = P.CASES[name]
    sub = P.scoring(name)[0]
    tot, declined = {}, False
    for pr, (oal, oops, ost) in zip(P.problems(name), P.oracle(name)):
        rc, al, ops, st = emul_problem(L, pr, sub, window=window)
        if ost["trivial_candidate"]:                           # the reference decides by the sequences' names: declined
            assert rc == NH_IDENTICAL, (name, pr["strand"], rc)
            declined = True
            continue
        assert rc == 0, (name, pr["strand"], rc)
        assert len(al) == len(oal) and (al == oal).all() and len(ops) == len(oops) and (ops == oops).all(), (name, pr["strand"])
        assert st["dp_cells"] == ost["dp_cells"] and st["anchors_extended"] == ost["anchors_extended"], (name, pr["strand"], st, ost)
        for k, v in st.items():
            tot[k] = tot.get(k, 0) + v
    assert declined == c["declined"], name
    return tot


@pytest.mark.parametrize("name", list(P.CASES))
def test_case_equals_the_oracle(L, name):
    st = check_case(L, name)
    if name == "wide":
        assert st["wide_runs"] > 0


@pytest.mark.parametrize("window", [1, 3])
def test_bounds_across_rounds(L, window):
    """one and three anchors speculated per round: later anchors are bounded by alignments of earlier rounds, of the same
    and of other partitions"""
    st = check_case(L, "bounds", window=window)
    assert st["rounds"] > 3


def test_two_waves_per_dp_and_the_sixteen_bit_row():
    """the build of dp_kernels_narrow.hip (128 lanes per DP, four cells per batch, the 16-bit sweep row on every DP the rule
    admits) on every case, in a process of its own (EMUL_ROW16 is read once)"""
    code = ("import sys\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import helpers as H, partition_cases as P, test_emul_partitions as T\n"
            "lib = T.bind(H.build_emul(tag='n128', flags=['-DLZ_DP_LANES=128', '-DLZ_DP_BATCH=4']))\n"
            "for name in P.CASES:\n"
            "    T.check_case(lib, name)\n"
            "assert lib.emul_gapped_row16_runs() > 100\n"
            "print('row16', lib.emul_gapped_row16_runs())\n" % (H.ROOT, os.path.join(H.ROOT, "tests")))
    env = dict(os.environ); env["EMUL_ROW16"] = "1"
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=H.ROOT, timeout=1500)
    assert p.returncode == 0 and "row16" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
