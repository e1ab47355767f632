"""Score matrices other than HOXD70 on the CPU (tests/scorings.py holds the family and says what each member is for):

  * the oracle under three of them against goldens the pristine reference binary wrote (tests/golden/scorings_*, recipe:
    tests/golden/make_scorings_golden.py) and, where oracle/_ref/lastz exists, against a live run;
  * the seed-stage emulator (the kernels' per-lane functions, lz_lut.hpp included) against the oracle on every seed-stage
    row, without and with special bytes, and the scan mode each row takes;
  * the DP emulator against the oracle on every DP row, as is and with the 16-bit sweep row forced on;
  * every entry of the look-up tables lzh_lut_build fills against a plain statement of lz_lut.hpp's header comment, and the
    verdict of lzh_lut_eligible on every row, the one-off neighbours of its limits included."""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import lzo
from lastz_amd import seqio, lzgpu
import helpers as H
import scorings as S
import test_emul_vs_oracle as TE
import test_emul_gapped as TG

G = H.GOLDEN
HSP_FORMAT = "--format=general-:name2,start1,end1,start2,end2,strand2,score"


# ---- the oracle under the family

def oracle_rows(t, q, masked, **kw):
    tab = lzo.Table(t, lzo.seed())
    rows = []
    for strand, _, qq in H.strands(q):
        hsps, _ = lzo.seed_hit_search(tab, qq, masked, **kw)
        rows += H.hsps_as_tsv_rows("query", strand, hsps)
    return rows


def oracle_dp(t, q, sub, masked, xdrop, thr, kw):
    """per strand: (reversed?, query, segments, alignments, ops, stats) of the oracle's search + gapped extension"""
    tab = lzo.Table(t, lzo.seed())
    out = []
    for _, rev, qq in H.strands(q):
        hsps, _ = lzo.seed_hit_search(tab, qq, masked, xdrop=xdrop, hsp_threshold=thr)
        segs = lzo.hsps_to_segments(hsps, rev)
        al, ops, st = lzo.gapped_extend(t, qq, sub, lzo.reduce_to_points(t, qq, sub, segs), gap_open=kw["gap_open"],
                                        gap_extend=kw["gap_extend"], ydrop=kw["ydrop"], score_thresh=kw["thresh"])
        out.append((rev, qq, segs, al, ops, st))
    return out


def oracle_blocks(name):
    """the oracle's LAV blocks for a golden matrix: its seed-stage row's search, its DP row's extension, on the CPU pair"""
    t, q, masked, skw, _ = S.seed_case(name)
    sub, _ = S.m4_scoring(S.MATRICES[name])
    res = oracle_dp(t, q, sub, masked, skw["xdrop"], skw["hsp_threshold"], S.DP_CASES[name][2])
    return [(1, rev, H.blocks_of(al, ops)) for rev, _, _, al, ops, _ in res if len(al)]


@pytest.mark.parametrize("name", S.GOLDEN_MATRICES)
def test_score_file_parses_back_to_the_matrix(name):
    text = open(os.path.join(G, "scorings_%s.q" % name)).read()
    M4, bad, fill = S.parse_score_file(text)
    assert (M4 == S.MATRICES[name]).all() and (bad, fill) == (-1000, -100)
    assert text == S.score_file_text(S.MATRICES[name])
    M = S.MATRICES[name]
    assert all(M[a, b] == M[3 - a, 3 - b] for a in range(4) for b in range(4))
    if name == "eight":
        assert (M != M.T).any() and len({int(M[a, b]) for a in range(4) for b in range(4)}) == 8
    hox, _, _ = S.parse_score_file(open(os.path.join(H.ROOT, "lastz_amd", "data", "HOXD70.q")).read())
    assert (hox == S.HOXD70).all()


@pytest.mark.parametrize("name", S.GOLDEN_MATRICES)
def test_oracle_equals_the_reference_goldens(name):
    t, q, masked, skw, _ = S.seed_case(name)
    rows = oracle_rows(t, q, masked, **skw)
    assert rows == H.read_hsp_tsv(os.path.join(G, "scorings_%s.hsp.tsv" % name))
    assert {r[5] for r in rows} == {"+", "-"}
    blocks = oracle_blocks(name)
    assert blocks == H.lav_blocks(os.path.join(G, "scorings_%s.lav" % name))
    assert sum(len(b[2]) for b in blocks) > 10


@pytest.mark.skipif(lzo.ref_binary() is None, reason="oracle/_ref/lastz not built")
@pytest.mark.parametrize("name", list(S.GOLDEN_MATRICES) + ["x15000", "mis0"])
def test_live_reference_under_the_family(tmp_path, name):
    t, q, masked, skw, _ = S.seed_case(name)
    tf, qf, sf = str(tmp_path / "t.fa"), str(tmp_path / "q.fa"), str(tmp_path / "m.q")
    seqio.write_fasta(tf, [("target", t)]); seqio.write_fasta(qf, [("query", q)])
    open(sf, "w").write(S.score_file_text(S.MATRICES[S.SEED_CASES[name][0]]))
    sargs = [tf, qf, "--scores=" + sf, "--xdrop=%d" % skw["xdrop"], "--hspthresh=%d" % skw["hsp_threshold"]]
    out = H.ref_run(sargs + ["--nogapped", HSP_FORMAT])
    gold = [(f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4]), f[5], int(f[6])) for f in (ln.split("\t") for ln in out.split("\n") if ln)]
    rows = oracle_rows(t, q, masked, **skw)
    assert rows == gold
    assert {r[5] for r in rows} == {"+", "-"}                    # HSPs on both strands
    if name in S.GOLDEN_MATRICES:
        kw = S.DP_CASES[name][2]
        lav = tmp_path / "o.lav"
        lav.write_text(H.ref_run(sargs + ["--gap=%d,%d" % (kw["gap_open"], kw["gap_extend"]), "--ydrop=%d" % kw["ydrop"],
                                          "--gappedthresh=%d" % kw["thresh"]]))
        assert oracle_blocks(name) == H.lav_blocks(str(lav))


# ---- seed-stage emulator

@pytest.fixture(scope="module")
def em():
    return lzgpu.Lib(path=H.build_emul(), prefix="emul_")


@pytest.mark.parametrize("specials", [False, True], ids=["plain", "specials"])
@pytest.mark.parametrize("name", list(S.SEED_CASES))
def test_seed_emulator_equals_the_oracle(em, name, specials):
    t, q, masked, skw, mode = S.seed_case(name, specials=specials)
    TE._check(em, t, q, masked=masked, **skw)
    assert TE._mode(em) == mode


# ---- DP emulator

def emul_dp_row(L, name):
    """one DP row through the emulator against the oracle -> the emulator's stats summed over the strands"""
    t, q, sub, masked, (xdrop, thr), kw, _ = S.dp_case(name)
    tot = {}
    for rev, qq, segs, oal, oops, ost in oracle_dp(t, q, sub, masked, xdrop, thr, kw):
        eal, eops, est = TG.emul_gapped(L, t, qq, sub, segs.view(lzgpu.SEG_DTYPE), **kw)
        assert len(oal) == len(eal) and (oal == eal).all() and (oops == eops).all(), (name, rev)
        assert est["dp_cells"] == ost["dp_cells"] and est["anchors_extended"] == ost["anchors_extended"], (name, rev)
        for k, v in est.items():
            tot[k] = tot.get(k, 0) + v
        tot["aligns"] = tot.get("aligns", 0) + len(oal)
    return tot


def emul_dp_rows_row16(L):
    """(child process under EMUL_ROW16=1) every DP row; which of them ran on the 16-bit row.  A cell out of the 16-bit range
    aborts the process (lz_dp_row16_overflow)"""
    L.emul_gapped_row16_runs.restype = C.c_uint64
    for name, case in S.DP_CASES.items():
        n0 = L.emul_gapped_row16_runs(); st = emul_dp_row(L, name); n1 = L.emul_gapped_row16_runs()
        if case[3] == "row32":
            assert n1 == n0, (name, n0, n1)
        else:
            assert n1 - n0 >= st["dp_runs"] > 0, (name, n0, n1, st)     # every DP (each attempt of one counts) on the 16-bit row
        print("row16", name, n1 - n0, st["dp_runs"], st["wide_runs"])


@pytest.mark.parametrize("name", list(S.DP_CASES))
def test_dp_emulator_equals_the_oracle(name):
    L = C.CDLL(H.build_emul()); L.emul_gapped_extend.argtypes = TG.ARGTYPES
    st = emul_dp_row(L, name)
    assert st["aligns"] > 0 and st["dp_runs"] > 0
    if S.DP_CASES[name][3] == "wide":
        assert st["wide_runs"] > 0


def test_dp_emulator_on_the_sixteen_bit_row():
    """EMUL_ROW16 is read when the library loads: a child process.  The `_last` rows run on the 16-bit row, the `_over` rows never do"""
    code = ("import sys, ctypes as C\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import helpers as H, test_emul_gapped as TG, test_scorings as T\n"
            "lib = C.CDLL(H.build_emul()); lib.emul_gapped_extend.argtypes = TG.ARGTYPES\n"
            "T.emul_dp_rows_row16(lib)\n"
            "print('row16 rows ok')\n" % (H.ROOT, os.path.join(H.ROOT, "tests")))
    env = dict(os.environ); env["EMUL_ROW16"] = "1"
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=H.ROOT, timeout=1500)
    assert p.returncode == 0 and "row16 rows ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


# ---- the look-up tables, entry by entry

@pytest.fixture(scope="module")
def lut():
    d = tempfile.mkdtemp(prefix="emul_lut_")
    so = os.path.join(d, "libemul_lut.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", so, os.path.join(H.ROOT, "tests", "emul", "emul_lut.cpp"),
                           os.path.join(H.ROOT, "lastz_amd", "csrc", "lz_host.cpp")])
    L = C.CDLL(so)
    L.emul_lut_eligible.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.emul_lut_build.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.emul_lut_build.restype = C.c_uint32
    return L


def eligible(L, masked, xdrop):
    ctb = lzo.upper_nuc_to_bits()
    occ = np.zeros(256, dtype=np.uint8); occ[list(b"ACGT")] = 1
    M4 = np.zeros(16, dtype=np.int32)
    m = np.ascontiguousarray(masked, dtype=np.int32)
    return L.emul_lut_eligible(m.ctypes.data, ctb.ctypes.data, occ.ctypes.data, occ.ctypes.data, xdrop, M4.ctypes.data), M4.reshape(4, 4)


def plain_tables(M4, xdrop):
    """lz_lut.hpp's header comment in plain words.  Entry (dir, idx): byte xb = idx & 255 holds x = t ^ q of four bases (Gray
    codes A=0 C=1 G=3 T=2, base j in bits 2j, 2j+1), nibble idx >> 8 the low bit w of the TARGET's Gray code of each.  dir 0
    consumes base 0 first, dir 1 base 3 first.  With P1..P4 the prefix sums of the four scores in consumption order:
    A = max(0, -min Pj), B' = xDrop - max(0, max Pj) as a signed 16-bit number, and the scores as signed bytes, first consumed
    in byte 0."""
    code_of_gray = {0: 0, 1: 1, 3: 2, 2: 3}
    out = np.zeros((2 * 4096, 2), dtype=np.uint32)
    for d in (0, 1):
        for idx in range(4096):
            xb, wn = idx & 255, idx >> 8
            p, ps, sc = 0, [], 0
            for k in range(4):
                j = k if d == 0 else 3 - k
                x, w = (xb >> (2 * j)) & 3, (wn >> j) & 1
                vals = {int(M4[code_of_gray[gt], code_of_gray[gt ^ x]]) for gt in (w, w | 2)}   # the target's two bases with that low bit
                assert len(vals) == 1, "matrix is not invariant under complementing both bases"
                v = vals.pop()
                sc |= (v & 0xFF) << (8 * k)
                p += v; ps.append(p)
            A = max(0, -min(ps)); B = xdrop - max(0, max(ps))
            assert 0 <= A <= 0xFFFF and -32768 <= B <= 32767
            out[d * 4096 + idx] = (A | ((B & 0xFFFF) << 16), sc)
    return out


@pytest.mark.parametrize("name", S.ELIGIBLE)
def test_every_table_entry_against_the_plain_statement(lut, name):
    mname, xdrop, _, _, _ = S.SEED_CASES[name]
    _, masked = S.m4_scoring(S.MATRICES[mname])
    ok, M4 = eligible(lut, masked, xdrop)
    assert ok == 1 and (M4 == S.MATRICES[mname]).all()
    got = np.zeros((2 * 4096, 2), dtype=np.uint32)
    m4 = np.ascontiguousarray(M4.reshape(16), dtype=np.int32)
    assert lut.emul_lut_build(m4.ctypes.data, xdrop, got.ctypes.data) == 2 * 4096
    want = plain_tables(S.MATRICES[mname], xdrop)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])


def test_eligibility_verdict_of_every_row(lut):
    """which rows may use the tables: the table's expected-mode column, with the one-off neighbours of each limit
    (xDrop 380 / 381 under +-127, 2 / 3 under +-1, 15000 / 15001, a score of 127 / 128) and the matrix that is not
    invariant under complementing both bases"""
    for name, (mname, xdrop, _, mode, _) in S.SEED_CASES.items():
        _, masked = S.m4_scoring(S.MATRICES[mname])
        assert eligible(lut, masked, xdrop)[0] == (1 if mode == 0 else 0), name
    by = {k: (v[0], v[1], v[3]) for k, v in S.SEED_CASES.items()}
    assert by["unit"][:2] == ("unit", 3) and by["unit_x2"][:2] == ("unit", 2)
    assert by["ext"][:2] == ("ext", 381) and by["ext_x380"][:2] == ("ext", 380)
    assert by["x15000"][:2] == ("hoxd70", 15000) and by["x15001"][:2] == ("hoxd70", 15001)
    assert S.MATRICES["ext"].max() == 127 and S.MATRICES["ext"].min() == -127 and S.MATRICES["s128"].max() == 128
    _, hm = S.m4_scoring(S.HOXD70)
    assert eligible(lut, hm, 910)[0] == 1 and (S.MATRICES["nonsym"] != S.HOXD70).sum() == 1
