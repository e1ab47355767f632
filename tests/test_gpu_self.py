"""Self-alignment (lastz --self, --band) with the seed search on the device: lzgpu_seed_hit_search_self against the
pristine reference's HSP rows and counters (tests/golden/self_*, recorded by tools/make_self_golden.py) and against
the pristine binary live, and the bound binary (integration/_build/lastz_gpu) against the pristine one, with the
search done on the GPU for every strand.  Needs an MI355X."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import lzo
from lastz_amd import seqio
import helpers as H
from lavparse import normalize_lav

pytestmark = pytest.mark.gpu
CTB = lzo.upper_nuc_to_bits()
GPU_BIN = os.path.join(H.ROOT, "integration", "_build", "lastz_gpu")
REF_BIN = os.path.join(H.ROOT, "oracle", "_ref", "lastz")
FMT = "--format=general-:name1,start1,end1,name2,start2,end2,strand2,score"


def load(name):
    """-> (sequence as lastz holds it, separators or [], record names, golden rows, golden stats, strands)"""
    z = np.load(os.path.join(H.GOLDEN, "self_%s.npz" % name))
    seq, records = z["seq"], [int(x) for x in z["records"]]
    rows = [tuple(l.split("\t")) for l in open(os.path.join(H.GOLDEN, "self_%s.hsp.tsv" % name)).read().splitlines()]
    stats = json.load(open(os.path.join(H.GOLDEN, "self_%s.stats.json" % name)))
    if not records:
        return seq, [], ["s"], rows, stats
    seps, at = [0], 0
    for n in records:
        at += n + 1
        seps.append(at)
    v = np.zeros(at, dtype=np.uint8)                  # NUL, record, NUL, record, ... (src/sequences.c:1896-1931)
    cuts = np.cumsum([0] + records)
    for k in range(len(records)):
        v[seps[k] + 1:seps[k + 1]] = seq[cuts[k]:cuts[k + 1]]
    return v, seps, ["r%d" % k for k in range(len(records))], rows, stats


def minus(v, seps):
    """the reverse strand as lastz makes it: the whole sequence, or every partition on its own"""
    if not seps:
        return seqio.revcomp(v)
    q = v.copy()
    for k in range(len(seps) - 1):
        q[seps[k] + 1:seps[k + 1]] = seqio.revcomp(v[seps[k] + 1:seps[k + 1]])
    return q


def as_rows(hsps, seps, names, strand):
    out = []
    for h in hsps:
        e1, e2, ln = int(h["pos1"]), int(h["pos2"]), int(h["length"])
        if seps:
            i1 = int(np.searchsorted(seps, e1 - ln, side="right")) - 1
            i2 = int(np.searchsorted(seps, e2 - ln, side="right")) - 1
            o1, o2 = seps[i1], seps[i2]
        else:
            i1 = i2 = 0
            o1 = o2 = -1
        # 1-based, inclusive, relative to the record: base x of the sequence is x - o of its record
        out.append((names[i1], str(e1 - ln - o1), str(e1 - 1 - o1), names[i2], str(e2 - ln - o2), str(e2 - 1 - o2),
                    strand, str(int(h["score"]))))
    return out


def self_search(gpu, v, seps, names, band=0, plus_only=False, counters=False):
    masked = H.scoring()[1]
    gpu.table_prepare(v, gpu.seed(), CTB)
    gpu.counters_reset()
    rows = []
    for strand in ("+",) if plus_only else ("+", "-"):
        q = v if strand == "+" else minus(v, seps)
        hs = gpu.seed_hit_search_self(masked, q=q, same_strand=(strand == "+"), band_width=band,
                                      sep1=seps or None, sep2=seps or None)
        rows += as_rows(hs, seps, names, strand)
    return (rows, gpu.counters()) if counters else rows


@pytest.mark.parametrize("name", ["plain", "multi", "band"])
def test_library_rows_and_counters_match_the_reference(gpu, name):
    v, seps, names, want, stats = load(name)
    band = 2000 if name == "band" else 0
    rows, c = self_search(gpu, v, seps, names, band=band, plus_only=(name == "band"), counters=True)
    assert len(want) > 20
    assert rows == want                                                   # discovery order, both strands
    for k in ("raw_hits", "extensions", "bp_extended", "hsps", "words"):
        assert c[k] == stats[k], k


def test_band_drops_what_is_off_the_band(gpu):
    v, seps, names, want, _ = load("band")
    wide = self_search(gpu, v, seps, names, band=0, plus_only=True)
    assert len(wide) > len(want)                                          # the band did drop HSPs of this sequence


def test_small_chunks_same_rows(gpu):
    v, seps, names, want, _ = load("multi")
    try:
        gpu.set_hit_capacity(4096)                                        # ~50 k surviving hits a strand: a dozen chunks
        rows = self_search(gpu, v, seps, names)
    finally:
        gpu.set_hit_capacity(1 << 28)
    assert rows == want


@pytest.mark.parametrize("name", ["plain", "multi"])
def test_plain_search_unchanged_on_the_same_input(gpu, name):
    """lzgpu_seed_hit_search (not self) on the same sequences: still the oracle's HSPs and counters"""
    v, seps, _, _, _ = load(name)
    masked = H.scoring()[1]
    gpu.table_prepare(v, gpu.seed(), CTB)
    tab = lzo.Table(v, lzo.seed())
    for q in (v, minus(v, seps)):
        gpu.counters_reset()
        got = gpu.seed_hit_search(masked, q=q)
        want, st = lzo.seed_hit_search(tab, q, masked)
        assert len(got) == len(want) and (got == want).all()
        c = gpu.counters()
        assert (c["raw_hits"], c["extensions"], c["bp_extended"]) == (st["raw_hits"], st["extensions"], st["bp_extended"])


@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/lastz not built (needs the reference sources at build time)")
def test_library_against_pristine_binary_2mbp(gpu, tmp_path):
    v = np.concatenate(seqio.synth_pair(1_000_000, 1_000_000, seed=13))
    seqio.write_fasta(tmp_path / "s.fa", [("s", v)])
    out = subprocess.run([REF_BIN, str(tmp_path / "s.fa"), "--self", "--nogapped", "--nomirror", FMT],
                         capture_output=True, text=True, timeout=900, check=True).stdout
    want = [tuple(l.split("\t")) for l in out.splitlines()]
    rows = self_search(gpu, v, [], ["s"])
    assert len(want) > 1000 and rows == want


# ---- the bound binary
def run(binary, args, cwd, env_extra=None):
    env = dict(os.environ); env.update(env_extra or {})
    p = subprocess.run([binary] + args, cwd=cwd, capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout, p.stderr


@pytest.fixture(scope="module")
def sandbox(tmp_path_factory):
    d = tmp_path_factory.mktemp("lzself")
    os.makedirs(d / "test_data"); os.makedirs(d / "src")
    import shutil
    shutil.copy(os.path.join(H.GOLDEN, "aglobin.2bit"), d / "test_data" / "aglobin.2bit")
    s = np.concatenate(seqio.synth_pair(400_000, 400_000, seed=21))
    seqio.write_fasta(d / "s.fa", [("s", s)])
    m = np.concatenate(seqio.synth_pair(200_000, 220_000, seed=22))
    seqio.write_fasta(d / "m.fa", [("c1", m[:150_000]), ("c2", m[150_000:170_000]), ("c3", m[170_000:])])
    v, _, _, _, _ = load("band")
    seqio.write_fasta(d / "b.fa", [("b", v)])
    return d


CLI = [(["s.fa", "--self"], 2, "lav"),
       (["s.fa", "--self", "--nomirror"], 2, "lav"),
       (["s.fa", "--self", "--nogapped", "--format=maf"], 2, "maf"),
       (["m.fa[multi]", "--self", "--format=maf"], 2, "maf"),           # ([multi] cannot be written as LAV)
       (["b.fa", "--self", "--strand=plus", "--band=2000"], 1, "lav"),
       (["s.fa", "--self", "--chain"], 2, "lav"),
       (["../test_data/aglobin.2bit/human", "--self"], 2, "lav")]


IDS = ["self", "nomirror", "nogapped-maf", "multi", "band", "chain", "aglobin-human"]
needs_bins = pytest.mark.skipif(not (os.path.exists(GPU_BIN) and os.path.exists(REF_BIN)), reason="integration/_build/lastz_gpu not built")
_runs = {}


def both(sandbox, args):
    """(lastz_gpu stdout, its stderr, pristine stdout), once per command line"""
    key = tuple(args)
    if key not in _runs:
        cwd = sandbox / "src" if args[0].startswith("../") else sandbox
        a, err = run(GPU_BIN, args, cwd, {"LZGPU_VERBOSE": "1"})
        b, _ = run(REF_BIN, args, cwd)
        _runs[key] = (a, err, b)
    return _runs[key]


def binding_binds_self():
    """whether lastz_gpu was linked from a shim that sends --self searches to lzgpu_seed_hit_search_self.  The shim can
    only be compiled where the reference sources are; elsewhere integration/Makefile restores the binaries stashed in
    oracle/_ref/ by an earlier build, which may predate the binding (they then run --self on the reference's routine)."""
    return b"lzgpu_seed_hit_search_self" in open(GPU_BIN, "rb").read()


@needs_bins
@pytest.mark.parametrize("args,strands,fmt", CLI, ids=IDS)
def test_cli_self_same_bytes(sandbox, args, strands, fmt):
    a, _, b = both(sandbox, args)
    strip = lambda s: "\n".join(l for l in s.split("\n") if not l.startswith("#"))
    norm = normalize_lav if fmt == "lav" else (lambda s: s)
    assert strip(norm(a)) == strip(norm(b))
    assert len(a) > 500


@needs_bins
@pytest.mark.skipif(os.path.exists(GPU_BIN) and not binding_binds_self(),
                    reason="integration/_build/lastz_gpu predates the --self binding (restored from oracle/_ref/ without the reference sources to rebuild it)")
@pytest.mark.parametrize("args,strands,fmt", CLI, ids=IDS)
def test_cli_self_search_on_gpu(sandbox, args, strands, fmt):
    _, err, _ = both(sandbox, args)
    assert err.count("[lzgpu] search: done on the GPU") == strands, err[-2000:]
    assert "[lzgpu] search: reference path" not in err and "[lzgpu] search: declined" not in err
    assert "table: copied to the host for a reference routine" not in err, err[-2000:]
