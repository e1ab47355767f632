#!/usr/bin/env python3
"""Record the self-alignment fixtures of tests/test_gpu_self.py and tests/test_self_oracle.py with the PRISTINE
reference binaries (oracle/_ref/lastz, oracle/_ref/lastz_stats, built by oracle/Makefile where the reference sources lie).

Run where those binaries exist:
    python tools/make_self_golden.py                    the cases of tests/self_cases.py that a command line can say
    python tools/make_self_golden.py plain multi band   the three recorded cases of tests/test_gpu_self.py, by name only

For each of the three named cases <name> it writes, under tests/golden/:
  self_<name>.npz         the sequence bytes (`seq`) and the [multi] record lengths (`records`, empty for one record)
  self_<name>.hsp.tsv     the HSP rows of `--self --nogapped --nomirror` in discovery order:
                          name1 start1 end1 name2 start2 end2 strand2 score (contig-relative, 1-based starts)
  self_<name>.stats.json  the run's counters (words, raw seed hits, extensions, bp extended, HSPs)

and for a case of tests/self_cases.py (its sequence is rebuilt from a fixed seed, so none is stored):
  self_<name>.hsp.tsv     the same rows; where they run past 8 KiB, the first and the last 50 only
  self_<name>.stats.json  the counters, and of ALL the rows their number (`rows`) and SHA-256 (`rows_sha256`)
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lastz_amd import seqio  # noqa: E402
from make_golden import parse_stats  # noqa: E402
import self_cases  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "lastz")
REF_STATS = os.path.join(ROOT, "oracle", "_ref", "lastz_stats")
FMT = "--format=general-:name1,start1,end1,name2,start2,end2,strand2,score"


def tandem(n=120_000, seed=9):
    """random sequence with tandem copies (mutated, some reverse-complemented) 0.2-1.8 kbp after their source"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    s = acgt[rng.integers(0, 4, n)]
    at = 2000
    while at < n - 6000:
        ulen = int(rng.integers(300, 1500)); gap = int(rng.integers(200, 1800))
        blk = seqio._mutate(rng, s[at:at + ulen], 0.08, 0.005)
        if rng.random() < 0.3:
            blk = seqio.revcomp(blk)
        d = at + ulen + gap
        s[d:d + len(blk)] = blk[: max(0, min(len(blk), n - d))]
        at = d + len(blk) + int(rng.integers(1000, 6000))
    return s


def cases():
    plain = np.concatenate(seqio.synth_pair(150_000, 150_000, seed=5))
    multi = np.concatenate(seqio.synth_pair(100_000, 110_000, seed=6))
    return {
        "plain": (plain, [], []),
        # three records; the second is short (partitions of very different lengths)
        "multi": (multi, [90_000, 25_000, len(multi) - 115_000], []),
        "band": (tandem(), [], ["--strand=plus", "--band=2000"]),
    }


def run_reference(seq, records, extra, with_stats=True):
    """-> (the rows as the binary wrote them, its counters); records: the lengths of a [multi] file's records, [] for one"""
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "s.fa")
        if records:
            cuts = np.cumsum([0] + records)
            seqio.write_fasta(f, [("r%d" % k, seq[cuts[k]:cuts[k + 1]]) for k in range(len(records))])
            arg = f + "[multi]"
        else:
            seqio.write_fasta(f, [("s", seq)])
            arg = f
        args = [arg, "--self", "--nogapped", "--nomirror"] + extra
        rows = subprocess.check_output([REF] + args + [FMT])
        if not with_stats:
            return rows, None
        st = os.path.join(d, "st.txt")
        subprocess.check_output([REF_STATS] + args + [FMT, "--stats=" + st], stderr=subprocess.DEVNULL)
        return rows, parse_stats(open(st).read())


def matrix_case(name):
    """a case of tests/self_cases.py as run_reference's arguments"""
    c = self_cases.CASES[name]
    _, seps, seq = self_cases.sequence(name)
    records = [seps[k + 1] - seps[k] - 1 for k in range(len(seps) - 1)]
    return seq, records, list(c["cli"])


ROWS_WHOLE = 8 << 10            # rows longer than this are stored as a digest and their two ends
ROWS_ENDS = 50


def stored_rows(rows):
    lines = rows.splitlines(keepends=True)
    return rows if len(rows) <= ROWS_WHOLE else b"".join(lines[:ROWS_ENDS] + lines[-ROWS_ENDS:])


def main():
    out_dir = os.path.join(ROOT, "tests", "golden")
    old = cases() if len(sys.argv) > 1 else {}
    for name in sys.argv[1:]:
        seq, records, extra = old[name]
        rows, stats = run_reference(seq, records, extra)
        np.savez_compressed(os.path.join(out_dir, "self_%s.npz" % name), seq=seq, records=np.array(records, dtype=np.int64))
        open(os.path.join(out_dir, "self_%s.hsp.tsv" % name), "wb").write(rows)
        json.dump(stats, open(os.path.join(out_dir, "self_%s.stats.json" % name), "w"), indent=1)
        print(name, len(seq), "bp,", rows.count(b"\n"), "HSPs,", stats)
    for name in ([] if old else [k for k, c in self_cases.CASES.items() if c["cli"] is not None]):
        assert name not in cases(), name
        seq, records, extra = matrix_case(name)
        rows, stats = run_reference(seq, records, extra)
        stats = {k: stats[k] for k in self_cases.COUNTERS}
        stats["rows"] = rows.count(b"\n")
        stats["rows_sha256"] = hashlib.sha256(rows).hexdigest()
        open(os.path.join(out_dir, "self_%s.hsp.tsv" % name), "wb").write(stored_rows(rows))
        json.dump(stats, open(os.path.join(out_dir, "self_%s.stats.json" % name), "w"), indent=1)
        print(name, len(seq), "bp,", extra, stats)


if __name__ == "__main__":
    main()
