#!/usr/bin/env python3
"""Record the self-alignment fixtures of tests/test_gpu_self.py with the PRISTINE reference binaries
(oracle/_ref/lastz, oracle/_ref/lastz_stats, built by oracle/Makefile where the reference sources lie).

Run where those binaries exist:   python tools/make_self_golden.py
For every case <name> it writes, under tests/golden/:
  self_<name>.npz         the sequence bytes (`seq`) and the [multi] record lengths (`records`, empty for one record)
  self_<name>.hsp.tsv     the HSP rows of `--self --nogapped --nomirror` in discovery order:
                          name1 start1 end1 name2 start2 end2 strand2 score (contig-relative, 1-based starts)
  self_<name>.stats.json  the run's counters (words, raw seed hits, extensions, bp extended, HSPs)
"""
import json
import os
import subprocess
import sys
import tempfile
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from lastz_amd import seqio  # noqa: E402
from make_golden import parse_stats  # noqa: E402

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


def main():
    out_dir = os.path.join(ROOT, "tests", "golden")
    for name, (seq, records, extra) in cases().items():
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
            st = os.path.join(d, "st.txt")
            subprocess.check_output([REF_STATS] + args + [FMT, "--stats=" + st], stderr=subprocess.DEVNULL)
            stats = parse_stats(open(st).read())
        np.savez_compressed(os.path.join(out_dir, "self_%s.npz" % name), seq=seq, records=np.array(records, dtype=np.int64))
        open(os.path.join(out_dir, "self_%s.hsp.tsv" % name), "wb").write(rows)
        json.dump(stats, open(os.path.join(out_dir, "self_%s.stats.json" % name), "w"), indent=1)
        print(name, len(seq), "bp,", rows.count(b"\n"), "HSPs,", stats)


if __name__ == "__main__":
    main()
