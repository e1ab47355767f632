"""Record the --masking goldens under tests/golden/ from the PRISTINE reference binary (oracle/_ref/lastz):

    python tests/golden/make_masking_golden.py

Target: 60 kbp of random bases.  Queries: 24 reads, the first nine cut from the same 3 kbp of the target (each with its own
2 % of substitutions, every third one reverse-complemented), so that --masking=2 masks that region after the second read and
the later ones find it gone; the next three come from elsewhere in the target and keep their alignments; the last twelve are
short (45 to 70 bases, 8 % substitutions, from elsewhere again): a read that short has few seed hits, and a table of every
20th position (--step=20) misses some of them altogether.  Inputs are written
from fixed seeds into a temporary directory; the outputs of LINES are kept as masking_<name>.<ext>.

So that no line passes vacuously, each is refused here unless, with the pristine binary alone,
  * its output differs from the same line without --masking;
  * at least three (query, strand) events mask something (the x stanzas of the same line in LAV: masking does not depend on
    the output format);
  * a read after the third event still has rows;
  * the --step=20 line differs from the same line without --step.
"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "lastz")
sys.path.insert(0, ROOT)

SEG = ["--nogapped", "--format=segments"]
#        name       arguments                                   file
LINES = {"segments": (["--masking=2"] + SEG,                      "masking_segments.segments"),
         "step20":   (["--masking=2", "--step=20"] + SEG,         "masking_step20.segments"),
         "gapped":   (["--masking=2", "--format=maf-"],           "masking_gapped.maf")}
TLEN, REGION, NREADS = 60000, (20000, 23000), 24


def sequences():
    import numpy as np
    from lastz_amd import seqio
    rng = np.random.default_rng(20240521)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    t = acgt[rng.integers(0, 4, TLEN)].copy()
    reads = []
    for k in range(NREADS):
        if k < 9:
            a = REGION[0] + int(rng.integers(0, 600)); b = REGION[1] - int(rng.integers(0, 600))
        elif k < 12:
            a = 40000 + 4000 * (k - 9); b = a + 2500
        else:
            a = 1000 + 1100 * (k - 12); b = a + 45 + int(rng.integers(0, 26))
        r = t[a:b].copy()
        at = rng.choice(len(r), len(r) // 50 if k < 12 else max(1, (8 * len(r)) // 100), replace=False)
        r[at] = acgt[(np.searchsorted(acgt, r[at]) + rng.integers(1, 4, len(at))) % 4]
        reads.append(("read%02d" % k, seqio.revcomp(r) if k % 3 == 2 else r))
    return t, reads


def write_inputs(d):
    """target.fa and reads.fa in directory d"""
    from lastz_amd import seqio
    t, reads = sequences()
    seqio.write_fasta(os.path.join(str(d), "target.fa"), [("target", t)])
    seqio.write_fasta(os.path.join(str(d), "reads.fa"), reads)


def run(args, d, binary=REF):
    return subprocess.check_output([binary, "target.fa", "reads.fa"] + list(args), cwd=str(d), stderr=subprocess.DEVNULL).decode()


def golden(name):
    return open(os.path.join(HERE, LINES[name][1])).read()


def masked_per_event(args, d):
    """bases masked by every (query, strand) of the line, from the x stanzas of its LAV form"""
    lav = run([a for a in args if not a.startswith("--format")] + ["--format=lav"], d)
    return [int(n) for n in re.findall(r"^x \{\n  n (\d+)\n\}", lav, flags=re.M)]


if __name__ == "__main__":
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/lastz is not built here")
    with tempfile.TemporaryDirectory() as d:
        write_inputs(d)
        for name, (args, fn) in LINES.items():
            out = run(args, d)
            plain = run([a for a in args if not a.startswith("--masking")], d)
            events = masked_per_event(args, d)
            hit = [k for k, n in enumerate(events) if n > 0]
            if out == plain:
                sys.exit("%s: --masking changes nothing" % name)
            if len(hit) < 3:
                sys.exit("%s: only %d events mask something" % (name, len(hit)))
            later = ["read%02d" % k for k in range(hit[2] // 2 + 1, NREADS)]
            if not any(r in out for r in later):
                sys.exit("%s: no read after the third masking event has rows" % name)
            if name == "step20" and out == run([a for a in args if not a.startswith("--step")], d):
                sys.exit("step20: --step=20 changes nothing")
            open(os.path.join(HERE, fn), "w").write(out)
            print("%-9s %5d lines (%d without --masking), %d events mask %d bases, %d bytes -> %s"
                  % (name, len(out.splitlines()), len(plain.splitlines()), len(hit), sum(events), len(out), fn))
