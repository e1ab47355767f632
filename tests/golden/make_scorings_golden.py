"""Generate the goldens of tests/test_scorings.py from the PRISTINE reference binary (oracle/_ref/lastz, built by
oracle/Makefile where the reference's sources lie), for the matrices tests/scorings.py::GOLDEN_MATRICES on the CPU pair of
that file (inputs are rebuilt from the seed there; nothing large is committed):

  scorings_<name>.q        the matrix as a --scores file (settings only), written by scorings.score_file_text
  scorings_<name>.hsp.tsv  `--nogapped` HSPs in discovery order: name2 start1(1-based) end1 start2 end2 strand2 score
  scorings_<name>.lav      the gapped run with the gap / drop parameters of scorings.DP_CASES[<name>]

Run in the build container only:   python tests/golden/make_scorings_golden.py
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from lastz_amd import seqio  # noqa: E402
import scorings as S  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "lastz")
HSP_FORMAT = "--format=general-:name2,start1,end1,start2,end2,strand2,score"


def hsp_args(name, scores):
    _, xdrop, thr, _, _ = S.SEED_CASES[name]
    return ["--scores=" + scores, "--xdrop=%d" % xdrop, "--hspthresh=%d" % thr]


def gapped_args(name):
    kw = S.DP_CASES[name][2]
    return ["--gap=%d,%d" % (kw["gap_open"], kw["gap_extend"]), "--ydrop=%d" % kw["ydrop"], "--gappedthresh=%d" % kw["thresh"]]


def main():
    t, q = seqio.synth_pair(**S.PAIRS["main"][0])
    for name in S.GOLDEN_MATRICES:
        qfile = os.path.join(HERE, "scorings_%s.q" % name)
        open(qfile, "w").write(S.score_file_text(S.MATRICES[name]))
        with tempfile.TemporaryDirectory() as d:
            tf, qf = os.path.join(d, "t.fa"), os.path.join(d, "q.fa")
            seqio.write_fasta(tf, [("target", t)]); seqio.write_fasta(qf, [("query", q)])
            hsp = subprocess.check_output([REF, tf, qf] + hsp_args(name, qfile) + ["--nogapped", HSP_FORMAT])
            open(os.path.join(HERE, "scorings_%s.hsp.tsv" % name), "wb").write(hsp)
            lav = subprocess.check_output([REF, tf, qf] + hsp_args(name, qfile) + gapped_args(name)).decode()
            lav = lav.replace(d + "/", "").replace(HERE + "/", "")
            open(os.path.join(HERE, "scorings_%s.lav" % name), "w").write(lav)
        print(name, len(hsp.split(b"\n")) - 1, "HSPs;", lav.count("a {"), "gapped blocks;", len(lav), "bytes of LAV")


if __name__ == "__main__":
    main()
