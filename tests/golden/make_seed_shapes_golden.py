"""Record the seed-shape goldens under tests/golden/ from the PRISTINE reference binary (oracle/_ref/lastz):

    python tests/golden/make_seed_shapes_golden.py

For every case of tests/seed_shape_cases.py (and heavy_blocks, its 300 kbp pair) the case's sequences are written as FASTA
into a temporary directory and
    lastz <pair>_t.fa <pair>_q.fa <the case's seed options> --nogapped --format=general-:name2,start1,end1,start2,end2,strand2,score
is run, the seed given by its command-line name where it has one (--seed=14of22, --seed=match14, ...), else as
--seed=<pattern>; --step and --hspthresh where the case has them.  The output goes to seed_shapes_<case>.tsv; a case
whose output is empty shows nothing and is refused.  tests/test_seed_shapes_oracle.py compares the rows with the oracle.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "lastz")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def names():
    import seed_shape_cases as SC
    return list(SC.CASES) + ["heavy_blocks"]


def pair_of(name):
    import seed_shape_cases as SC
    return SC.HEAVY["seq"] if name == "heavy_blocks" else SC.CASES[name]["seq"]


def options(name):
    import seed_shape_cases as SC
    return SC.lastz_options(SC.HEAVY["case"] if name == "heavy_blocks" else name) + ["--nogapped", SC.GOLDEN_FORMAT]


def write_inputs(d, pairs=None):
    """<pair>_t.fa (record "target") and <pair>_q.fa (record "query") in directory d"""
    from lastz_amd import seqio
    import seed_shape_cases as SC
    for pair in pairs or SC.SEQS:
        t, q = SC.sequences(pair)
        seqio.write_fasta(os.path.join(str(d), pair + "_t.fa"), [("target", t)])
        seqio.write_fasta(os.path.join(str(d), pair + "_q.fa"), [("query", q)])


def run(name, d, binary=REF):
    """stdout of the case's run on the files write_inputs(d) wrote"""
    pair = pair_of(name)
    args = [os.path.join(str(d), pair + "_t.fa"), os.path.join(str(d), pair + "_q.fa")] + options(name)
    return subprocess.check_output([binary] + args, stderr=subprocess.DEVNULL).decode()


def path(name):
    return os.path.join(HERE, "seed_shapes_%s.tsv" % name)


def golden(name):
    return open(path(name)).read()


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        write_inputs(d)
        for name in names():
            out = run(name, d)
            if not out.strip():
                sys.exit("%s prints nothing: drop the case" % name)
            open(path(name), "w").write(out)
            print("%-12s %5d rows  %s" % (name, len(out.splitlines()), " ".join(options(name)[:-2])))
