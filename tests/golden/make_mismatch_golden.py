"""Record the N-mismatch goldens under tests/golden/ from the PRISTINE reference binary (oracle/_ref/lastz):

    python tests/golden/make_mismatch_golden.py

For every case of tests/mismatch_cases.py (but `chunks`, which is `spaced` again) the case's sequences are written as FASTA
into a temporary directory and
    lastz t.fa q.fa --mismatch=<M>,<thr> <the case's seed options> --strand=plus --nogapped --format=general-:name1,start1,end1,name2,start2,end2,strand2,score
is run, with t.fa[multi] where the target has several records.  The output goes to mismatch_<case>.tsv; a case whose output
is empty shows nothing and is refused.  tests/test_mismatch_cases.py compares the rows with the serial routine's.
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
    import mismatch_cases as MC
    return list(MC.GOLDEN_CASES)


def write_inputs(d, name):
    """<case>_t.fa and <case>_q.fa (record "query") in directory d -> the two file arguments"""
    from lastz_amd import seqio
    import mismatch_cases as MC
    tf, qf = os.path.join(str(d), name + "_t.fa"), os.path.join(str(d), name + "_q.fa")
    recs = MC.target_records(name)
    seqio.write_fasta(tf, recs)
    seqio.write_fasta(qf, [("query", MC.records(name)[1])])
    return [tf + ("[multi]" if len(recs) > 1 else ""), qf]


def options(name, spelling=0):
    import mismatch_cases as MC
    return MC.lastz_options(name, spelling) + ["--nogapped", MC.GOLDEN_FORMAT]


def run(name, d, binary=REF, spelling=0):
    """stdout of the case's run"""
    return subprocess.check_output([binary] + write_inputs(d, name) + options(name, spelling), stderr=subprocess.DEVNULL).decode()


def path(name):
    return os.path.join(HERE, "mismatch_%s.tsv" % name)


def golden(name):
    return open(path(name)).read()


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        for name in names():
            out = run(name, d)
            if not out.strip():
                sys.exit("%s prints nothing: drop the case" % name)
            open(path(name), "w").write(out)
            print("%-10s %5d rows  %s" % (name, len(out.splitlines()), " ".join(options(name)[:-2])))
