"""Record the seed-hit filter goldens under tests/golden/ from the PRISTINE reference binary (oracle/_ref/lastz):

    python tests/golden/make_filter_golden.py

For every golden case of tests/filter_cases.py the case's sequences are written as FASTA into a temporary directory and
    lastz t.fa q.fa --filter=<...> [--exact=<length> | --mismatch=<count>,<length>] <the case's seed options> --nogapped --format=general-:name1,start1,end1,name2,start2,end2,strand2,score
is run, both strands, with t.fa[multi] where the target has several records.  The output goes to filter_<case>.tsv; a case
whose output is empty shows nothing and is refused.  tests/test_filter_cases.py compares the rows with the CPU statement's.
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
    import filter_cases as FC
    return list(FC.GOLDEN_CASES)


def write_inputs(d, name):
    """<case>_t.fa and <case>_q.fa (record "query") in directory d -> the two file arguments"""
    from lastz_amd import seqio
    import filter_cases as FC
    tf, qf = os.path.join(str(d), name + "_t.fa"), os.path.join(str(d), name + "_q.fa")
    recs = FC.target_records(name)
    seqio.write_fasta(tf, recs)
    seqio.write_fasta(qf, [("query", FC.records(name)[1])])
    return [tf + ("[multi]" if len(recs) > 1 else ""), qf]


def options(name):
    import filter_cases as FC
    return FC.lastz_options(name) + ["--nogapped", FC.GOLDEN_FORMAT]


def run(name, d, binary=REF):
    """stdout of the case's run"""
    return subprocess.check_output([binary] + write_inputs(d, name) + options(name), stderr=subprocess.DEVNULL).decode()


def path(name):
    return os.path.join(HERE, "filter_%s.tsv" % name)


def golden(name):
    return open(path(name)).read()


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        for name in names():
            out = run(name, d)
            if not out.strip():
                sys.exit("%s prints nothing: drop the case" % name)
            open(path(name), "w").write(out)
            print("%-12s %5d rows  %s" % (name, len(out.splitlines()), " ".join(options(name)[:-2])))
