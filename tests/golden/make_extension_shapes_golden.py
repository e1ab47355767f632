"""Record the goldens of tests/extension_shape_cases.py under tests/golden/ from the PRISTINE reference binary (oracle/_ref/lastz):

    python tests/golden/make_extension_shapes_golden.py

For every case lastz's command line can say (extension_shape_cases.GOLDEN_CASES: all but the interval table, the masked table and
the lifted limit, which is the unlimited case again) the case's sequences are written as FASTA into a temporary directory and
    lastz t.fa q.fa [--exact=<length> | --mismatch=<count>,<length>] <the seed> [--step=3] [--maxwordcount=<n>] [--filter=<...>] --nogapped --format=general-:name1,start1,end1,name2,start2,end2,strand2,score
is run, both strands, with t.fa[multi] where the target has several records.  The output goes to extshape_<case>.tsv, rows only;
a case whose output is empty shows nothing and is refused.  The command lines themselves go to extension_shapes_index.json, which
the command-line tier on the GPU reads.  tests/test_extension_shapes.py compares rows and command lines with the case table's.
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "lastz")
INDEX = os.path.join(HERE, "extension_shapes_index.json")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def names():
    """the cases with a golden file of their own"""
    import extension_shape_cases as X
    return [n for n in X.GOLDEN_CASES if X.golden_name(n) == n]


def write_inputs(d, name):
    """<pair>_t.fa and <pair>_q.fa (record "query") in directory d -> the two file arguments"""
    from lastz_amd import seqio
    import extension_shape_cases as X
    seq = X.CASES[name]["seq"]
    tf, qf = os.path.join(str(d), seq + "_t.fa"), os.path.join(str(d), seq + "_q.fa")
    recs = X.target_records(name)
    if not os.path.exists(tf):
        seqio.write_fasta(tf, recs)
        seqio.write_fasta(qf, [("query", X.records(name)[1])])
    return [tf + ("[multi]" if len(recs) > 1 else ""), qf]


def options(name):
    import extension_shape_cases as X
    return X.lastz_options(name) + ["--nogapped", X.GOLDEN_FORMAT]


def run(name, d, binary=REF):
    """stdout of the case's run"""
    return subprocess.check_output([binary] + write_inputs(d, name) + options(name), stderr=subprocess.DEVNULL).decode()


def path(name):
    import extension_shape_cases as X
    return os.path.join(HERE, "extshape_%s.tsv" % X.golden_name(name))


def golden(name):
    return open(path(name)).read()


def index():
    """{case: its options as they were when the goldens were recorded}"""
    return json.load(open(INDEX))


if __name__ == "__main__":
    recorded = {}
    with tempfile.TemporaryDirectory() as d:
        for name in names():
            out = run(name, d)
            if not out.strip():
                sys.exit("%s prints nothing: drop the case" % name)
            open(path(name), "w").write(out)
            recorded[name] = options(name)
            print("%-34s %5d rows  %s" % (name, len(out.splitlines()), " ".join(options(name)[:-2])))
    with open(INDEX, "w") as f:
        json.dump(recorded, f, indent=1)
        f.write("\n")
