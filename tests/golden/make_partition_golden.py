"""Record the goldens of the partitioned gapped stage under tests/golden/ from the PRISTINE reference binary (oracle/_ref/lastz):

    python tests/golden/make_partition_golden.py

For every case of tests/partition_cases.py that lastz's command line can state, the records of both sequences are written as
FASTA into a temporary directory (t.fa: records t0, t1, ...; q.fa: q0, q1, ...) and the output of
    lastz t.fa[multi] q.fa[multi] --strand=... <the case's flags> --format=general-:name1,zstart1,end1,name2,strand2,zstart2,end2,score,cigar
goes to partition_<case>.tsv as the binary wrote it ([multi] only for a sequence the case partitions).  "DP cells visited" of the
same run of oracle/_ref/lastz_stats goes to partition_stats.json.  tests/test_partition_oracle.py compares both with the oracle,
tests/test_gpu_partitions.py with the library.
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "lastz")
REF_STATS = os.path.join(ROOT, "oracle", "_ref", "lastz_stats")
STATS = os.path.join(HERE, "partition_stats.json")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def arguments(name, d):
    """writes the case's inputs into directory d -> the arguments of the binary"""
    from lastz_amd import seqio
    import partition_cases as P
    import scorings
    c = P.CASES[name]
    files = []
    for fn, recs, nms, parted in zip(("t.fa", "q.fa"), P.records(name), P.names(name), c["parted"]):
        path = os.path.join(str(d), fn)
        seqio.write_fasta(path, list(zip(nms, recs)))
        files.append(path + ("[multi]" if parted else ""))
    scores = os.path.join(str(d), "scores.txt")
    if c["matrix"] is not None:
        open(scores, "w").write(scorings.score_file_text(scorings.MATRICES[c["matrix"]]))
    strand = {("+", "-"): "both", ("+",): "plus", ("-",): "minus"}[tuple(c["strands"])]
    return files + ["--strand=" + strand] + [f.format(scores=scores) for f in c["flags"]] + [P.GOLDEN_FORMAT]


def run(name, d, binary=REF):
    """stdout of the case's run"""
    return subprocess.check_output([binary] + arguments(name, d), stderr=subprocess.DEVNULL).decode()


def cells(name, d, binary=REF_STATS):
    """"DP cells visited" of the case's run of the collect_stats build"""
    from make_golden import parse_stats
    st = os.path.join(str(d), "st.txt")
    subprocess.check_output([binary] + arguments(name, d) + ["--stats=" + st], stderr=subprocess.DEVNULL)
    return parse_stats(open(st).read())["dp_cells"]


def golden(name):
    """-> (the recorded output, the recorded DP cells) of a case"""
    return open(os.path.join(HERE, "partition_%s.tsv" % name)).read(), json.load(open(STATS))[name]


if __name__ == "__main__":
    import partition_cases as P
    stats = {}
    for name in P.GOLDEN:
        with tempfile.TemporaryDirectory() as d:
            out = run(name, d)
            stats[name] = cells(name, d)
        open(os.path.join(HERE, "partition_%s.tsv" % name), "w").write(out)
        print("%-22s %3d rows  %10d cells" % (name, len(out.splitlines()), stats[name]))
    json.dump(stats, open(STATS, "w"), indent=1, sort_keys=True)
