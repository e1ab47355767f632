"""Record the --maxwordcount goldens under tests/golden/ from the PRISTINE reference binary (oracle/_ref/lastz):

    python tests/golden/make_word_limit_golden.py

Target rep20 (tests/self_cases.py), both strands, inputs written as FASTA into a temporary directory; the output of
    lastz rep20.fa <query>.fa [--maxwordcount=<n> | --maxwordcount=<p>%] --nogapped --format=segments
for the query rep with the limits GOLDEN_LIMITS of tests/word_limit_cases.py, and for the query probe (310 bases cut out of
rep20's own repeats: rep shares only the poly-A and the AC runs with rep20, so every limit below 191 prints the same rows
there) with GOLDEN_PROBE_LIMITS; for both, the percentages GOLDEN_PERCENTS and the run without the option.  Many of these
runs print the same bytes, so each distinct output is kept once, as word_limit_<query>_<first option that printed it>.segments,
and word_limit_index.json says for every (query, option) which file holds its output.  A limit of GOLDEN_LIMITS below the
longest list whose output is empty or equals the unlimited one shows nothing and is refused here.
tests/test_word_limit_oracle.py compares the outputs with the oracle.
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "lastz")
ARGS = ["--nogapped", "--format=segments"]
INDEX = os.path.join(HERE, "word_limit_index.json")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def write_inputs(d):
    """rep20.fa, rep.fa and probe.fa in directory d"""
    from lastz_amd import seqio
    import word_limit_cases as W
    for name in ("rep20", "rep", "probe"):
        seqio.write_fasta(os.path.join(str(d), name + ".fa"), [(name, W.SEQS[name]())])


def run(option, d, extra=ARGS, binary=REF, query="rep"):
    """stdout of one run on the files write_inputs(d) wrote; option: "--maxwordcount=..." or None"""
    args = [os.path.join(str(d), "rep20.fa"), os.path.join(str(d), query + ".fa")] + ([option] if option else []) + list(extra)
    return subprocess.check_output([binary] + args, stderr=subprocess.DEVNULL).decode()


def key_of(option):
    """the index's name of an option: none, <n>, p<p>"""
    if option is None:
        return "none"
    v = option.split("=")[1]
    return "p" + v[:-1] if v.endswith("%") else v


def options(query):
    import word_limit_cases as W
    limits = W.GOLDEN_LIMITS if query == "rep" else W.GOLDEN_PROBE_LIMITS
    return [None] + ["--maxwordcount=%d" % n for n in limits] + ["--maxwordcount=%s%%" % p for p in W.GOLDEN_PERCENTS]


def golden(query, option):
    """the recorded output of (query, option)"""
    index = json.load(open(INDEX))
    return open(os.path.join(HERE, index[query][key_of(option)])).read()


if __name__ == "__main__":
    import word_limit_cases as W
    index = {}
    with tempfile.TemporaryDirectory() as d:
        write_inputs(d)
        for query in ("rep", "probe"):
            index[query], files = {}, {}
            for option in options(query):
                out = run(option, d, query=query)
                if len(out.splitlines()) < 2:
                    sys.exit("%s against %s leaves nothing: drop the case" % (option, query))
                if query == "rep" and option and "%" not in option and out == run(None, d) and option != "--maxwordcount=%d" % max(W.GOLDEN_LIMITS):
                    sys.exit("%s changes nothing: drop the case" % option)
                if out not in files:
                    files[out] = "word_limit_%s_%s.segments" % (query, key_of(option))
                    open(os.path.join(HERE, files[out]), "w").write(out)
                index[query][key_of(option)] = files[out]
                print("%-6s %-8s %4d rows  %s" % (query, key_of(option), len(out.splitlines()) - 1, files[out]))
    json.dump(index, open(INDEX, "w"), indent=1, sort_keys=True)
