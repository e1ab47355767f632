"""Record the --chores goldens under tests/golden/ from the PRISTINE reference binary (oracle/_ref/lastz):

    python tests/golden/make_chores_golden.py

For every chores file chores_<name>.chores (committed, written by hand) the output of
    lastz pseudocat.fa pseudopig.2bit --chores=chores_<name>.chores --nogapped --format=segments
goes to chores_<name>.segments.  The query is the 2bit file: a chores list visits a query several times, which lastz
can do only in a file format with random access.  tests/test_pos_filter_oracle.py compares the outputs with the oracle.
"""
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "lastz")
ARGS = ["--nogapped", "--format=segments"]


def run(chores, extra=ARGS, binary=REF):
    """stdout of one chores run, started in tests/golden (the files are named without directories)"""
    return subprocess.check_output([binary, "pseudocat.fa", "pseudopig.2bit", "--chores=" + os.path.basename(chores)] + list(extra),
                                   cwd=HERE, stderr=subprocess.DEVNULL).decode()


if __name__ == "__main__":
    for chores in sorted(glob.glob(os.path.join(HERE, "chores_*.chores"))):
        out = run(chores)
        open(chores[:-len(".chores")] + ".segments", "w").write(out)
        print("%-24s %3d rows" % (os.path.basename(chores), len(out.splitlines()) - 1))
