"""lastz --maxwordcount through integration/_build/lastz_gpu -- the reference's host code bound to liblzgpu.so -- and through
the pristine binary on the same box, rep20 against rep (tests/self_cases.py, written as FASTA into a temporary directory):
the outputs must be identical byte for byte for a count, a percentage, a self-comparison, a count with dynamic masking and
the chasm form.  A second test asks where the work ran, wherever lastz_gpu was linked from this tree's shim: the limit is
set on the device's table (lzgpu_table_limit), a percentage is resolved there (lzgpu_table_find_limit), every seed search
stays on the GPU and the table is not copied to the host -- except for masking, which reads the host copy (limited by
the reference's own routine), and the chasm form, which keeps the reference path.

One process at a time, each under its own time limit; a run that fails ends the test, and nothing is started after it."""
import os
import subprocess
import sys

import pytest

import helpers as H
import word_limit_cases as W
from test_gpu_base_tests import GPU_BIN, REF_BIN, needs_bins, notes

sys.path.insert(0, H.GOLDEN)
import make_word_limit_golden as M                  # noqa: E402

pytestmark = pytest.mark.gpu
SEG = ["--nogapped", "--format=segments"]
#            name         files            arguments
LINES = {"count":      ("rep20 rep", ["--maxwordcount=7"] + SEG),
         "probe":      ("rep20 probe", ["--maxwordcount=%s%%" % W.GOLDEN_PERCENTS[1]] + SEG),
         "gapped":     ("rep20 rep", ["--maxwordcount=7"]),
         "percent":    ("rep20 rep", ["--maxwordcount=%s%%" % W.GOLDEN_PERCENTS[-1]] + SEG),
         "self":       ("rep20",     ["--self", "--maxwordcount=40", "--nogapped"]),
         "masking":    ("rep20 rep", ["--maxwordcount=7", "--masking=3"]),
         "chasm":      ("rep20 rep", ["--maxwordcount=7,500"])}
ON_THE_GPU = ["count", "probe", "gapped", "percent", "self"]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("word_limit_cli")
    M.write_inputs(d)
    return d


def run(binary, d, files, extra, verbose=False):
    env = dict(os.environ)
    if verbose:
        env["LZGPU_VERBOSE"] = "1"
    p = subprocess.run([binary] + [f + ".fa" for f in files.split()] + extra, cwd=str(d), capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout, p.stderr


_runs = {}


def both(d, name):
    """(the pristine binary's stdout, lastz_gpu's stdout, its stderr), once per command line"""
    if name not in _runs:
        files, extra = LINES[name]
        want, _ = run(REF_BIN, d, files, extra)
        got, err = run(GPU_BIN, d, files, extra, verbose=True)
        _runs[name] = (want, got, err)
    return _runs[name]


def binding_binds_limit():
    """whether lastz_gpu was linked from a shim that sends --maxwordcount to lzgpu_table_limit.  The shim can only be compiled
    where the reference's sources are; elsewhere integration/Makefile restores the binaries stashed in oracle/_ref/ by an
    earlier build, which may predate the binding (they then limit the host copy and search on the reference's routine)."""
    return b"lzgpu_table_limit" in open(GPU_BIN, "rb").read()


@needs_bins
@pytest.mark.parametrize("name", list(LINES))
def test_run_equals_the_pristine_binary(inputs, name):
    want, got, _ = both(inputs, name)
    assert got == want
    assert len(want.splitlines()) > (20 if name != "probe" else 10)
    if name == "probe":
        assert got == M.golden("probe", LINES[name][1][0])
    if name in ("count", "percent"):
        assert got == M.golden("rep", LINES[name][1][0])


@needs_bins
@pytest.mark.skipif(os.path.exists(GPU_BIN) and not binding_binds_limit(),
                    reason="integration/_build/lastz_gpu predates the --maxwordcount binding (restored from oracle/_ref/ without the reference sources to rebuild it)")
@pytest.mark.parametrize("name", list(LINES))
def test_where_the_limit_and_the_searches_ran(inputs, name):
    _, _, err = both(inputs, name)
    n = notes(err)
    searches = 2                                                            # one query, two strands
    assert n.get("table", {}).get("built on the GPU") == 1, n
    if name in ON_THE_GPU:
        want = {"done on the GPU": 1}
        if name in ("percent", "probe"):
            want["found on the GPU"] = 1
        assert n.get("limit") == want, n
        assert n.get("search") == {"done on the GPU": searches}, n
        assert "copied to the host for a reference routine" not in n["table"], n
    elif name == "masking":
        # the first search runs on the limited device table; masking then reads (and rewrites) the host copy
        assert n.get("limit") == {"done on the GPU": 1}, n
        assert n["table"].get("copied to the host for a reference routine") == 1, n
        assert n["search"].get("done on the GPU", 0) >= 1, n
        lines = [x for x in err.split("\n") if x.startswith("[lzgpu] ")]
        assert lines.index("[lzgpu] limit: done on the GPU") < lines.index("[lzgpu] table: copied to the host for a reference routine")
    else:                                                                   # the chasm form: as before this binding
        assert n.get("limit") == {"reference path": 1}, n
        assert n.get("search") == {"reference path": searches}, n
        assert n["table"].get("copied to the host for a reference routine") == 1, n
