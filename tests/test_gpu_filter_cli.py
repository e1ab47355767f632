"""lastz --filter through integration/_build/lastz_gpu -- the reference's host code bound to liblzgpu.so -- and through the
pristine binary on the same box, on the command lines of the goldens (tests/filter_cases.py, both strands): --filter=2,15,
--filter=cares:12, --filter=2,15 --exact=25, and --filter=2,15 under a --chores file.  The outputs must be identical byte for
byte, the golden's where there is one, and every seed search must have run on the GPU (lzgpu_set_hit_filter around the
search's entry point) wherever lastz_gpu was linked from this tree's shim.

One process at a time, each under its own time limit; a run that fails ends the test, and nothing is started after it."""
import os
import subprocess
import sys

import pytest

import helpers as H
import chores_golden as CG
import filter_cases as FC
from test_gpu_base_tests import GPU_BIN, REF_BIN, needs_bins, notes

sys.path.insert(0, H.GOLDEN)
import make_filter_golden as M                      # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["whole_2_15", "cares_12", "exact"]
CHORES = "chores_basic"


def run(binary, args, cwd=None, verbose=False):
    env = dict(os.environ)
    if verbose:
        env["LZGPU_VERBOSE"] = "1"
    p = subprocess.run([binary] + args, cwd=cwd, capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout, p.stderr


_runs = {}


def both(key, args, cwd=None):
    """(the pristine binary's stdout, lastz_gpu's stdout, its stderr), once per command line"""
    if key not in _runs:
        want, _ = run(REF_BIN, args, cwd)
        got, err = run(GPU_BIN, args, cwd, verbose=True)
        _runs[key] = (want, got, err)
    return _runs[key]


def case_runs(tmp, name):
    d = tmp / name
    d.mkdir(exist_ok=True)
    return both(name, M.write_inputs(d, name) + M.options(name))


def chores_runs():
    return both("chores", ["pseudocat.fa", "pseudopig.2bit", "--chores=%s.chores" % CHORES, FC.filter_option("whole_2_15"), "--nogapped", "--format=segments"],
                cwd=H.GOLDEN)


def binding_binds_filter():
    """whether lastz_gpu was linked from a shim that sets the hit filter.  The shim can only be compiled where the reference's
    sources are; elsewhere integration/Makefile restores the binaries stashed in oracle/_ref/ by an earlier build, which may
    predate the binding (they then run a filtered search on the reference's routine)."""
    return b"lzgpu_set_hit_filter" in open(GPU_BIN, "rb").read()


predates = pytest.mark.skipif(os.path.exists(GPU_BIN) and not binding_binds_filter(),
                              reason="integration/_build/lastz_gpu predates the --filter binding (restored from oracle/_ref/ without the reference sources to rebuild it)")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("filter_cli")


@needs_bins
@pytest.mark.parametrize("name", NAMES)
def test_filtered_run_equals_the_pristine_binary_and_the_golden(tmp, name):
    want, got, _ = case_runs(tmp, name)
    assert got == want
    assert got == M.golden(name) and len(got.splitlines()) > 3


@needs_bins
@predates
@pytest.mark.parametrize("name", NAMES)
def test_filtered_searches_run_on_the_gpu(tmp, name):
    _, _, err = case_runs(tmp, name)
    n = notes(err)
    assert n.get("table") == {"built on the GPU": 1}, n
    assert n.get("search") == {"done on the GPU": 2}, n                     # one query, two strands


@needs_bins
def test_filtered_chores_run_equals_the_pristine_binary():
    want, got, _ = chores_runs()
    assert got == want and len(want.splitlines()) > 3
    plain, _ = run(REF_BIN, ["pseudocat.fa", "pseudopig.2bit", "--chores=%s.chores" % CHORES, "--nogapped", "--format=segments"], cwd=H.GOLDEN)
    assert plain != want                                                    # (the filter takes something away from this run)


@needs_bins
@predates
def test_filtered_chores_searches_run_on_the_gpu():
    _, _, err = chores_runs()
    n = notes(err)
    searches = sum(len(c[3]) for c in CG.read_chores(CHORES))
    assert n.get("table") == {"built on the GPU": 1}, n
    assert n.get("search") == {"done on the GPU": searches}, n
