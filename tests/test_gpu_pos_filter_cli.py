"""lastz --chores through integration/_build/lastz_gpu -- the reference's host code bound to liblzgpu.so -- and through the
pristine binary on the same box, on the chores files of the goldens (tests/golden/chores_*.chores): the outputs must be
identical byte for byte, without and with the gapped stage, and every gapped stage must have run on the reference's
routine (under a chores list it narrows each anchor's DP to the chore's intervals: not on the device).  A second test
asks that every seed search ran on the GPU (lzgpu_seed_hit_search_within, the target's fences patched into the device's
copy), wherever lastz_gpu was linked from this tree's shim.

One process at a time, each under its own time limit; a run that fails ends the test, and nothing is started after it."""
import os
import subprocess

import pytest

import helpers as H
import chores_golden as CG
from test_gpu_base_tests import GPU_BIN, REF_BIN, needs_bins, notes

pytestmark = pytest.mark.gpu
OUTPUTS = {"nogapped": ["--nogapped", "--format=segments"], "gapped": []}


def run(binary, name, extra, verbose=False):
    env = dict(os.environ)
    if verbose:
        env["LZGPU_VERBOSE"] = "1"
    p = subprocess.run([binary, "pseudocat.fa", "pseudopig.2bit", "--chores=%s.chores" % name] + extra, cwd=H.GOLDEN,
                       capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout, p.stderr


_runs = {}


def both(name, output):
    """(the pristine binary's stdout, lastz_gpu's stdout, its stderr), once per command line"""
    if (name, output) not in _runs:
        want, _ = run(REF_BIN, name, OUTPUTS[output])
        got, err = run(GPU_BIN, name, OUTPUTS[output], verbose=True)
        _runs[name, output] = (want, got, err)
    return _runs[name, output]


def binding_binds_within():
    """whether lastz_gpu was linked from a shim that sends --chores searches to lzgpu_seed_hit_search_within.  The shim
    can only be compiled where the reference's sources are; elsewhere integration/Makefile restores the binaries stashed
    in oracle/_ref/ by an earlier build, which may predate the binding (they then run such a search on the reference's
    routine, as tests/test_gpu_self.py says of --self)."""
    return b"lzgpu_seed_hit_search_within" in open(GPU_BIN, "rb").read()


@needs_bins
@pytest.mark.parametrize("output", list(OUTPUTS))
@pytest.mark.parametrize("name", CG.NAMES)
def test_chores_run_equals_the_pristine_binary(name, output):
    want, got, err = both(name, output)
    assert got == want
    if output == "nogapped":
        assert got == open(os.path.join(H.GOLDEN, name + ".segments")).read()
    n = notes(err)
    if output == "gapped":
        assert set(n.get("gapped", {})) == {"reference path"} and len(want.splitlines()) > 20, n
    else:
        assert "gapped" not in n, n


@needs_bins
@pytest.mark.skipif(os.path.exists(GPU_BIN) and not binding_binds_within(),
                    reason="integration/_build/lastz_gpu predates the --chores binding (restored from oracle/_ref/ without the reference sources to rebuild it)")
@pytest.mark.parametrize("output", list(OUTPUTS))
@pytest.mark.parametrize("name", CG.NAMES)
def test_chores_searches_run_on_the_gpu(name, output):
    _, _, err = both(name, output)
    n = notes(err)
    searches = sum(len(c[3]) for c in CG.read_chores(name))
    assert n.get("table") == {"built on the GPU": 1}, n
    assert n.get("search") == {"done on the GPU": searches}, n
