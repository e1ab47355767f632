"""lastz --exact=<length> through integration/_build/lastz_gpu -- the reference's host code bound to liblzgpu.so -- and through
the pristine binary on the same box, on the sequences of tests/exact_cases.py, both strands, without and with the gapped
stage: the outputs must be identical byte for byte, and every seed search must have run on the GPU
(lzgpu_seed_hit_search_exact) wherever lastz_gpu was linked from this tree's shim.  --mismatch stays on the reference's
routine and still agrees.

One process at a time, each under its own time limit; a run that fails ends the test, and nothing is started after it."""
import os
import subprocess
import sys

import pytest

import helpers as H
import exact_cases as EC
from test_gpu_base_tests import GPU_BIN, REF_BIN, needs_bins, notes

sys.path.insert(0, H.GOLDEN)
import make_exact_golden as M                       # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["spaced", "long", "bytes"]
OUTPUTS = {"nogapped": ["--nogapped", EC.GOLDEN_FORMAT], "gapped": [EC.GOLDEN_FORMAT]}       # (no lav: a [multi] target rules it out)


def run(binary, files, options, verbose=False):
    env = dict(os.environ)
    if verbose:
        env["LZGPU_VERBOSE"] = "1"
        env["LZGPU_MIN_TARGET"] = "1"                # (the binding leaves targets under 10 kbp to the reference: `long` and `bytes` are shorter)
    p = subprocess.run([binary] + files + options, capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout, p.stderr


_runs = {}


def both(tmp, name, options):
    """(the pristine binary's stdout, lastz_gpu's stdout, its stderr), once per command line"""
    key = (name, tuple(options))
    if key not in _runs:
        d = tmp / name
        d.mkdir(exist_ok=True)
        files = M.write_inputs(d, name)
        want, _ = run(REF_BIN, files, options)
        got, err = run(GPU_BIN, files, options, verbose=True)
        _runs[key] = (want, got, err)
    return _runs[key]


def exact_options(name, output):
    c = EC.CASES[name]
    return ["--exact=%d" % c["thr"]] + c["option"] + c["extra"] + OUTPUTS[output]        # (both strands: lastz's default)


def binding_binds_exact():
    """whether lastz_gpu was linked from a shim that sends --exact searches to lzgpu_seed_hit_search_exact.  The shim can
    only be compiled where the reference's sources are; elsewhere integration/Makefile restores the binaries stashed in
    oracle/_ref/ by an earlier build, which may predate the binding (they then run such a search on the reference's routine)."""
    return b"lzgpu_seed_hit_search_exact" in open(GPU_BIN, "rb").read()


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("exact_cli")


@needs_bins
@pytest.mark.parametrize("output", list(OUTPUTS))
@pytest.mark.parametrize("name", NAMES)
def test_exact_run_equals_the_pristine_binary(tmp, name, output):
    want, got, _ = both(tmp, name, exact_options(name, output))
    assert got == want
    assert len(want.splitlines()) > (5 if output == "nogapped" else 0)
    if output == "nogapped":                                                # the plus strand's rows are the golden's
        plus = [r for r in EC.parse_rows(got) if r[6] == "+"]
        assert sorted(plus) == sorted(EC.parse_rows(M.golden(name)))


@needs_bins
@pytest.mark.skipif(os.path.exists(GPU_BIN) and not binding_binds_exact(),
                    reason="integration/_build/lastz_gpu predates the --exact binding (restored from oracle/_ref/ without the reference sources to rebuild it)")
@pytest.mark.parametrize("output", list(OUTPUTS))
@pytest.mark.parametrize("name", NAMES)
def test_exact_searches_run_on_the_gpu(tmp, name, output):
    _, _, err = both(tmp, name, exact_options(name, output))
    n = notes(err)
    assert n.get("table") == {"built on the GPU": 1}, n
    assert n.get("search") == {"done on the GPU": 2}, n                     # one query, two strands


@needs_bins
def test_mismatch_stays_on_the_reference_path(tmp):
    c = EC.CASES["spaced"]
    want, got, err = both(tmp, "spaced", ["--mismatch=2,30"] + c["option"] + OUTPUTS["nogapped"])
    assert got == want and len(want.splitlines()) > 5
    assert notes(err).get("search") == {"reference path": 2}, notes(err)
