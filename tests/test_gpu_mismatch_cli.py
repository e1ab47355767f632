"""lastz --mismatch=<count>,<length> through integration/_build/lastz_gpu under LZGPU_MISMATCH=1 -- the reference's host code
bound to liblzgpu.so -- and through the pristine binary on the same box, on sequences of tests/mismatch_cases.py, both strands,
without and with the gapped stage, in both spellings of the option: the outputs must be identical byte for byte, and every seed
search must have run on the GPU (lzgpu_seed_hit_search_mismatch) wherever lastz_gpu was linked from this tree's shim.  (Without
the switch such a search stays on the reference's routine: tests/test_gpu_exact_cli.py.)

One process at a time, each under its own time limit; a run that fails ends the test, and nothing is started after it."""
import os
import subprocess
import sys

import pytest

import helpers as H
import mismatch_cases as MC
from test_gpu_base_tests import GPU_BIN, REF_BIN, needs_bins, notes

sys.path.insert(0, H.GOLDEN)
import make_mismatch_golden as M                    # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["spaced", "long", "bytes"]
OUTPUTS = {"nogapped": ["--nogapped", MC.GOLDEN_FORMAT], "gapped": [MC.GOLDEN_FORMAT]}       # (no lav: a [multi] target rules it out)
SPELLINGS = (0, 1)                                   # --mismatch=<count>,<length> and --<count>mismatch=<length>


def run(binary, files, options, gpu=False):
    env = dict(os.environ)
    env.pop("LZGPU_MISMATCH", None)
    if gpu:
        env["LZGPU_MISMATCH"] = "1"
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
        got, err = run(GPU_BIN, files, options, gpu=True)
        _runs[key] = (want, got, err)
    return _runs[key]


def mismatch_options(name, output, spelling):
    return [o for o in MC.lastz_options(name, spelling) if o != "--strand=plus"] + OUTPUTS[output]     # (both strands: lastz's default)


def binding_binds_mismatch():
    """whether lastz_gpu was linked from a shim that sends --mismatch searches to lzgpu_seed_hit_search_mismatch (the shim can
    only be compiled where the reference's sources are; a binary restored from oracle/_ref/ may predate the binding)"""
    return b"lzgpu_seed_hit_search_mismatch" in open(GPU_BIN, "rb").read()


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("mismatch_cli")


@needs_bins
@pytest.mark.parametrize("spelling", SPELLINGS)
@pytest.mark.parametrize("output", list(OUTPUTS))
@pytest.mark.parametrize("name", NAMES)
def test_mismatch_run_equals_the_pristine_binary(tmp, name, output, spelling):
    want, got, _ = both(tmp, name, mismatch_options(name, output, spelling))
    assert got == want
    assert len(want.splitlines()) > (5 if output == "nogapped" else 0)
    if output == "nogapped":                                                # the plus strand's rows are the golden's
        plus = [r for r in MC.parse_rows(got) if r[6] == "+"]
        assert sorted(plus) == sorted(MC.parse_rows(M.golden(name)))


@needs_bins
@pytest.mark.skipif(os.path.exists(GPU_BIN) and not binding_binds_mismatch(),
                    reason="integration/_build/lastz_gpu predates the --mismatch binding (restored from oracle/_ref/ without the reference sources to rebuild it)")
@pytest.mark.parametrize("spelling", SPELLINGS)
@pytest.mark.parametrize("output", list(OUTPUTS))
@pytest.mark.parametrize("name", NAMES)
def test_mismatch_searches_run_on_the_gpu(tmp, name, output, spelling):
    _, _, err = both(tmp, name, mismatch_options(name, output, spelling))
    n = notes(err)
    assert n.get("table") == {"built on the GPU": 1}, n
    assert n.get("search") == {"done on the GPU": 2}, n                     # one query, two strands
