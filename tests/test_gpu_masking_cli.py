"""lastz --masking=<count> with LZGPU_MASKING=1 through integration/_build/lastz_gpu -- the reference's host code bound to
liblzgpu.so -- and through the pristine binary on the same box: the outputs must be identical byte for byte, and with the
switch the masking must have run on the device (lzgpu_table_mask): every seed search stays on the GPU and the table is never
copied to the host.  The lines: the base test's own masking line (tests/test_gpu_base_tests.py pins it WITHOUT the switch),
and three on a generated target with 12 reads of one region (tests/golden/make_masking_golden.py: segments, --step=20, gapped).

One process at a time, each under its own time limit; a run that fails ends the test, and nothing is started after it."""
import os
import shutil
import subprocess
import sys

import pytest

import helpers as H
from lavparse import normalize_lav
from test_gpu_base_tests import GPU_BIN, REF_BIN, needs_bins, notes

sys.path.insert(0, H.GOLDEN)
import make_masking_golden as M                      # noqa: E402

pytestmark = pytest.mark.gpu
BASE = ["../test_data/fake_apple.fa", "../test_data/fake_orange_reads.fa", "--masking=3"]     # run in <inputs>/src, as the base tests run


def binding_binds_masking():
    """whether lastz_gpu was linked from a shim that sends masked intervals to lzgpu_table_mask (the shim can only be compiled
    where the reference's sources are; elsewhere integration/Makefile restores binaries stashed by an earlier build)"""
    return b"lzgpu_table_mask" in open(GPU_BIN, "rb").read()


needs_binding = pytest.mark.skipif(os.path.exists(GPU_BIN) and not binding_binds_masking(),
                                   reason="integration/_build/lastz_gpu predates the --masking binding (restored from oracle/_ref/ without the reference sources to rebuild it)")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("masking_cli")
    os.makedirs(d / "test_data"); os.makedirs(d / "src")
    M.write_inputs(d / "src")
    for f in BASE[:2]:
        shutil.copy(os.path.join(H.GOLDEN, os.path.basename(f)), d / "test_data" / os.path.basename(f))
    return d / "src"


def run(binary, d, args, masking=False, verbose=False):
    env = {k: v for k, v in os.environ.items() if k != "LZGPU_MASKING"}
    if verbose:
        env["LZGPU_VERBOSE"] = "1"
    if masking:
        env["LZGPU_MASKING"] = "1"
    p = subprocess.run([binary] + args, cwd=str(d), capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout, p.stderr


def check_on_the_gpu(n, searches):
    assert n.get("table", {}).get("built on the GPU") == 1, n
    assert "copied to the host for a reference routine" not in n["table"], n
    assert n.get("search") == {"done on the GPU": searches}, n
    assert n.get("mask", {}).get("done on the GPU", 0) >= 1 and "reference path" not in n["mask"], n


@needs_bins
@needs_binding
def test_base_test_masking_line(inputs):
    want, _ = run(REF_BIN, inputs, BASE)
    got, err = run(GPU_BIN, inputs, BASE, masking=True, verbose=True)
    assert got == want
    assert normalize_lav(got) == normalize_lav(open(os.path.join(H.GOLDEN, "base_test.masking.lav")).read())
    n = notes(err)
    check_on_the_gpu(n, 200)
    # the gapped stage as the parent's path runs it: the same binary without the switch is the yardstick
    plain, perr = run(GPU_BIN, inputs, BASE, verbose=True)
    assert plain == want
    p = notes(perr)
    assert "mask" not in p and p["search"].get("reference path", 0) > 0, p
    assert n.get("gapped") == p.get("gapped"), (n, p)


@needs_bins
@needs_binding
@pytest.mark.parametrize("name", list(M.LINES))
def test_generated_reads(inputs, name):
    args = ["target.fa", "reads.fa"] + M.LINES[name][0]
    want, _ = run(REF_BIN, inputs, args)
    got, err = run(GPU_BIN, inputs, args, masking=True, verbose=True)
    assert got == want
    assert got == M.golden(name)
    check_on_the_gpu(notes(err), 2 * M.NREADS)
