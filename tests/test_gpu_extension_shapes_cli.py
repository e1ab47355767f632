"""lastz --exact / --mismatch / --filter with other seeds, --step and --maxwordcount through integration/_build/lastz_gpu -- the
reference's host code bound to liblzgpu.so -- on the command lines the goldens of tests/extension_shape_cases.py were recorded
with (tests/golden/extension_shapes_index.json), both strands: the output must be the golden byte for byte, and the table, the
limit and every seed search must have run on the GPU wherever lastz_gpu was linked from this tree's shim.  --mismatch goes to
the device under LZGPU_MISMATCH=1.  One of the lines says everything at once: seed + --step + --maxwordcount + --filter + --exact.

One fresh process per command line, each under its own time limit; a run that fails ends the test, and nothing is started
after it."""
import os
import subprocess
import sys

import pytest

import helpers as H
import extension_shape_cases as X
from test_gpu_base_tests import GPU_BIN, notes

sys.path.insert(0, H.GOLDEN)
import make_extension_shapes_golden as M            # noqa: E402

pytestmark = pytest.mark.gpu
# one line per seed and per table form, the filters on each kind of search, and the line that says everything
NAMES = ["long31_spaced_exact", "long31_bytes_mismatch", "parts6_spaced_mismatch", "ends29_edges_exact", "s14of22_spaced_mismatch",
         "match14_collide_exact", "s1111_bytes_mismatch", "s11_edges_exact", "s101_edges_mismatch", "step3_long31_spaced_exact",
         "step3_s14of22_spaced_mismatch", "limit_s1111_edges_exact", "limit_12of19_spaced_mismatch", "f_2_25_long31_xdrop",
         "f_27_long31_exact", "f_cares_13_long31_mismatch", "f_cares_2_ends29_exact", "f_1_4_s1111_mismatch", "all_s1111_exact"]
needs_bin = pytest.mark.skipif(not os.path.exists(GPU_BIN), reason="integration/_build/lastz_gpu not built (it needs the reference's sources at build time)")


def binding_binds_all():
    """whether lastz_gpu was linked from a shim that sends --exact, --mismatch, --filter and --maxwordcount to the library (a
    binary restored from oracle/_ref/ without the reference's sources to rebuild it may predate a binding)"""
    blob = open(GPU_BIN, "rb").read()
    return all(s in blob for s in (b"lzgpu_seed_hit_search_exact", b"lzgpu_seed_hit_search_mismatch", b"lzgpu_set_hit_filter", b"lzgpu_table_limit"))


_runs = {}


def run(tmp, name):
    """(lastz_gpu's stdout, its stderr), once per command line"""
    if name not in _runs:
        env = dict(os.environ, LZGPU_VERBOSE="1", LZGPU_MIN_TARGET="1")       # (the binding leaves targets under 10 kbp to the reference)
        env.pop("LZGPU_MISMATCH", None)
        if X.CASES[name]["kind"] == "mismatch":
            env["LZGPU_MISMATCH"] = "1"
        p = subprocess.run([GPU_BIN] + M.write_inputs(tmp, name) + M.index()[name], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        _runs[name] = (p.stdout, p.stderr)
    return _runs[name]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("extension_shapes_cli")


def test_the_lines_are_the_recorded_ones():
    assert all(n in M.index() for n in NAMES)
    line = M.index()["all_s1111_exact"]
    assert all(any(o.startswith(p) for o in line) for p in ("--seed=", "--step=", "--maxwordcount=", "--filter=", "--exact="))
    for n in NAMES:
        assert M.index()[n] == M.options(n), n


@needs_bin
@pytest.mark.parametrize("name", NAMES)
def test_run_prints_the_golden(tmp, name):
    got, _ = run(tmp, name)
    assert got == M.golden(name) and len(got.splitlines()) >= 1


@needs_bin
@pytest.mark.skipif(os.path.exists(GPU_BIN) and not binding_binds_all(),
                    reason="integration/_build/lastz_gpu predates a binding (restored from oracle/_ref/ without the reference sources to rebuild it)")
@pytest.mark.parametrize("name", NAMES)
def test_searches_run_on_the_gpu(tmp, name):
    _, err = run(tmp, name)
    n = notes(err)
    assert n.get("table") == {"built on the GPU": 1}, n
    assert n.get("search") == {"done on the GPU": 2}, n                     # one query, two strands
    assert n.get("limit") == ({"done on the GPU": 1} if X.CASES[name]["limit"] else None), n
