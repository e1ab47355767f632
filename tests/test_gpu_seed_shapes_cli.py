"""The seed shapes of tests/seed_shape_cases.py on the command line: integration/_build/lastz_gpu against the pristine
binary on a 300,000 x 300,000 synthetic pair with two query records, the seeds given as lastz names them (--seed=14of22,
T=4, --seed=match14, ...).  Same bytes for --format=general and for the default gapped LAV, and the notes say that the
table was built and the search done on the GPU.  A seed outside the fast path (match15: 30 bits) gives the same bytes through the reference's routines, quietly;
--seed=match1 is refused by lastz's own option parser ("seed length must be at least two"), the same way by both binaries.
Needs an MI355X and the prebuilt binaries."""
import re

import pytest

from lastz_amd import seqio
import seed_shape_cases as SC
from lavparse import normalize_lav
from test_gpu_lastz_cli import GPU_BIN, REF_BIN, needs_bins, run

pytestmark = pytest.mark.gpu
LONG31 = SC.CASES["long31"]["pattern"]
#        id             pair     options
ON_GPU = [("14of22",     "big",   ["--seed=14of22"]),
          ("T4",         "big",   ["T=4"]),
          ("14of22-t2",  "big",   ["--seed=14of22", "--transition=2"]),
          ("match14",    "big",   ["--seed=match14", "--notransition"]),
          ("match13-t2", "big",   ["--seed=match13", "--transition=2"]),
          ("long31",     "big",   ["--seed=" + LONG31]),
          ("match4",     "small", ["--seed=match4", "--notransition"])]         # 12,000 x 3000: just above LZGPU_MIN_TARGET
DECLINED = [("match15",  "big",   ["--seed=match15"])]
FORMATS = {"general": ["--format=general"], "lav": []}


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("seed_shapes_cli")
    t, q = seqio.synth_pair(300_000, 300_000, seed=6)
    q = q.copy()
    q[600:1800] = SC._diverged(t[5000:6200], 23)                                # (the cuts share no homology of their own)
    for name, tl, ql in (("big", 300_000, 300_000), ("small", 12_000, 3000), ("tiny", 12_000, 300)):
        seqio.write_fasta(d / (name + "_t.fa"), [("target", t[:tl])])
        seqio.write_fasta(d / (name + "_q.fa"), [("q1", q[:ql // 2]), ("q2", q[ql // 2:ql])])
    return d


def _both(inputs, pair, options, fmt):
    args = [pair + "_t.fa", pair + "_q.fa"] + options + FORMATS[fmt]
    a, err = run(GPU_BIN, args, inputs, {"LZGPU_VERBOSE": "1"})
    b, ref_err = run(REF_BIN, args, inputs)
    strip = normalize_lav if fmt == "lav" else (lambda s: "\n".join(ln for ln in s.split("\n") if not ln.startswith("#")))
    assert strip(a) == strip(b)
    return a, err, ref_err


@needs_bins
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("pair,options", [c[1:] for c in ON_GPU], ids=[c[0] for c in ON_GPU])
def test_named_seeds_stay_on_the_gpu(inputs, pair, options, fmt):
    out, err, _ = _both(inputs, pair, options, fmt)
    assert "[lzgpu] table: built on the GPU" in err and err.count("[lzgpu] search: done on the GPU") == 4, err[-1500:]
    assert "reference path" not in "".join(ln for ln in err.splitlines(True) if "] table:" in ln or "] search:" in ln), err[-1500:]
    assert out.count("\na {") >= 1 if fmt == "lav" else len([ln for ln in out.splitlines() if not ln.startswith("#")]) >= 1


@needs_bins
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("pair,options", [c[1:] for c in DECLINED], ids=[c[0] for c in DECLINED])
def test_seeds_outside_the_fast_path_take_the_reference_path(inputs, pair, options, fmt):
    out, err, ref_err = _both(inputs, pair, options, fmt)
    assert re.search(r"\[lzgpu\] table: (declined, )?reference path", err), err[-1500:]
    assert err.count("[lzgpu] search: reference path") == 4, err[-1500:]
    assert "table: built on the GPU" not in err and "search: done on the GPU" not in err
    rest = [ln for ln in err.splitlines() if not ln.startswith("[lzgpu]")]
    assert rest == ref_err.splitlines(), rest[:5]                               # besides the notes only what the reference says itself
    assert len(out) > 1000


@needs_bins
def test_match1_is_refused_by_both_binaries_alike(inputs):
    import subprocess
    args = ["tiny_t.fa", "tiny_q.fa", "--seed=match1"]
    a, b = (subprocess.run([binary] + args, cwd=inputs, capture_output=True, text=True, timeout=120) for binary in (GPU_BIN, REF_BIN))
    assert a.returncode == b.returncode != 0 and a.stdout == b.stdout
    assert "seed length must be at least two" in a.stderr and a.stderr == b.stderr
