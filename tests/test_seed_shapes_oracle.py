"""The seed shapes of tests/seed_shape_cases.py against the pristine binary, on the CPU: what lastz printed for each case
(tests/golden/seed_shapes_<case>.tsv, recorded by tests/golden/make_seed_shapes_golden.py with the seed given by its
command-line name: --seed=14of22, --seed=match14, ...) is what the oracle finds with the case's pattern; where
oracle/_ref/lastz is present it is run again.  Every case reaches what it is for (seed_shape_cases.reaches), the declined
patterns are declined, and lzgpu.Lib.table_export sizes last[] by the resident table's seed, not by the last one prepared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import lzo
from lastz_amd import lzgpu
import helpers as H
import seed_shape_cases as SC

sys.path.insert(0, H.GOLDEN)
import make_seed_shapes_golden as M                 # noqa: E402


def _masked():
    return H.scoring()[1]


def _rows(hs):
    return [r for strand, h in zip("+-", hs) for r in H.hsps_as_tsv_rows("query", strand, h)]


@pytest.mark.parametrize("name", list(SC.CASES))
def test_golden_is_the_oracles_search(name):
    gold = H.read_hsp_tsv(M.path(name))
    assert len(gold) > 0
    assert _rows(SC.oracle_search(lzo, name, _masked())[0]) == gold


def test_heavy_blocks_golden_and_reach():
    assert _rows(SC.heavy_search(lzo, _masked())[1]) == H.read_hsp_tsv(M.path("heavy_blocks"))
    assert SC.heavy_reaches(lzo, _masked()) is None


@pytest.mark.parametrize("name", list(SC.CASES))
def test_case_reaches_what_it_is_for(name):
    assert SC.reaches(lzo, name, _masked()) is None


def test_trimmed_pattern_is_its_twin():
    c = SC.CASES["trimmed"]
    t, _ = SC.sequences(c["seq"])
    tab = lzo.Table(t, lzo.seed(c["twin"], c["trans"]))
    for q, want in zip(SC.queries("trimmed"), SC.oracle_search(lzo, "trimmed", _masked())[0]):
        got, _ = lzo.seed_hit_search(tab, q, _masked(), hsp_threshold=c["thr"])
        assert len(got) == len(want) and (got == want).all()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(lzgpu.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return lzgpu.Lib()


def test_library_compiles_the_cases_as_the_oracle_does(lib):
    for name, c in SC.CASES.items():
        for pattern in filter(None, (c["pattern"], c["twin"])):
            a, b = lib.seed(pattern, c["trans"]), lzo.seed(c["pattern"], c["trans"])
            assert (a.length, a.weight_bits, a.num_parts, a.num_probes) == (b.length, b.weight, b.num_parts, b.num_probes), name
            assert [(a.shift[i], a.mask[i]) for i in range(a.num_parts)] == [(b.shift[i], b.mask[i]) for i in range(b.num_parts)], name
            assert [a.probe_xor[i] for i in range(a.num_probes)] == [b.probe_xor[i] for i in range(b.num_probes)], name


def test_declined_patterns(lib):
    for pattern, trans in SC.DECLINED_SEEDS:
        with pytest.raises(lzgpu.NotHandled) as e:
            lib.seed(pattern, trans)
        assert e.value.rc == 1, pattern                                     # LZGPU_NH_SEED
    for pattern, trans in SC.DECLINED_TABLES:                               # compiled here, declined by lzgpu_table_prepare (GPU tier)
        sd = lib.seed(pattern, trans)
        assert (sd.length, sd.weight_bits) == (1, 2)


def test_table_export_sizes_last_by_the_resident_tables_seed():
    """prepare an 8-mer, load a 14-mer's table: the buffer handed to lzgpu_table_export has 2^28 entries"""
    class L:                                                                # a stand-in for liblzgpu.so: it remembers the geometry only
        geom, seen = None, None

        def lzgpu_table_prepare(self, t, n, start, end, ctb, sd, step):
            L.geom = (n, start, end or n, step, sd._obj.weight_bits); return 0

        def lzgpu_table_load(self, path):
            L.geom = (1000, 0, 1000, 1, 28); return 0

        def lzgpu_table_geom(self, g):
            g._obj.tlen, g._obj.start, g._obj.end, g._obj.step, g._obj.seed.weight_bits = L.geom; return 0

        def lzgpu_table_export(self, last, prev):
            L.seen = (last, prev); return 0

    g = lzgpu.Lib.__new__(lzgpu.Lib)
    g.L, g.px, g._keep = L(), "lzgpu_", {}
    sd = lzgpu.SeedDesc(); sd.weight_bits = 16
    g.table_prepare(np.zeros(500, np.uint8), sd, np.zeros(256, np.int8))
    assert len(g.table_export(501)[0]) == 1 << 16
    g.table_load("a 14-mer's table")
    last, prev = g.table_export(1001)
    assert len(last) == 1 << 28 and len(prev) == 1001 and L.seen[0].value == last.ctypes.data
    with pytest.raises(lzgpu.LzGpuError):                                   # a prev[] of another table's size is not handed over
        g.table_export(501)


@pytest.mark.parametrize("name", M.names())
def test_live_reference_run(tmp_path_factory, name):
    if lzo.ref_binary() is None:
        pytest.skip("oracle/_ref/lastz is not built here (the goldens above always run)")
    d = tmp_path_factory.getbasetemp() / "seed_shape_inputs"
    if not d.exists():
        d.mkdir()
        M.write_inputs(d)
    assert M.run(name, d) == M.golden(name)
