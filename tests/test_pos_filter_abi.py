"""The C ABI of lzgpu_seed_hit_search_within (lastz --chores, include/lzgpu.h): lz_pos_filter's layout against the ctypes
mirror, the symbol, and no fall-back without a device.  CPU only."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from lastz_amd import lzgpu
import helpers as H


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(lzgpu.LIB_PATH):
        g.build()
    return lzgpu.Lib()


def test_pos_filter_layout():
    fields = ("t_start", "t_end", "q_start", "q_end")
    src = '#include "lzgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu' + " %zu" * len(fields) + '\\n",' \
          "sizeof(lz_pos_filter)," + ",".join("offsetof(lz_pos_filter,%s)" % f for f in fields) + ");return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(H.ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    P = lzgpu.PosFilter
    assert got == [C.sizeof(P)] + [getattr(P, f).offset for f in fields] == [16, 0, 4, 8, 12]
    assert [n for n, _ in P._fields_] == list(fields)


def test_entry_point_is_exported(lib):
    assert hasattr(lib.L, "lzgpu_seed_hit_search_within")
    assert "lzgpu_seed_hit_search_within" in lzgpu.EXPORTS
    assert callable(lib.seed_hit_search_within)
    header = open(os.path.join(H.ROOT, "include", "lzgpu.h")).read()
    assert "int lzgpu_seed_hit_search_within(const lz_search_args* args, const lz_pos_filter* within, lz_hsp** out, uint64_t* n_out);" in header


@pytest.mark.skipif(torch.cuda.is_available(), reason="this checks the no-GPU behaviour")
def test_no_device_no_fallback(lib):
    assert lib.probe() == -1                                    # LZGPU_ERR_NO_DEVICE
    _, masked = H.scoring()
    q = np.frombuffer(b"ACGT" * 100, dtype=np.uint8)
    a = lzgpu.SearchArgs()
    a.query, a.qlen, a.query_slot = q.ctypes.data, len(q), -1
    a.sub, a.xdrop, a.hsp_threshold, a.entropic, a.extend = masked.ctypes.data, 910, 3000, 1, 1
    out, n = C.c_void_p(), C.c_uint64(7)
    for w in (lzgpu.PosFilter(0, 400, 0, 400), lzgpu.PosFilter(0, 0, 0, 0), lzgpu.PosFilter(9, 3, 0, 400)):
        assert lib.L.lzgpu_seed_hit_search_within(C.byref(a), C.byref(w), C.byref(out), C.byref(n)) == -1
        assert not out.value
    with pytest.raises(lzgpu.LzGpuError):
        lib.seed_hit_search_within(masked, (0, 400), (0, 400), q=q)
