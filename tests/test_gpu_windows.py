"""lzgpu_window_search past one window per workgroup: the cases of tests/window_cases.py (stated and checked for what they
reach by tests/test_window_cases.py on the CPU), each window's HSPs against the oracle run on the cut-out pieces, order
included.  `many` hands 1536 windows to one launch, so that every block walks several of them whatever the number of CUs
-- a heavy window after a small one and before one, a small one after a 20 kbp one -- and the launcher runs the kernel a
second time with room for all HSPs; `retry_small` does that on a call of 8 windows and searches them again at once;
`edges` puts HSPs on the first and the last diagonal of a window and along all of a 20480-base side; `light_*` are inner
seeds of 4 to 14 bits, two of them with fewer words than the workgroup has lanes.  Needs an MI355X."""
import time

import pytest

from oracle import lzo
import window_cases as WC

pytestmark = pytest.mark.gpu
CTB = lzo.upper_nuc_to_bits()


@pytest.fixture(scope="module")
def resident(gpu):
    """the pair's table and target on the device, the query in slot 5"""
    t, q = WC.pair()
    gpu.table_prepare(t, gpu.seed(), CTB)
    gpu.query_upload(5, q)
    return gpu


def _search(gpu, case, thr, **kw):
    c = WC.CASES[case]
    isd = gpu.seed(c.get("pattern", WC.INNER), 0)
    t0 = time.perf_counter()
    got = gpu.window_search(WC.masked(), c["windows"](), isd, CTB, slot=5, hsp_threshold=thr, **kw)
    return got, time.perf_counter() - t0


def _is_the_oracles(got, case, thr):
    want = WC.expected(case, thr)
    k = WC.differs(got, want)
    assert k is None, (case, thr, k, k >= 0 and (WC.CASES[case]["windows"]()[k], len(got[k]), len(want[k])))


@pytest.mark.parametrize("thr", WC.CASES["many"]["thresholds"])
def test_many_windows_in_one_call(resident, thr):
    got, s = _search(resident, "many", thr)
    print("\nmany at %d: %d HSPs in %d windows, %.3f s on the device" % (thr, sum(len(x) for x in got), len(got), s))
    _is_the_oracles(got, "many", thr)


def test_more_hsps_than_room_in_a_small_call(resident):
    """the launcher's second run with room for all, then the same windows at a threshold that needs none: the grown buffer
    and the count word do not carry over"""
    for thr in WC.CASES["retry_small"]["thresholds"]:
        got, _ = _search(resident, "retry_small", thr)
        _is_the_oracles(got, "retry_small", thr)


@pytest.mark.parametrize("thr", WC.CASES["edges"]["thresholds"])
def test_hsps_on_the_edges_of_a_window(resident, thr):
    got, _ = _search(resident, "edges", thr)
    _is_the_oracles(got, "edges", thr)
    full = got[WC.edges().index(WC.IDENTICAL)]
    assert (full["length"] == WC.LZ_WIN_MAXLEN).sum() == 1


@pytest.mark.parametrize("pattern", list(WC.LIGHT))
def test_light_inner_seeds(resident, pattern):
    """no pattern of these is declined: one probe, at most 14 bits (lzgpu_window_search)"""
    got, _ = _search(resident, "light_" + pattern, WC.LIGHT_THR)
    _is_the_oracles(got, "light_" + pattern, WC.LIGHT_THR)


def test_the_query_as_host_bytes_and_after_another_case(resident):
    """`many` at 2200 from host bytes, right after the heaviest call of the module: equal to the oracle again"""
    _search(resident, "edges", 600)
    got, _ = _search_host(resident)
    _is_the_oracles(got, "many", 2200)


def _search_host(gpu):
    t0 = time.perf_counter()
    got = gpu.window_search(WC.masked(), WC.many()[0], gpu.seed(WC.INNER, 0), CTB, q=WC.pair()[1], hsp_threshold=2200)
    return got, time.perf_counter() - t0
