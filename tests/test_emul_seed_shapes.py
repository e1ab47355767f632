"""The seed shapes of tests/seed_shape_cases.py through the CPU emulation of the device pipeline (tests/emul): table
CSR, HSPs, order and counters in both modes equal the oracle's, for heavy (28-bit), long (31), many-part, many-probe
(106) and very light (4-bit) seeds.  The cases of the 120 kbp pair run on its first 60,000 x 50,000 bases.  The emulator
holds the per-lane logic only; what a GPU alone runs of these shapes is tests/test_gpu_seed_shapes.py's."""
import pytest

import seed_shape_cases as SC
from test_emul_vs_oracle import _check, em          # noqa: F401  (em: the module-scoped fixture)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_emulator_equals_oracle(em, name):
    c = SC.CASES[name]
    t, q = SC.emul_sequences(name)
    _check(em, t, q, pattern=c["pattern"], wt=c["trans"], cap=c["capacity"], step=c["step"], hsp_threshold=c["thr"])


def test_declined_table_leaves_the_emulator_usable(em):
    from lastz_amd import lzgpu
    from oracle import lzo
    t, q = SC.emul_sequences("light2")
    for pattern, trans in SC.DECLINED_TABLES:
        with pytest.raises(lzgpu.NotHandled) as e:
            em.table_prepare(t, em.seed(pattern, trans), lzo.upper_nuc_to_bits())
        assert e.value.rc == 1
    _check(em, t, q, pattern="11", wt=0, cap=50_000, hsp_threshold=1500)
