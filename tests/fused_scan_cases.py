"""The cases of tests/test_gpu_fused_scan.py, run by tests/gpu_child.py under whatever LZGPU_FUSED_SCAN /
LZGPU_TASK_REGION_CAP the parent put into its environment."""
import numpy as np

from lastz_amd import seqio
from oracle import lzo
import helpers as H

CTB = lzo.upper_nuc_to_bits()


def tandem_pair():
    """a 61-base unit 700 times in the target and 40 times in the query: a word of the unit has a list of 700 entries, the
    query positions that hold it are neighbours in the word-sorted list, so one wave's 64 entries concatenate to far more
    than LZ_F2_CAP = 2560 hits (and than the fused kernel's pieces)"""
    rng = np.random.default_rng(5)
    t, q = seqio.synth_pair(200_000, 200_000, seed=41)
    unit = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 61)]
    t = t.copy(); q = q.copy()
    t[50_000:50_000 + 61 * 700] = np.tile(unit, 700)
    q[120_000:120_000 + 61 * 40] = np.tile(unit, 40)
    return t, q


def pair_case(g, t, q, with_trans=1, capacity=None):
    _, masked = H.scoring()
    g.table_prepare(t, g.seed(H.DEFAULT_SEED, with_trans), CTB)
    if capacity:
        g.set_hit_capacity(capacity)
    try:
        yield H.search_strands(g, lambda qq: g.seed_hit_search(masked, q=qq), [qq for _, _, qq in H.strands(q)])
    finally:
        if capacity:
            g.set_hit_capacity(1 << 28)


def self_case(g):
    import test_gpu_self as S
    v, seps, names, _, _ = S.load("plain")
    masked = H.scoring()[1]
    g.table_prepare(v, g.seed(), CTB)
    yield H.search_strands(g, lambda strand: g.seed_hit_search_self(masked, q=(v if strand == "+" else S.minus(v, seps)), same_strand=(strand == "+"),
                                                                    sep1=seps or None, sep2=seps or None), ("+", "-"))


CASES = {
    "synth3": lambda g: pair_case(g, *seqio.synth_pair(400_000, 400_000, seed=3)),
    "synth4": lambda g: pair_case(g, *seqio.synth_pair(300_000, 500_000, seed=4)),
    "synth2m": lambda g: pair_case(g, *seqio.synth_pair(2_000_000, 2_000_000, seed=12)),
    "tandem": lambda g: pair_case(g, *tandem_pair()),
    "two_transitions": lambda g: pair_case(g, *seqio.synth_pair(300_000, 300_000, seed=6), with_trans=2),
    "chunks": lambda g: pair_case(g, *seqio.synth_pair(1_000_000, 1_000_000, seed=7), capacity=150_000),
    "self_plain": self_case,
}


def run(g, case):
    return CASES[case](g)
