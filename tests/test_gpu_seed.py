"""Parity tests proper for the seed stage (B1 + B2): the HIP path, called through the C ABI,
against the oracle / the reference's golden vectors.  Bit-exact: integer scores, coordinates,
order and work counters.  Needs an MI355X."""
import os
import subprocess
import sys
import numpy as np
import pytest

from oracle import lzo
from lastz_amd import seqio, lzgpu
import helpers as H

pytestmark = pytest.mark.gpu
CTB = lzo.upper_nuc_to_bits()


def _prep(gpu, t, pattern=H.DEFAULT_SEED, wt=1, step=1, start=0, end=0):
    sd = gpu.seed(pattern, wt)
    gpu.table_prepare(t, sd, CTB, step=step, start=start, end=end)
    return lzo.Table(t, lzo.seed(pattern, wt), step=step, start=start, end=end)


def _same_hsps(gpu, tab, qq, masked, **kw):
    gpu.counters_reset()
    got = gpu.seed_hit_search(masked, q=qq, **kw)
    okw = dict(kw)
    mode = 0 if okw.pop("extend", True) else 1
    want, st = lzo.seed_hit_search(tab, qq, masked, mode=mode, **okw)
    assert len(got) == len(want)
    assert (got == want).all()
    c = gpu.counters()
    assert c["words"] == st["words"] and c["raw_hits"] == st["raw_hits"]
    if mode == 0:
        assert c["extensions"] == st["extensions"] and c["bp_extended"] == st["bp_extended"] and c["hsps"] == st["hsps"]
    return got


@pytest.mark.parametrize("pattern,wt,step,start,end", [(H.DEFAULT_SEED, 1, 1, 0, 0), ("11111111", 0, 1, 0, 0),
                                                        ("111101101111", 1, 3, 0, 0), (H.DEFAULT_SEED, 1, 1, 1000, 15000),
                                                        ("1111111111", 0, 25, 7, 18000)])
def test_position_table_matches_reference_layout(gpu, pattern, wt, step, start, end):
    """B1: device CSR table, exported in the reference's last[]/prev[] layout, equals the oracle's
    restatement of build_seed_position_table (which is pinned against the reference)."""
    tgt = seqio.read_fasta(os.path.join(H.GOLDEN, "pseudocat.fa"))[0][1].copy()
    tgt[5000:5040] = ord("N"); tgt[9000:9100] |= 0x20           # bytes that break words
    tab = _prep(gpu, tgt, pattern, wt, step, start, end)
    pt = tab.pt.contents
    assert gpu.table_num_words() == pt.words_in_table
    last, prev = gpu.table_export(pt.prev_entries)
    assert (last == np.ctypeslib.as_array(pt.last, shape=(pt.word_entries,))).all()
    assert (prev == np.ctypeslib.as_array(pt.prev, shape=(pt.prev_entries,))).all()


def test_table_file_round_trip(gpu, tmp_path):
    """SURVEY 8f N4 (the capsule's role): a table saved to this library's versioned file, loaded into a fresh library
    state, gives the same table and the same HSPs; damaged and foreign files are refused."""
    t, q = seqio.synth_pair(300_000, 120_000, seed=77)
    _, masked = H.scoring()
    tab = _prep(gpu, t, "111101101111", 1, 2, 500, 290_000)
    f = str(tmp_path / "t.lztab")
    gpu.table_save(f)
    gpu.shutdown(); gpu.init()
    gpu.table_load(f)
    pt = tab.pt.contents
    assert gpu.table_num_words() == pt.words_in_table
    last, prev = gpu.table_export(pt.prev_entries)
    assert (last == np.ctypeslib.as_array(pt.last, shape=(pt.word_entries,))).all()
    assert (prev == np.ctypeslib.as_array(pt.prev, shape=(pt.prev_entries,))).all()
    for strand in (0, 1):
        qq = q if strand == 0 else seqio.revcomp(q)
        _same_hsps(gpu, tab, qq, masked, xdrop=910, hsp_threshold=3000)
    raw = bytearray(open(f, "rb").read())
    raw[len(raw) // 2] ^= 0x40
    open(f, "wb").write(bytes(raw))
    with pytest.raises(lzgpu.LzGpuError, match="checksum"):
        gpu.table_load(f)
    open(f, "wb").write(bytes(raw[:len(raw) // 3]))
    with pytest.raises(lzgpu.LzGpuError, match="truncated"):
        gpu.table_load(f)
    open(f, "wb").write(b"not a table" * 20)
    with pytest.raises(lzgpu.LzGpuError, match="not a version-1 table"):
        gpu.table_load(f)
    gpu.table_prepare(t, gpu.seed(H.DEFAULT_SEED, 1), CTB)       # and the library recovers
    assert gpu.table_num_words() > 0


def test_reference_goldens_hits_and_hsps(gpu):
    """base_test.hits.lav (raw hits, plain processor) and base_test.hsp.lav (X-drop HSPs)"""
    tgt = seqio.read_fasta(os.path.join(H.GOLDEN, "pseudocat.fa"))[0][1]
    qs = seqio.read_fasta(os.path.join(H.GOLDEN, "pseudopig.fa"))
    _, masked = H.scoring()
    _prep(gpu, tgt, "11111111", 0)
    gold_hits = H.lav_blocks(os.path.join(H.GOLDEN, "base_test.hits.lav"))
    gold_hsp = H.lav_blocks(os.path.join(H.GOLDEN, "base_test.hsp.lav"))
    mine = []
    for ci, (_, q) in enumerate(qs):
        hits = gpu.seed_hit_search(masked, q=q, extend=False)
        assert [((int(h["pos1"]) - 7, int(h["pos2"]) - 7), (int(h["pos1"]), int(h["pos2"]))) for h in hits] == \
               [(b["b"], b["e"]) for b in gold_hits[ci][2]]
        for _, rev, qq in H.strands(q):
            hsps = gpu.seed_hit_search(masked, q=qq)
            if len(hsps):
                mine.append((ci + 1, rev, [(int(h["score"]), int(h["pos1"] - h["length"]) + 1, int(h["pos2"] - h["length"]) + 1,
                                            int(h["pos1"]), int(h["pos2"])) for h in hsps]))
    assert mine == [(c, r, [(b["score"],) + b["b"] + b["e"] for b in bl]) for c, r, bl in gold_hsp]


@pytest.mark.parametrize("case,cap", [("synth200k", None), ("synth200k", 30000), ("synth_overlap", None), ("adversarial", 4096)])
def test_golden_cases_against_reference_output(gpu, case, cap):
    """HSP rows and collect_stats counters produced by the pristine reference (tests/golden)"""
    t, q = H.load_case(case)
    _, masked = H.scoring()
    _prep(gpu, t)
    gpu.set_hit_capacity(cap or (1 << 28))
    gold = H.read_hsp_tsv(os.path.join(H.GOLDEN, case + ".hsp.tsv"))
    gst = H.load_stats(case)
    rows = []
    gpu.counters_reset()
    for strand, _, qq in H.strands(q):
        rows += H.hsps_as_tsv_rows("query", strand, gpu.seed_hit_search(masked, q=qq))
    gpu.set_hit_capacity(1 << 28)
    assert rows == gold
    c = gpu.counters()
    for k in ("words", "raw_hits", "extensions", "bp_extended", "hsps"):
        assert c[k] == gst[k], k


def test_seeds_steps_thresholds_vs_oracle(gpu):
    t, q = seqio.synth_pair(120000, 90000, seed=31, block_min=500, block_max=4000)
    _, masked = H.scoring()
    for pattern, wt, step, kw in [("111101101111", 1, 3, {}), ("11111111", 2, 1, dict(hsp_threshold=2000, xdrop=500)),
                                  ("1111111111", 0, 1, dict(entropic=False)), (H.DEFAULT_SEED, 0, 1, dict(extend=False))]:
        tab = _prep(gpu, t, pattern, wt, step)
        for _, _, qq in H.strands(q):
            _same_hsps(gpu, tab, qq, masked, **kw)


def test_edge_cases(gpu):
    _, masked = H.scoring()
    t, q = seqio.synth_pair(30000, 30000, seed=9)
    tab = _prep(gpu, t)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    assert len(gpu.seed_hit_search(masked, q=acgt[[0, 1, 2]])) == 0          # shorter than the seed
    assert len(gpu.seed_hit_search(masked, q=np.full(5000, ord("N"), np.uint8))) == 0
    _same_hsps(gpu, tab, q | 0x20, masked)                                    # all lower case
    _same_hsps(gpu, tab, q, masked, start=1234, end=20001)                    # sub-interval of the query
    q2 = q.copy(); q2[::97] = ord("N"); q2[5000:5600] |= 0x20
    _same_hsps(gpu, tab, q2, masked)
    # ragged: query much shorter / longer than the target, target == tiny
    _same_hsps(gpu, tab, q[:200], masked)
    tab2 = _prep(gpu, t[:100])
    _same_hsps(gpu, tab2, q, masked)
    # a seed hit at the very ends of both sequences
    tab3 = _prep(gpu, t)
    q3 = np.concatenate([t[:40], q[:5000], t[-40:]])
    _same_hsps(gpu, tab3, q3, masked, hsp_threshold=1500)


def test_matrix_with_more_than_8_classes(gpu):
    """general (masked, 32x32-table) scan path instead of the whole-block 8x8 one"""
    t, q = seqio.synth_pair(150000, 120000, seed=77, block_min=500, block_max=3000)
    q = q.copy(); q[::53] = ord("R"); q[7::61] = ord("Y"); q[3000:3500] |= 0x20; q[11::97] = ord("N")
    m = H.many_class_scoring()
    tab = _prep(gpu, t)
    for _, _, qq in H.strands(q):
        _same_hsps(gpu, tab, qq, m, hsp_threshold=2200)
    _, masked = H.scoring()
    _same_hsps(gpu, tab, q, masked)                         # and back: the class tables are re-derived


def test_scan_modes_lut_and_byte_code(gpu):
    """phase A: look-up-table scans on 2-bit codes without (0) / with (1) special-byte masks, byte-code scans
    (2); each forced downgrade gives the oracle's answer too (src/seed_search.c:2623-2632, 2684-2693)"""
    _, masked = H.scoring()
    t, q = H.load_case("synth200k")
    ta, qa = H.load_case("adversarial")
    try:
        for forced in (0, 1, 2):
            gpu.set_scan_mode(forced)
            tab = _prep(gpu, t)
            for _, _, qq in H.strands(q):
                _same_hsps(gpu, tab, qq, masked)
                assert gpu.last_scan_mode() == forced
            tab = _prep(gpu, ta)
            gpu.set_hit_capacity(5000)
            for _, _, qq in H.strands(qa):
                _same_hsps(gpu, tab, qq, masked)
                assert gpu.last_scan_mode() == max(forced, 1)
            gpu.set_hit_capacity(1 << 28)
        gpu.set_scan_mode(0)
        qr = q.copy(); qr[::997] = ord("R")                # fillScore (-100) does not end a scan: consumed with its real score,
        tab = _prep(gpu, t)                                # the scan goes on behind it (round 4; byte-code scans before)
        _same_hsps(gpu, tab, qr, masked)
        assert gpu.last_scan_mode() == 1
    finally:
        gpu.set_scan_mode(0); gpu.set_hit_capacity(1 << 28)


@pytest.mark.parametrize("seed", [4, 5])
def test_lut_scans_through_special_bytes_that_do_not_end_a_scan(gpu, seed):
    """IUPAC bytes single, in pairs and in runs (fillScore -100 in lastz's matrices, partial credit in the many-class
    matrix): a scan consumes them with their real scores and goes on behind them; lower case still ends it"""
    rng = np.random.default_rng(seed)
    t, q = seqio.synth_pair(400000, 300000, seed=200 + seed, block_min=300, block_max=3000)
    t = t.copy(); q = q.copy()
    iupac = np.frombuffer(b"RYKMSWBDHV", dtype=np.uint8)
    for arr in (t, q):
        n = len(arr)
        idx = rng.integers(0, n, n // 25)
        arr[idx] = iupac[rng.integers(0, len(iupac), len(idx))]
        for s in rng.integers(0, n - 20, 400):
            k = int(rng.integers(2, 12))
            arr[s:s + k] = iupac[rng.integers(0, len(iupac), k)]
        arr[rng.integers(0, n, n // 300)] |= 0x20
    _, masked = H.scoring()
    tab = _prep(gpu, t)
    for _, _, qq in H.strands(q):
        _same_hsps(gpu, tab, qq, masked, hsp_threshold=1800)
    assert gpu.last_scan_mode() == 1
    for _, _, qq in H.strands(q):
        _same_hsps(gpu, tab, qq, H.many_class_scoring(), hsp_threshold=1800, xdrop=600)
    assert gpu.last_scan_mode() == 1


@pytest.mark.parametrize("seed", [1, 2])
def test_lut_scans_dense_specials_short_sequences(gpu, seed):
    """special bytes every few bases, sequence ends inside the scan windows, several xDrop values"""
    rng = np.random.default_rng(seed)
    t, q = seqio.synth_pair(300000, 240000, seed=100 + seed, block_min=300, block_max=2500)
    t = t.copy(); q = q.copy()
    for arr in (t, q):
        n = len(arr)
        arr[rng.integers(0, n, n // 40)] |= 0x20
        for s in rng.integers(0, n - 50, 600):
            arr[s:s + int(rng.integers(1, 40))] = ord("N")
    _, masked = H.scoring()
    tab = _prep(gpu, t)
    for xd in (910, 400, 375, 374):
        for _, _, qq in H.strands(q):
            _same_hsps(gpu, tab, qq, masked, xdrop=xd, hsp_threshold=2000)
        assert gpu.last_scan_mode() == (1 if xd >= 375 else 2)
    tab = _prep(gpu, t[:300], "11111111", 0)
    _same_hsps(gpu, tab, q[:200], masked, hsp_threshold=800)


def test_bucket_ownership_sharding_inside_one_query(gpu):
    """the hashed-diagonal buckets dealt out to n processes; merged lists == the single list"""
    from lastz_amd import shard
    t, q = seqio.synth_pair(400000, 300000, seed=41, block_min=500, block_max=6000)
    _, masked = H.scoring()
    tab = _prep(gpu, t)
    try:
        for qq in (q, seqio.revcomp(q)):
            gpu.set_bucket_owner(1, 0)
            gpu.counters_reset()
            whole = gpu.seed_hit_search(masked, q=qq)
            cw = gpu.counters()
            want, _ = lzo.seed_hit_search(tab, qq, masked)
            assert len(whole) == len(want) and (whole == want).all()
            for n in (2, 3, 8):
                parts, tot = [], dict(raw_hits=0, extensions=0, bp_extended=0, hsps=0)
                for r in range(n):
                    gpu.set_bucket_owner(n, r)
                    gpu.counters_reset()
                    h = gpu.seed_hit_search(masked, q=qq)
                    parts.append((h, gpu.last_hsp_order(len(h))))
                    c = gpu.counters()
                    assert c["words"] == cw["words"]
                    for k in tot: tot[k] += c[k]
                merged = shard.merge_bucket_owners(parts)
                assert len(merged) == len(whole) and (merged == whole).all()
                assert all(tot[k] == cw[k] for k in tot)
    finally:
        gpu.set_bucket_owner(1, 0)


def test_diag_hash_collisions_and_long_hsps(gpu):
    """tandem repeats: thousands of hits per hashed diagonal, clipped left extensions"""
    t, q = H.load_case("adversarial")
    _, masked = H.scoring()
    big_t = np.concatenate([t, seqio.synth_pair(140000, 10, seed=1)[0], t[::-1].copy()])   # > 65536 apart copies
    tab = _prep(gpu, big_t)
    for _, _, qq in H.strands(np.concatenate([q, q])):
        _same_hsps(gpu, tab, qq, masked)


def test_two_mbp_pair_and_capacity_invariance(gpu):
    t, q = seqio.synth_pair(2_000_000, 2_000_000, seed=12)
    _, masked = H.scoring()
    tab = _prep(gpu, t)
    for _, _, qq in H.strands(q):
        a = _same_hsps(gpu, tab, qq, masked)
        gpu.set_hit_capacity(300000)
        b = gpu.seed_hit_search(masked, q=qq)
        gpu.set_hit_capacity(1 << 28)
        assert (a == b).all()


def test_many_small_chunks_in_a_fresh_process(gpu, tmp_path):
    """many small chunks (hit capacities 150,000 and 700,000: about 21 and 5 per strand, about nine tiles per small one),
    both strands, in a fresh process: diagEnd carries from chunk to chunk, and the HSP list is the one-chunk list of
    this process.  Once on the fused scan path (LZGPU_FUSED_SCAN unset) and once on the split one (=0)."""
    t, q = seqio.synth_pair(2_000_000, 2_000_000, seed=12)
    _, masked = H.scoring()
    _prep(gpu, t)
    want = [gpu.seed_hit_search(masked, q=qq) for _, _, qq in H.strands(q)]
    np.save(tmp_path / "want0.npy", want[0]); np.save(tmp_path / "want1.npy", want[1])
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from lastz_amd import seqio, lzgpu; import helpers as H; from oracle import lzo\n"
            "g = lzgpu.Lib(); g.init()\n"
            "t, q = seqio.synth_pair(2_000_000, 2_000_000, seed=12); _, masked = H.scoring()\n"
            "g.table_prepare(t, g.seed(H.DEFAULT_SEED, 1), lzo.upper_nuc_to_bits())\n"
            "for cap in (150000, 700000):\n"
            "    g.set_hit_capacity(cap)\n"
            "    for k, (_, _, qq) in enumerate(H.strands(q)):\n"
            "        got = g.seed_hit_search(masked, q=qq); want = np.load(%r %% k)\n"
            "        assert len(got) == len(want) and (got == want).all(), (cap, k)\n"
            "print('chunks ok')\n" % (H.ROOT, os.path.join(H.ROOT, "tests"), str(tmp_path / "want%d.npy")))
    for fused in (None, "0"):
        env = dict(os.environ); env.pop("LZGPU_FUSED_SCAN", None)
        if fused is not None:
            env["LZGPU_FUSED_SCAN"] = fused
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0 and "chunks ok" in r.stdout, (fused, r.stdout + r.stderr)


def test_same_results_after_shutdown_and_init(gpu):
    """a search in several chunks (blk_start holds several blocks of positions) and an opposite-strand self search of a
    [multi] sequence (self_sep holds its separators), then shutdown + init: the same two searches give the same HSPs
    and counters as before.  A guard on results: that shutdown releases every buffer is read off
    LzCtx::release_device_memory (lz_ctx.hpp), not shown here -- on one device a stale pointer would still work."""
    import self_cases as S
    _, masked = H.scoring()
    t, q = seqio.synth_pair(300_000, 120_000, seed=77)
    c = S.CASES["multi_ragged"]
    v, seps, _ = S.sequence("multi_ragged")

    def searches():
        try:
            gpu.set_hit_capacity(4096)                      # ~28,000 expected hits: 16 blocks, several chunks
            tab = _prep(gpu, t)
            a = _same_hsps(gpu, tab, q, masked)
            ca = gpu.counters()
        finally:
            gpu.set_hit_capacity(1 << 28)
        gpu.table_prepare(v, gpu.seed(c["pattern"], c["trans"]), CTB, step=c["step"])
        gpu.counters_reset()
        b = gpu.seed_hit_search_self(masked, q=S.minus(v, seps), same_strand=False, sep1=seps, sep2=seps)
        return a, ca, b, gpu.counters()

    a0, ca0, b0, cb0 = searches()
    want, _ = lzo.seed_hit_search(lzo.Table(v, lzo.seed(c["pattern"], c["trans"]), step=c["step"]), S.minus(v, seps), masked,
                                  self_strand="opposite", sep1=seps, sep2=seps)
    assert len(a0) > 0 and len(b0) == len(want) > 0 and (b0 == want).all()
    gpu.shutdown(); gpu.init()
    a1, ca1, b1, cb1 = searches()
    assert len(a1) == len(a0) and (a1 == a0).all() and ca1 == ca0
    assert len(b1) == len(b0) and (b1 == b0).all() and cb1 == cb0


def test_full_task_regions_leave_hits_to_phase_b(gpu, tmp_path):
    """a scan that goes on past its first window becomes a task in its wave's region of the task list; with the
    regions forced down to two entries most such hits find theirs full, stay "alive" and are extended exactly by
    phase B instead -- same HSPs, same counters (fresh process: the cap is read once)"""
    t, q = seqio.synth_pair(1_000_000, 1_000_000, seed=31)
    _, masked = H.scoring()
    tab = _prep(gpu, t)
    want = [_same_hsps(gpu, tab, qq, masked) for _, _, qq in H.strands(q)]
    np.save(tmp_path / "w0.npy", want[0]); np.save(tmp_path / "w1.npy", want[1])
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from lastz_amd import seqio, lzgpu; import helpers as H; from oracle import lzo\n"
            "g = lzgpu.Lib(); g.init()\n"
            "t, q = seqio.synth_pair(1_000_000, 1_000_000, seed=31); _, masked = H.scoring()\n"
            "g.table_prepare(t, g.seed(H.DEFAULT_SEED, 1), lzo.upper_nuc_to_bits())\n"
            "for k, (_, _, qq) in enumerate(H.strands(q)):\n"
            "    got = g.seed_hit_search(masked, q=qq); want = np.load(%r %% k)\n"
            "    assert len(got) == len(want) and (got == want).all(), k\n"
            "print('regions ok')\n" % (H.ROOT, os.path.join(H.ROOT, "tests"), str(tmp_path / "w%d.npy")))
    env = dict(os.environ); env["LZGPU_TASK_REGION_CAP"] = "2"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "regions ok" in r.stdout, r.stdout + r.stderr


def test_full_size_properties(gpu):
    """BASELINE.json configs[1] size (50 Mbp x 50 Mbp, one strand): properties that do not
    need the oracle -- determinism, chunk-capacity invariance, every HSP re-scores to its score on
    the host, HSPs arrive in discovery-compatible order, counters obey H >= E >= HSPs."""
    t, q = seqio.synth_pair(50_000_000, 50_000_000, seed=1000)        # the exact pair bench.py times
    sub, masked = H.scoring()
    _prep(gpu, t)
    gpu.counters_reset()
    a = gpu.seed_hit_search(masked, q=q)
    c = gpu.counters()
    # ... and one check that does: the SHA-256 of the pristine reference's HSP list for this pair, both strands
    # (tests/golden/bench50m.sha.json, made by tests/golden/make_bench_sha.py in 40 minutes of CPU)
    import json, bench
    gold = json.load(open(os.path.join(H.GOLDEN, "bench50m.sha.json")))
    sha, rows = bench.hsp_rows_sha([a, gpu.seed_hit_search(masked, q=seqio.revcomp(q))])
    assert rows == gold["hsp_rows"] and sha == gold["hsp_sha"]
    gpu.set_hit_capacity(1 << 26)
    b = gpu.seed_hit_search(masked, q=q)
    gpu.set_hit_capacity(1 << 28)
    assert len(a) > 1000 and (a == b).all()
    assert c["raw_hits"] >= c["extensions"] >= c["hsps"] == len(a)
    assert c["words"] == len(q) - 18
    # expected random hits ~ 13 * T * Q / 2^24; within 10 %
    model = 13.0 * len(t) * len(q) / 2 ** 24
    assert 0.9 * model < c["raw_hits"] < 1.3 * model
    rng = np.random.default_rng(0)
    for h in a[rng.integers(0, len(a), 300)]:
        s1, s2, n = int(h["pos1"] - h["length"]), int(h["pos2"] - h["length"]), int(h["length"])
        raw = int(masked[t[s1:s1 + n], q[s2:s2 + n]].sum())
        assert raw >= h["score"] >= 3000                      # entropy only ever lowers a score
        if raw > 9000:
            assert raw == h["score"]


def test_north_star_pair_against_the_reference_fingerprints(gpu):
    """BASELINE.json north_star size (200 Mbp x 200 Mbp, both strands): the HSP list of the seed stage and the alignments of the gapped
    stage against the pristine reference's output for this exact pair (tests/golden/bench200m.sha.json: four one-strand reference
    processes of ~5.4 h each, tests/golden/make_bench200m_sha.py).  The LAV's own SHA is checked by bench.py through the bound CLI."""
    import json, bench
    from lastz_amd import lzgpu
    gold = json.load(open(os.path.join(H.GOLDEN, "bench200m.sha.json")))
    t, q = seqio.synth_pair(gold["tlen"], gold["qlen"], seed=gold["seed"])
    sub, masked = H.scoring()
    gpu.table_prepare(t, gpu.seed(H.DEFAULT_SEED, 1), CTB)
    gpu.set_hit_capacity(1 << 31)
    gpu.query_upload(0, q); gpu.query_upload(1, seqio.revcomp(q))
    hs = [gpu.seed_hit_search(masked, slot=s) for s in (0, 1)]
    gpu.set_hit_capacity(1 << 28)
    sha, rows = bench.hsp_rows_sha(hs)
    assert rows == gold["hsp_rows"] and sha == gold["hsp_sha"]
    res = gpu.gapped_extend_batch(sub, [dict(anchors=bench.hsps_to_segs(lzgpu, h, s), slot=s, ydrop=9430) for s, h in enumerate(hs)])
    assert sum(len(al) for al, _ in res) == gold["lav_blocks"]
    # ... and their bytes (VERDICT r4 #3d): written out as the reference writes a LAV -- score, begin, end, every gap-free piece and its
    # identity column, block by block -- the batch's alignments have the fingerprint of the file the pristine reference wrote for the pair
    from lastz_amd import lav
    assert lav.fingerprint(lav.render(t, [q, seqio.revcomp(q)], res, sub)) == gold["lav_sha"]


@pytest.mark.skipif(lzo.ref_binary() is None, reason="oracle/_ref/lastz not present")
def test_live_against_reference_binary(gpu, tmp_path):
    """same run, same inputs: the pristine reference binary vs the HIP path"""
    t, q = seqio.synth_pair(1_000_000, 1_000_000, seed=77)
    tf, qf = str(tmp_path / "t.fa"), str(tmp_path / "q.fa")
    seqio.write_fasta(tf, [("target", t)]); seqio.write_fasta(qf, [("query", q)])
    out = H.ref_run([tf, qf, "--nogapped", "--format=general-:name2,start1,end1,start2,end2,strand2,score"])
    gold = [(f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4]), f[5], int(f[6]))
            for f in (ln.split("\t") for ln in out.split("\n") if ln)]
    _, masked = H.scoring()
    _prep(gpu, t)
    rows = []
    for strand, _, qq in H.strands(q):
        rows += H.hsps_as_tsv_rows("query", strand, gpu.seed_hit_search(masked, q=qq))
    assert rows == gold


def test_resident_query_slots_and_torch_first_process(gpu):
    """bench.py's mode: queries resident in HBM; and the library loaded AFTER torch (so that it binds
    the HIP runtime torch brought in), in a fresh process."""
    t, q = H.load_case("synth200k")
    _, masked = H.scoring()
    tab = _prep(gpu, t)
    gpu.query_upload(0, q); gpu.query_upload(1, seqio.revcomp(q))
    for slot, (_, _, qq) in enumerate(H.strands(q)):
        want, _ = lzo.seed_hit_search(tab, qq, masked)
        got = gpu.seed_hit_search(masked, slot=slot)
        assert (got == want).all()
    code = ("import torch, sys; sys.path.insert(0, %r); import __graft_entry__ as g; "
            "torch.cuda.init(); g.smoke()" % H.ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


def test_bench_plain_line_and_dumped_outputs(gpu, tmp_path):
    """bench.py without --full: one JSON line with the contract's keys and none of the --full legs; --dump-outputs writes the HSP lists
    of the last timed step, and they are the library's own for the same pair, field by field"""
    import json, bench
    d = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(H.ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--tlen", "2000000", "--qlen", "2000000", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=H.ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.split("\n")
    assert len(lines) == 2 and lines[1] == "", p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "Gbp/s" and line["higher_is_better"] is True and line["dtype"] == "s32" and "Gbp-of-target" in line["metric"]
    assert not {"parity", "gapped", "chain", "cli", "north_star", "content", "cpu_baseline", "configs2"} & set(line)
    t, q = seqio.synth_pair(2_000_000, 2_000_000, seed=1000)
    _, masked = H.scoring()
    _prep(gpu, t)
    want = [gpu.seed_hit_search(masked, q=qq) for qq in (q, seqio.revcomp(q))]
    assert line["hsps"] == len(want[0]) + len(want[1]) > 100
    for name, w in zip(("hsp_plus", "hsp_minus"), want):
        assert np.load(d / (name + "_rows.npy")).tolist() == [len(w)]
        for f in bench.HSP_FIELDS:
            got = np.load(d / ("%s_%s.npy" % (name, f)))
            assert got.dtype == np.float64 and (got == w[f]).all()


def test_window_search_of_many_rectangles(gpu):
    """lzgpu_window_search: the table + search of src/tweener.c's in-between windows -- an exact 7-mer on
    rectangles of at most 20 kbp a side, no entropy -- for all windows in one launch, against the oracle run on the
    cut-out pieces: same HSPs, same order, window coordinates.  With a low-complexity stretch (one word's list longer
    than the kernel's hit buffer), lower case and N runs, windows at the sequence ends, empty and tiny windows."""
    t, q = H.load_case("synth200k")
    t = t.copy(); q = q.copy()
    t[30000:37000] = ord("A"); q[28000:33500] = ord("A")          # a word with thousands of positions
    t[52000:52400] = ord("N"); q[51000:51050] = ord("n"); q[60000:60300] |= 32      # bytes that cannot be in a seed word / score as masked
    _, masked = H.scoring()
    gpu.table_prepare(t, gpu.seed(), CTB)
    gpu.query_upload(3, q)
    rng = np.random.default_rng(11)
    wins = [(27000, 12000, 26000, 9000), (0, 20000, 0, 20000), (len(t) - 20480, 20480, len(q) - 20480, 20480),
            (40000, 3, 40000, 5000), (40000, 5000, 40000, 0), (51000, 3000, 50500, 2000)]
    for _ in range(40):
        tl, ql = int(rng.integers(50, 20000)), int(rng.integers(50, 20000))
        t0 = int(rng.integers(0, len(t) - tl))
        q0 = min(max(0, t0 + int(rng.integers(-3000, 3000))), len(q) - ql)
        wins.append((t0, tl, q0, ql))
    isd, osd = gpu.seed("1111111", 0), lzo.seed("1111111", 0)
    for thr in (2200, 3000):
        got = gpu.window_search(masked, wins, isd, CTB, slot=3, hsp_threshold=thr)
        total = 0
        for (t0, tl, q0, ql), g in zip(wins, got):
            tt, qq = t[t0:t0 + tl], q[q0:q0 + ql]
            want = np.zeros(0, dtype=lzgpu.HSP_DTYPE)
            if tl >= 7 and ql >= 7:
                want, _ = lzo.seed_hit_search(lzo.Table(tt, osd), qq, masked, hsp_threshold=thr, entropic=False)
            assert len(g) == len(want) and (g == want).all(), (t0, tl, q0, ql)
            total += len(g)
        assert total > 50
    # the query may also come as host bytes; a window outside the sequences is an error, a window too large is declined
    again = gpu.window_search(masked, wins[:3], isd, CTB, q=q, hsp_threshold=2200)
    assert all((x == y).all() for x, y in zip(again, gpu.window_search(masked, wins[:3], isd, CTB, slot=3, hsp_threshold=2200)))
    with pytest.raises(Exception):
        gpu.window_search(masked, [(len(t) - 10, 100, 0, 100)], isd, CTB, slot=3)
    with pytest.raises(Exception):
        gpu.window_search(masked, [(0, 30000, 0, 100)], isd, CTB, slot=3)
