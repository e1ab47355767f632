// emul_tile_cursor.cpp -- TEST INFRASTRUCTURE: the rank -> record mapping of phase B with the entry cursor
// (lastz_amd/csrc/lz_tile_runs.hpp, lz_settle_sorters.inc) run on the CPU, for tests/test_tile_cursor.py.  Never linked
// into liblzgpu.so.
//
// The same interface and invariants as emul_tile_runs.cpp, which replays the procedure k_settle2 had before (a mark per run,
// a running maximum over the window).  Restated here, lane by lane: what k_partition leaves (tiles sorted in place, hist,
// run_addr), the two k_hist_scan kernels, and a sorter wave's load_block / advance_early / load_tile with the cursor: the
// entry that holds the first covered rank from a count over the block, then one wave-uniform (entry, displacement, next
// first rank) that steps through the rounds of 64 ranks.  The arithmetic is the header's.
#include <string.h>
#include <vector>
#include "../../lastz_amd/csrc/lz_tile_runs.hpp"

namespace {
struct Wave {                                    // a sorter wave's cursor block
    u32 cur = 0, bf[64][LZ_TR_K], ba[64][LZ_TR_K];
    u64 loads = 0;
};
struct Tables { const u32 *hist, *part, *run_addr; u32 ntiles; };
u64 g_round_steps = 0;                           // most cursor steps inside one round, of the last call

void load_block(Wave& w, const Tables& T, u32 p, u32 r1)
{
    for (u32 lane = 0; lane < 64; lane++) for (u32 j = 0; j < LZ_TR_K; j++) {
        const u32 t = w.cur + lane * LZ_TR_K + j;
        w.bf[lane][j] = lz_tr_first(T.hist, T.part, T.ntiles, t, p, r1);
        w.ba[lane][j] = t < T.ntiles ? T.run_addr[(size_t)t * LZ_TR_NBIN + p] : 0u;
    }
    w.loads++;
}
u32 block_end(const Wave& w) { return w.bf[63][LZ_TR_K - 1]; }
// entry e of the block (the kernel: readlane at a wave-uniform index); e past the block is the procedure's own fault
bool entry_of(const u32 (*b)[LZ_TR_K], u32 e, u32& v) { if (e >= LZ_TR_BLOCK) return false; v = b[e / LZ_TR_K][e % LZ_TR_K]; return true; }

// the window [g0, g1) of partition p: idx[k] = index of rank g0 + k in the record array; returns the cursor moves it took
u32 locate_window(Wave& w, const Tables& T, u32 p, u32 r1, u32 g0, u32 g1, u32 window, u32* idx, u32* covered)
{
    u32 moves = 0;
    for (;;) {
        const u32 bend = block_end(w);
        if (!lz_tr_block_behind(bend, g0)) {
            const u32 bfirst = w.bf[0][0];
            const u32 s = lz_tc_start(g0, bfirst), lim = lz_tc_limit(g1, bend);
            if (s < lim) {
                u32 e = ~0u;                                    // the ballots' popcounts
                for (u32 j = 0; j < LZ_TR_K; j++) for (u32 lane = 0; lane < 64; lane++) e += lz_tc_at_or_below(w.bf[lane][j], s) ? 1u : 0u;
                u32 nf, a, f;
                if (e >= LZ_TR_BLOCK - 1) return ~0u;           // (no entry at or below s, or the bounding entry: never)
                if (!entry_of(w.bf, e + 1, nf) || !entry_of(w.ba, e, a) || !entry_of(w.bf, e, f)) return ~0u;
                u32 dcur = lz_tr_delta(a, f);
                for (u32 rr = 0; rr * 64u < window; rr++) {
                    const u32 base = g0 + rr * 64u;
                    u32 d[64];
                    for (u32 lane = 0; lane < 64; lane++) d[lane] = dcur;
                    u64 steps = 0;
                    while (lz_tc_step(nf, base, lim)) {
                        e++; steps++;
                        if (e >= LZ_TR_BLOCK - 1) return ~0u;   // the bounding entry is never taken as a run
                        if (!entry_of(w.ba, e, a)) return ~0u;
                        dcur = lz_tr_delta(a, nf);
                        for (u32 lane = 0; lane < 64; lane++) if (lz_tc_take(base + lane, nf)) d[lane] = dcur;
                        if (!entry_of(w.bf, e + 1, nf)) return ~0u;
                    }
                    if (steps > g_round_steps) g_round_steps = steps;
                    for (u32 lane = 0; lane < 64; lane++) {
                        const u32 g = base + lane;
                        if (lz_tr_covers(g, bfirst, bend, g1)) { idx[g - g0] = lz_tr_index(g, d[lane]); covered[g - g0]++; }
                    }
                }
            }
            if (bend >= g1) break;
        }
        w.cur += LZ_TR_BLOCK - 1; load_block(w, T, p, r1); moves++;
    }
    return moves;
}
}

// most cursor steps (runs entered, empty ones included) inside one round of 64 ranks during the last emul_tile_cursor
extern "C" u64 emul_tile_cursor_round_steps() { return g_round_steps; }

// vals[n] with partitions bins[n] -> out[n]: the records in partition-major order as the sorter waves of k_settle2 gather
// them (nwaves waves, windows of `window` ranks -- a multiple of 64 --, settle tiles of nwaves * window); bin_base[257];
// stats = { most cursor moves inside one window, block loads of the busiest wave, most block loads a wave may need }.
// Returns 0, or a negative code when the procedure broke one of its own invariants.
extern "C" int emul_tile_cursor(const u8* bins, const u64* vals, u64 n, u32 window, u32 nwaves, u64* out, u32* bin_base, u64* stats)
{
    const u32 TILE = LZ_PP_TILE_HOST, NB = LZ_TR_NBIN;
    const u32 ntiles = (u32)((n + TILE - 1) / TILE), nblocks = (ntiles + 255u) / 256u;
    if (window % 64u) return -4;
    g_round_steps = 0;
    std::vector<u64> recs(n);
    std::vector<u32> hist((size_t)ntiles * NB), run_addr((size_t)ntiles * NB), part((size_t)nblocks * NB + NB);
    // k_partition: every tile sorted by partition where it lies, stable
    for (u32 t = 0; t < ntiles; t++) {
        const u64 base = (u64)t * TILE;
        const u32 tile_n = n - base < TILE ? (u32)(n - base) : TILE;
        u32 cnt[NB] = {}, ts[NB];
        for (u32 k = 0; k < tile_n; k++) cnt[bins[base + k]]++;
        u32 acc = 0;
        for (u32 b = 0; b < NB; b++) { ts[b] = acc; acc += cnt[b]; hist[(size_t)t * NB + b] = cnt[b]; run_addr[(size_t)t * NB + b] = lz_tr_run_addr(t, ts[b]); }
        for (u32 k = 0; k < tile_n; k++) recs[base + ts[bins[base + k]]++] = vals[base + k];
    }
    // k_hist_scan1, k_hist_scan2
    for (u32 blk = 0; blk < nblocks; blk++) for (u32 b = 0; b < NB; b++) {
        u32 acc = 0;
        for (u32 t = blk * 256u; t < ntiles && t < blk * 256u + 256u; t++) { const u32 v = hist[(size_t)t * NB + b]; hist[(size_t)t * NB + b] = acc; acc += v; }
        part[(size_t)blk * NB + b] = acc;
    }
    {
        std::vector<u32> tot(NB);
        for (u32 b = 0; b < NB; b++) { u32 acc = 0; for (u32 blk = 0; blk < nblocks; blk++) { const u32 v = part[(size_t)blk * NB + b]; part[(size_t)blk * NB + b] = acc; acc += v; } tot[b] = acc; }
        u32 a = 0;
        for (u32 b = 0; b < NB; b++) { bin_base[b] = a; a += tot[b]; }
        bin_base[NB] = a;
        for (u32 b = 0; b < NB; b++) for (u32 blk = 0; blk < nblocks; blk++) part[(size_t)blk * NB + b] += bin_base[b];
    }
    // k_settle2's sorter waves
    const Tables T = { hist.data(), part.data(), run_addr.data(), ntiles };
    const u32 s2tile = window * nwaves;
    std::vector<u32> idx(window), covered(window);
    stats[0] = stats[1] = 0; stats[2] = (u64)ntiles / (LZ_TR_BLOCK - 1) + 1;
    for (u32 p = 0; p < NB; p++) {
        const u32 r0 = bin_base[p], r1 = bin_base[p + 1], np = r1 - r0, nst = (np + s2tile - 1) / s2tile;
        for (u32 sw = 0; sw < nwaves && nst; sw++) {
            Wave w;
            load_block(w, T, p, r1);
            for (u32 tt = 0; tt < nst; tt++) {
                const u32 g0 = r0 + tt * s2tile + sw * window;
                if (g0 >= r1) continue;
                u32 moves = 0;
                if (tt >= 3 && lz_tr_block_behind(block_end(w), g0)) { w.cur += LZ_TR_BLOCK - 1; load_block(w, T, p, r1); moves++; }   // advance_early
                const u32 g1 = (r1 - g0 < window) ? r1 : g0 + window;
                std::fill(covered.begin(), covered.end(), 0u);
                const u32 m = locate_window(w, T, p, r1, g0, g1, window, idx.data(), covered.data());
                if (m == ~0u) return -1;
                moves += m;
                if (moves > stats[0]) stats[0] = moves;
                for (u32 k = 0; g0 + k < g1; k++) {
                    if (covered[k] != 1u) return -2;            // every rank of the window in exactly one pass
                    if (idx[k] >= n) return -3;
                    out[g0 + k] = recs[idx[k]];
                }
                for (u32 k = g1 - g0; k < window; k++) if (covered[k]) return -5;      // and no rank past it
            }
            if (w.loads > stats[1]) stats[1] = w.loads;
        }
    }
    return 0;
}
