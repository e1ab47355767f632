// settle_kernels.hip -- gfx950 kernels behind phase A (DESIGN.md section 3, rows 6, 6b and 7, and the match counts row 8's
// host finish reads): every tile of hits sorted by partition where it lies, the runs' ranks, the bucket-serial walk with its
// wave-cooperative X-drop extension, and the candidates' entropy inputs; and the walk of an exact-match search (k_settle_exact).
#include <hip/hip_runtime.h>
#include <cstdio>
#include "lz_ctx.hpp"
#include "lz_lut.hpp"
#include "lz_tile_runs.hpp"
#include "lz_coop.hpp"
#include "lz_seed_dev.hpp"
#include "lz_exact.hpp"
#include "lz_mismatch.hpp"

// the tiles of k_partition (lz_tile_runs.hpp: LZ_PP_TILE_HOST sizes the tile tables on the host) and the 256 partitions
#define LZ_PP_TPB    1024                            // one workgroup per CU: 128 KiB of staging for a tile of 16384 hits (runs of 64 records per partition)
#define LZ_PP_WAVES  (LZ_PP_TPB / 64)
#define LZ_PP_ROUNDS (LZ_PP_TILE_HOST / LZ_PP_TPB)   // k_partition: records per lane
#define LZ_PP_TILE   (LZ_PP_TPB * LZ_PP_ROUNDS)      // hits per tile of k_partition
#define LZ_NBIN      256
static_assert(LZ_PP_TILE == LZ_PP_TILE_HOST, "lz_tile_runs.hpp addresses runs by the tile size");

// exclusive prefix sum over the first 256 threads of a workgroup (every thread of the workgroup calls it)
__device__ __forceinline__ u32 lz_exscan256(u32 v, u32* wtot /*LDS, [4]*/)
{
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    u32 inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const u32 t = __shfl_up(inc, d); if ((int)lane >= d) inc += t; }
    if (tid < 256 && lane == 63) wtot[w] = inc;
    __syncthreads();
    u32 pre = 0;
    if (tid < 256) for (u32 k = 0; k < w; k++) pre += wtot[k];
    return pre + inc - v;
}

// keys + summaries (or tagged records) -> records, every tile sorted by partition where it lies (lz_tile_runs.hpp).  One workgroup per tile;
// a wave owns 256 consecutive hits (64 per round), so ranks by (wave, round, lane) follow the discovery order.
struct LzPartShared {
    union alignas(16) {
        u64 stage[LZ_PP_TILE];                       // the tile's records, ordered by partition
        u64 bm[LZ_PP_WAVES][LZ_NBIN];                // peer bitmaps of the round in flight (all zero again before stage[] is written)
    };
    u32 wcnt[LZ_PP_WAVES][LZ_NBIN];                  // per wave and partition: records / running offset inside the partition
    u32 tstart[LZ_NBIN], wtot[4];
};
// the staged tile -> its own place in the record array, tags cleared: 16 bytes per lane, whole lines per wave
__device__ __forceinline__ void lz_part_store(const u64* stage, u32 tile_n, u64* out /*the tile's first record*/)
{
    typedef u64 lz_u64x2 __attribute__((ext_vector_type(2)));
    for (u32 k = threadIdx.x * 2u; k < tile_n; k += LZ_PP_TPB * 2u) {
        lz_u64x2 v = *reinterpret_cast<const lz_u64x2*>(stage + k);     // (k + 1 == tile_n: stage[k + 1] is inside stage[] and not stored)
        v.x = LZ_REC_UNTAG(v.x); v.y = LZ_REC_UNTAG(v.y);
        if (k + 1u < tile_n) *reinterpret_cast<lz_u64x2*>(out + k) = v;
        else out[k] = v.x;
    }
}
// TAGGED: recs holds tagged records (the fused path: the partition rides in bits 55..62); otherwise keys, whose summaries
// are in summ.  Either way the sort is in place: every record of the tile is in registers before the first store, and no
// other workgroup touches the tile.
template <bool TAGGED>
__global__ void __launch_bounds__(LZ_PP_TPB)
k_partition(u64* recs, u64 n, u32* __restrict__ hist, u32* __restrict__ run_addr, const u32* __restrict__ summ)
{
    __shared__ LzPartShared sh;
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const u32 tile = blockIdx.x;
    const u64 base = (u64)tile * LZ_PP_TILE;
    const u32 tile_n = (n - base < (u64)LZ_PP_TILE) ? (u32)(n - base) : (u32)LZ_PP_TILE;
    for (u32 k = tid; k < LZ_PP_WAVES * LZ_NBIN; k += LZ_PP_TPB) { (&sh.wcnt[0][0])[k] = 0; (&sh.bm[0][0])[k] = 0ull; }
    const u32 l0 = w * (64u * LZ_PP_ROUNDS) + lane;
    u64 kk[LZ_PP_ROUNDS]; u32 ss[LZ_PP_ROUNDS];
#pragma unroll
    for (u32 r = 0; r < LZ_PP_ROUNDS; r++) {
        const bool v = l0 + 64u * r < tile_n;
        kk[r] = v ? recs[base + l0 + 64u * r] : 0ull;             // (plain loads and stores here: non-temporal ones made this kernel 10-15 % slower)
        if (!TAGGED) ss[r] = v ? summ[base + l0 + 64u * r] : 0u;
    }
    __syncthreads();
    // The lanes of a round that hold the same partition find each other through a 64-bit bitmap in LDS (atomic OR of
    // 1 << lane, one read; the result does not depend on the order of the ORs), which gives rank and count in one pass and
    // leaves the per-wave totals behind -- no separate counting pass, no ballots.
    u32 slot[LZ_PP_ROUNDS];
#pragma unroll
    for (u32 r = 0; r < LZ_PP_ROUNDS; r++) {
        // (each wave works on its own rows of bm / wcnt: LDS operations of one wave execute in order)
        const bool valid = l0 + 64u * r < tile_n;
        const u32 bin = TAGGED ? LZ_REC_TAG(kk[r]) : LZ_KEY_BIN(kk[r]);
        if (valid) atomicOr((unsigned long long*)&sh.bm[w][bin], 1ull << lane);
        const u64 peers = valid ? sh.bm[w][bin] : 0ull;
        const u32 old = valid ? sh.wcnt[w][bin] : 0u;
        if (valid && (peers >> lane) == 1ull) { sh.wcnt[w][bin] = old + (u32)__popcll(peers); sh.bm[w][bin] = 0ull; }  // the highest peer
        slot[r] = old + (u32)__popcll(peers & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    // the per-partition counts chained in wave order in wcnt, the tile-local starts in tstart, the tile's two table rows
    u32 tot = 0;
    if (tid < LZ_NBIN) for (u32 k = 0; k < LZ_PP_WAVES; k++) { const u32 v = sh.wcnt[k][tid]; sh.wcnt[k][tid] = tot; tot += v; }
    const u32 ts = lz_exscan256(tot, sh.wtot);
    if (tid < LZ_NBIN) {
        sh.tstart[tid] = ts;
        hist[(size_t)tile * LZ_NBIN + tid] = tot;
        run_addr[(size_t)tile * LZ_NBIN + tid] = lz_tr_run_addr(tile, ts);
    }
    __syncthreads();
    // every record gets its place: rank among the same-partition lanes of its wave's round, on top of the wave's
    // running offset (stable: lanes, rounds and waves all follow the discovery order)
#pragma unroll
    for (u32 r = 0; r < LZ_PP_ROUNDS; r++) {
        const u32 bin = TAGGED ? LZ_REC_TAG(kk[r]) : LZ_KEY_BIN(kk[r]);
        if (l0 + 64u * r < tile_n) sh.stage[sh.tstart[bin] + sh.wcnt[w][bin] + slot[r]] = TAGGED ? kk[r] : lz_hit_record(kk[r], ss[r]);
    }
    __syncthreads();
    lz_part_store(sh.stage, tile_n, recs + base);
}

// the n hits of the chunk in c.keys -> records, in place.  tagged: the fused path's tagged records; otherwise keys, with their
// summaries in c.summ.  The tiles' counts -> c.hist, where their runs lie -> c.run_addr
int lzk_partition(LzCtx& c, bool tagged, u64 n)
{
    if (n == 0) return 0;
    if (!tagged && !c.summ.p) return LZGPU_ERR_ARG;
    const u32 ntiles = (u32)((n + LZ_PP_TILE - 1) / LZ_PP_TILE);
    u64* recs = c.keys.as<u64>(); u32* hist = c.hist.as<u32>(); u32* run_addr = c.run_addr.as<u32>();
    c.timer.begin("k_partition", c.stream);
    if (!tagged) hipLaunchKernelGGL(k_partition<false>, dim3(ntiles), dim3(LZ_PP_TPB), 0, c.stream, recs, n, hist, run_addr, c.summ.as<u32>());
    else         hipLaunchKernelGGL(k_partition<true>, dim3(ntiles), dim3(LZ_PP_TPB), 0, c.stream, recs, n, hist, run_addr, (const u32*)nullptr);
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    return 0;
}

// hist[tile][bin]: hits of the tile per partition, written by the partition kernels (lz_tile_runs.hpp)
// per block of 256 tiles: exclusive prefix down each column, column sums to part[block][bin]
__global__ void __launch_bounds__(LZ_NBIN)
k_hist_scan1(u32* __restrict__ hist, u32 ntiles, u32* __restrict__ part)
{
    const u32 t0 = blockIdx.x * 256u, t1 = (t0 + 256u < ntiles) ? t0 + 256u : ntiles;
    u32 acc = 0;
    for (u32 t = t0; t < t1; t++) { const size_t k = (size_t)t * LZ_NBIN + threadIdx.x; const u32 v = hist[k]; hist[k] = acc; acc += v; }
    part[(size_t)blockIdx.x * LZ_NBIN + threadIdx.x] = acc;
}
// one workgroup: part[block][bin] -> absolute offset of (block, bin); bin_base[0..256]
__global__ void __launch_bounds__(LZ_NBIN)
k_hist_scan2(u32* __restrict__ part, u32 nblocks, u32* __restrict__ bin_base)
{
    __shared__ u32 tot[LZ_NBIN];
    u32 acc = 0;
    for (u32 b = 0; b < nblocks; b++) { const size_t k = (size_t)b * LZ_NBIN + threadIdx.x; const u32 v = part[k]; part[k] = acc; acc += v; }
    tot[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) { u32 a = 0; for (int k = 0; k < LZ_NBIN; k++) { const u32 v = tot[k]; tot[k] = a; a += v; } bin_base[LZ_NBIN] = a; }
    __syncthreads();
    const u32 bb = tot[threadIdx.x];
    bin_base[threadIdx.x] = bb;
    for (u32 b = 0; b < nblocks; b++) part[(size_t)b * LZ_NBIN + threadIdx.x] += bb;
}

// after the partition of a chunk of n hits: c.hist[tile][bin] -> rank of the run's first record inside its block of 256 tiles,
// c.hist_part[block][bin] -> the block's first rank, c.bin_base[0..256]
int lzk_hist_scan(LzCtx& c, u64 n)
{
    const u32 ntiles = (u32)((n + LZ_PP_TILE - 1) / LZ_PP_TILE), nblocks = (ntiles + 255u) / 256u;
    u32* hist = c.hist.as<u32>(); u32* part = c.hist_part.as<u32>();
    c.timer.begin("k_hist_scan", c.stream);
    if (nblocks) hipLaunchKernelGGL(k_hist_scan1, dim3(nblocks), dim3(LZ_NBIN), 0, c.stream, hist, ntiles, part);
    hipLaunchKernelGGL(k_hist_scan2, dim3(1), dim3(LZ_NBIN), 0, c.stream, part, nblocks, c.bin_base.as<u32>());
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------
// The X-drop extension of one hit by a whole wave (lz_coop.hpp): every argument is wave-uniform, all 64 lanes
// take part -- lanes 0..31 run the left scan (loop 1), lanes 32..63 the right scan (loop 2), 16 bases per lane and
// step.  tab = the 32 x 32 class table in LDS.  Every lane returns its own side's result.
__device__ __forceinline__ LzCoopMap lz_coop_shfl_up32(const LzCoopMap& v, int d)
{ LzCoopMap r; r.A = __shfl_up(v.A, d, 32); r.B = __shfl_up(v.B, d, 32); r.C = __shfl_up(v.C, d, 32); return r; }
__device__ LzCoopSide lz_coop_extend_wave(const LzExtendParams& P, const s32* tab, u32 pos1, s32 diag, s32 stopl, s32 stopr, u32 lane)
{
    const s32 X = P.xdrop;
    const bool right = lane >= 32u;
    const u32 hl = lane & 31u;
    const s32 stop = right ? stopr : stopl;
    LzCoopSide out; out.stop_pos = pos1; out.best_pos = pos1; out.best = 0;
    s32 run0 = 0, best0 = 0; u32 s = pos1;
    bool alive = (right ? ((s32)s < stop) : ((s32)s > stop)) && X >= 0;        // uniform inside a half
    while (__ballot(alive)) {
        const u32 room = alive ? (right ? (u32)(stop - (s32)s) : (u32)((s32)s - stop)) : 0u;
        const u32 off = LZ_COOP_BLK * hl;
        const u32 nb = room > off ? (room - off < (u32)LZ_COOP_BLK ? room - off : (u32)LZ_COOP_BLK) : 0u;
        s32 sc[LZ_COOP_BLK];
        {
            LzVec16 tv = { { 0, 0, 0, 0 } }, qv = { { 0, 0, 0, 0 } };
            if (nb) {
                const s64 t0 = right ? (s64)s + off : (s64)s - off - LZ_COOP_BLK;
                tv = lz_load16(P.tcode + t0); qv = lz_load16(P.qcode + (t0 - diag));
            }
#pragma unroll
            for (int j = 0; j < LZ_COOP_BLK; j++) {
                const u32 tb = right ? LZ_VBYTE(tv, j) : LZ_VBYTE(tv, LZ_COOP_BLK - 1 - j);      // consumption order
                const u32 qb = right ? LZ_VBYTE(qv, j) : LZ_VBYTE(qv, LZ_COOP_BLK - 1 - j);
                sc[j] = tab[(LZ_CODE_CLASS(tb) << 5) | LZ_CODE_CLASS(qb)];
            }
        }
        LzCoopMap f; s32 mx; u32 jmx;
        lz_coop_block(sc, nb, X, f, mx, jmx);
        // inclusive scan of the maps in lane order inside the half (lower lanes act first), then shifted by one lane
        LzCoopMap inc = f;
#pragma unroll
        for (int d = 1; d < 32; d <<= 1) { const LzCoopMap g = lz_coop_shfl_up32(inc, d); if ((int)hl >= d) inc = lz_coop_compose(g, inc); }
        LzCoopMap ex = lz_coop_shfl_up32(inc, 1);
        if (hl == 0) ex = lz_coop_identity(X);
        const s32 m0 = run0 - best0 + X;
        const bool dead_before = lz_coop_fails(ex, m0);
        const s32 mi = lz_coop_apply(ex, m0), ri = run0 + ex.C;
        const bool fails_here = nb && !dead_before && lz_coop_fails(f, mi);
        const u64 fboth = __ballot(fails_here);                 // at most one lane per half: the blocks after it are "dead before"
        const u32 fmask = right ? (u32)(fboth >> 32) : (u32)fboth;
        // best prefix: (value, first position) as one key, larger is better
        long long key = -1;
        u32 used_here = 0;
        if (fails_here) {
            u32 used; bool stopped; s32 rmx; u32 rj;
            lz_coop_resolve(sc, nb, X, mi, ri, used, stopped, rmx, rj);
            used_here = used;
            if (rj) key = (((long long)rmx + LZ_COOP_INF) << 16) | (long long)(0xFFFFu - (off + rj));
        } else if (nb && jmx && !dead_before)
            key = (((long long)ri + mx + LZ_COOP_INF) << 16) | (long long)(0xFFFFu - (off + jmx));
#pragma unroll
        for (int d = 16; d > 0; d >>= 1) { const long long o = __shfl_xor(key, d, 32); if (o > key) key = o; }
        const int fl = fmask ? (int)__ffs((int)fmask) - 1 : 0;
        const u32 used_f = (u32)__shfl((int)used_here, fl, 32);
        const s32 totc = __shfl(inc.C, 31, 32);
        if (alive) {
            u32 used_total;
            if (fmask) { used_total = LZ_COOP_BLK * (u32)fl + used_f; alive = false; }
            else {
                used_total = room < (u32)(LZ_COOP_BLK * LZ_COOP_LANES) ? room : (u32)(LZ_COOP_BLK * LZ_COOP_LANES);
                if (room <= (u32)(LZ_COOP_BLK * LZ_COOP_LANES)) alive = false;
            }
            if (key >= 0) {
                const s32 v = (s32)((key >> 16) - LZ_COOP_INF); const u32 idx = 0xFFFFu - (u32)(key & 0xFFFF);
                if (v > best0) { best0 = v; out.best_pos = right ? s + idx : s - idx; }
            }
            run0 += totc;
            s = right ? s + used_total : s - used_total;
        }
    }
    out.stop_pos = s; out.best = best0;
    return out;
}

// ------------------------------------------------------------------------------------------
// -DLZ_PHASE_CLOCKS: shader-clock totals of k_settle2's phases (one lane per role adds its cycle-counter
// deltas to a device array the host prints at shutdown); off in the product build
#if defined(LZ_PHASE_CLOCKS)
__device__ unsigned long long g_phase_clk[6];
void lz_phase_clocks_print()
{
    unsigned long long h[6];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_phase_clk), sizeof(h)) != hipSuccess) return;
    fprintf(stderr, "[lzgpu phase clocks] settle (walker work, walker barrier wait, sorter work, sorter barrier wait, extensions of wave 0: cycles, count; cycles summed over the 256 partitions):");
    for (int k = 0; k < 6; k++) fprintf(stderr, " %llu", h[k]);
    fprintf(stderr, "\n");
}
// k_settle2: a walking wave's (slots 0, 1) and a sorting wave's (2, 3) cycles of work / of waiting at the tile barrier
#define LZ_S2_CLK_BEGIN(who) unsigned long long _s2a = (who) ? __builtin_readcyclecounter() : 0ull, _s2b = 0ull
#define LZ_S2_CLK_MID(who, slot) do { if (who) { _s2b = __builtin_readcyclecounter(); atomicAdd(&g_phase_clk[slot], _s2b - _s2a); } } while (0)
#define LZ_S2_CLK_END(who, slot) do { if (who) atomicAdd(&g_phase_clk[slot], __builtin_readcyclecounter() - _s2b); } while (0)
// ... of the walker's work: cycles in the wave-cooperative extensions of SLOW records (slot 4) and how many (5)
#define LZ_S2_CLK_EXT_BEGIN(who, m) const unsigned long long _s2x = (who) ? __builtin_readcyclecounter() : 0ull; const unsigned _s2n = (unsigned)__popcll(m)
#define LZ_S2_CLK_EXT_END(who) do { if (who) { atomicAdd(&g_phase_clk[4], __builtin_readcyclecounter() - _s2x); atomicAdd(&g_phase_clk[5], (unsigned long long)_s2n); } } while (0)
#else
#define LZ_S2_CLK_BEGIN(who)
#define LZ_S2_CLK_MID(who, slot)
#define LZ_S2_CLK_END(who, slot)
#define LZ_S2_CLK_EXT_BEGIN(who, m)
#define LZ_S2_CLK_EXT_END(who)
void lz_phase_clocks_print() {}
#endif

// ------------------------------------------------------------------------------------------
// B2 phase B: one workgroup of 1024 lanes per partition (256 buckets), diagEnd of its buckets in registers.  The
// partition's records arrive in discovery order; tiles of them are dealt out to the buckets inside LDS (counting
// sort by the record's low hash bits, a bucket's list contiguous and in order) and every bucket's list is walked
// by one lane (the fast path of lz_settle_record): the serial part of the whole search is this short walk.  A
// record that needs a real extension (an HSP candidate that passed the diagEnd test) is extended by the lane's
// whole wave (lz_coop_extend_wave), one such record at a time.  The 16 waves have two roles and meet at ONE
// barrier per tile (round 2's kernel did count / offsets / place / walk one after the other behind five barriers,
// 16 walking lanes in every wave):
//   waves 0..3   walkers: lane l of wave w walks bucket 64 w + l of the tile that was placed during the previous
//                interval -- all 64 lanes of a walking wave are busy;
//   waves 4..15  sorters: while tile t is walked they place tile t+1 (offsets from the counts taken one interval
//                earlier, each wave computing the 256 bucket bases for itself from the per-wave counts: no barrier
//                between scan and placement) and count tile t+2 (ranks inside (wave, bucket)).
// Ranks are deterministic: the lanes of a round that hold the same bucket find each other through a 64-bit
// bitmap in LDS (atomic OR of 1 << lane, then a read: the set of peers is independent of the order in which the
// hardware applies the ORs), rank = peers in lower lanes, and the highest peer adds the group to the wave's
// running count.  (Round 2 took the rank from the return value of a same-address LDS atomic add and repaired
// disorder after the fact, which leans on an order the ISA does not promise; here no order is assumed anywhere.)
#define LZ_S2_TPB     1024
#define LZ_ST_BATCH   4                                  // records a walking lane settles per straight-line step
#define LZ_S2_WALKW   4                                  // walking waves: 256 / LZ_S2_WALKW buckets each
#define LZ_S2_SORTW   (LZ_S2_TPB / 64 - LZ_S2_WALKW)     // 12 sorting waves
#define LZ_S2_ROUNDS  7                                  // records per sorter lane and tile (3: 26.7, 4: 24.6, 6: 22.8 ms per step; 6 -> 7 with one chunk per strand: 20.8 -> 20.1; 8 does not fit the LDS)
#define LZ_S2_TILE    (LZ_S2_SORTW * 64 * LZ_S2_ROUNDS)  // 5376
struct LzSettle2Shared {
    s32 tab[LZ_NCLASS * LZ_NCLASS];
    u64 rec[2][LZ_S2_TILE + LZ_ST_BATCH];                // the placed tiles (bucket-major), two take turns
    u64 bm[LZ_S2_SORTW][LZ_NBIN];                        // peer bitmaps of the round in flight (zero between rounds)
    u32 cnt[2][LZ_S2_SORTW][LZ_NBIN];                    // records per (wave, bucket) of the tile being counted / placed
    u32 woff[LZ_S2_SORTW][LZ_NBIN];                      // where wave w's records of bucket b start in the placed tile
    u32 lbeg[2][LZ_NBIN], lcnt[2][LZ_NBIN];              // bucket lists of the placed tiles
};
static_assert(sizeof(LzSettle2Shared) <= 160 * 1024, "k_settle2: one workgroup per CU");
__global__ void __launch_bounds__(LZ_S2_TPB)
k_settle2(LzExtendParams P, const u64* __restrict__ recs, u32 n_pp_tiles, const u32* __restrict__ hist, const u32* __restrict__ hist_part,
          const u32* __restrict__ run_addr, const u32* __restrict__ bin_base, u32* __restrict__ diag_end,
          const s32* __restrict__ score_tab_g, LzHspRec* __restrict__ out, u32* __restrict__ out_count, u32 out_cap,
          u64* __restrict__ counters)
{
    extern __shared__ __align__(16) unsigned char lz_s2_smem[];
    LzSettle2Shared& sh = *reinterpret_cast<LzSettle2Shared*>(lz_s2_smem);
    const u32 tid = threadIdx.x, lane = tid & 63u;
    const u32 w = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));   // wave-uniform, and the compiler knows it
    const u32 part = blockIdx.x;
    const u32 r0 = bin_base[part], r1 = bin_base[part + 1];
    const u32 n = r1 - r0, ntiles = (n + LZ_S2_TILE - 1) / LZ_S2_TILE;
    if (ntiles == 0) return;                                    // (uniform: nothing of this partition in the chunk)
    for (u32 k = tid; k < LZ_NCLASS * LZ_NCLASS; k += LZ_S2_TPB) sh.tab[k] = score_tab_g[k];
    // the sorter waves: tile-run gather, count and placement of tiles into sh.rec / sh.lbeg / sh.lcnt, up to the barriers at
    // which the walkers take over tile 0 (text shared with k_settle_exact; the sorters return inside it)
#include "lz_settle_sorters.inc"
    constexpr u32 BPW = LZ_NBIN / LZ_S2_WALKW;                   // buckets (= walking lanes) per walking wave
    const bool wl = lane < BPW;
    const u32 bucket = (w * BPW + lane) & (LZ_NBIN - 1);        // the lane's bucket
    const u32 h = part * LZ_NBIN + bucket;
    const u32 L = P.seed_len;
    u32 dend = wl ? diag_end[h] : 0u;
    u64 n_ext = 0, n_bp = 0;
    for (u32 t = 0; t < ntiles; t++) {
        LZ_S2_CLK_BEGIN(tid == 0);
        {
            const u64* const rec = sh.rec[t & 1u];
            u32 p = wl ? sh.lbeg[t & 1u][bucket] : 0u; const u32 end = wl ? p + sh.lcnt[t & 1u][bucket] : 0u;
            u32 ne = 0, nb = 0;
            for (;;) {
                // every lane settles records from their phase-A summaries, LZ_ST_BATCH at a time, until one needs a
                // real extension
                bool pending = false; u32 pp2 = 0, ppay = 0;
                while (__ballot(p < end && !pending)) {         // straight-line batches: a lane that has stopped idles through selects
                    u64 r[LZ_ST_BATCH];
#pragma unroll
                    for (int k = 0; k < LZ_ST_BATCH; k++) r[k] = rec[p + k];            // (reads past `end` stay inside rec[] and are not used)
                    bool live = !pending;
                    u32 np = 0;
#pragma unroll
                    for (int k = 0; k < LZ_ST_BATCH; k++) {
                        const u32 p2 = LZ_REC_POS2(r[k]), pay = LZ_REC_PAYLOAD(r[k]);
                        const bool in = live && (p + (u32)k < end);
                        const bool drop = dend > p2 - L;                           // :1113
                        const bool slow = LZ_REC_SLOW(r[k]) != 0 && !drop;
                        const bool go = in && !slow;                               // the record is consumed here
                        const bool fast = go && !drop;
                        const u32 room = p2 - dend, dlo = pay & 0xFFu, dext = pay >> 8;
                        const u32 extent = p2 + dext;                              // :2785
                        ne += fast ? 1u : 0u;
                        nb += fast ? (dlo < room ? dlo : room) + dext : 0u;        // :2818
                        dend = (fast && extent > dend) ? extent : dend;
                        np += go ? 1u : 0u;
                        if (in && slow) { pending = true; pp2 = p2; ppay = pay; }
                        live = go;
                    }
                    p += np;
                }
                u64 mask = __ballot(pending);
                if (!mask) break;
                LZ_S2_CLK_EXT_BEGIN(tid == 0, mask);
                while (mask) {                                  // the wave extends the pending hits, one at a time
                    const int src = (int)__ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const u32 sp2 = (u32)__shfl((int)pp2, src), spay = (u32)__shfl((int)ppay, src), sdend = (u32)__shfl((int)dend, src);
                    const u32 sh_ = part * LZ_NBIN + w * BPW + (u32)src;
                    const s32 diag = (s32)((spay << 16) | sh_);
                    const u32 pos1 = sp2 + (u32)diag;
                    s32 stopl = (s32)sdend + diag;  if (stopl < 0) stopl = 0;                                     // :2612-2616
                    const s32 stopr = ((s32)P.tlen <= (s32)P.qlen + diag) ? (s32)P.tlen : (s32)P.qlen + diag;     // :2675-2677
                    const LzCoopSide S = lz_coop_extend_wave(P, sh.tab, pos1, diag, stopl, stopr, lane);
                    const u32 l_stop = (u32)__shfl((int)S.stop_pos, 0), l_bpos = (u32)__shfl((int)S.best_pos, 0); const s32 l_best = __shfl(S.best, 0);
                    const u32 r_stop = (u32)__shfl((int)S.stop_pos, 32), r_bpos = (u32)__shfl((int)S.best_pos, 32); const s32 r_best = __shfl(S.best, 32);
                    if ((int)lane == src) {
                        ne++; nb += r_stop - l_stop;                                             // :2818
                        const u32 extent = (u32)((s32)r_stop - diag);                            // :2785
                        if (extent > dend) dend = extent;
                        const s32 sim = l_best + r_best;
                        if (sim >= P.min_score) {
                            const u32 oslot = atomicAdd(out_count, 1u);
                            if (oslot < out_cap) { LzHspRec o; o.seed_pos1 = pos1; o.seed_pos2 = sp2; o.end1 = r_bpos; o.length = r_bpos - l_bpos; o.score = sim; out[oslot] = o; }
                        }
                        p++;
                    }
                }
                LZ_S2_CLK_EXT_END(tid == 0);
            }
            n_ext += ne; n_bp += nb;
        }
        LZ_S2_CLK_MID(tid == 0, 0);
        __syncthreads();
        LZ_S2_CLK_END(tid == 0, 1);
    }
    if (wl) diag_end[h] = dend;
    for (int o = 32; o > 0; o >>= 1) { n_ext += __shfl_down(n_ext, o); n_bp += __shfl_down(n_bp, o); }
    if (lane == 0) {
        if (n_ext) atomicAdd((unsigned long long*)&counters[0], (unsigned long long)n_ext);
        if (n_bp)  atomicAdd((unsigned long long*)&counters[1], (unsigned long long)n_bp);
    }
}

// phase B of the chunk's n records in c.keys (runs: c.hist, c.hist_part, c.run_addr, c.bin_base): c.diag_end carries on from the chunk
// before; candidates -> c.hsp_out (room for out_cap) / c.hsp_count, extensions and bases -> c.dev_counters[0], [1]
int lzk_settle(LzCtx& c, const LzExtendParams& P, u64 n, u32 out_cap)
{
    if (n == 0) return 0;
    const u32 n_pp_tiles = (u32)((n + LZ_PP_TILE - 1) / LZ_PP_TILE);
    c.timer.begin("k_settle2", c.stream);
    // (the attribute belongs to the device the context was made on: lzgpu_shutdown clears the flag)
    if (!c.settle_attr_set) { LZ_HIP(hipFuncSetAttribute((const void*)k_settle2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(LzSettle2Shared))); c.settle_attr_set = true; }
    hipLaunchKernelGGL(k_settle2, dim3(LZ_NBIN), dim3(LZ_S2_TPB), sizeof(LzSettle2Shared), c.stream, P, c.keys.as<u64>(), n_pp_tiles,
                       c.hist.as<u32>(), c.hist_part.as<u32>(), c.run_addr.as<u32>(), c.bin_base.as<u32>(),
                       c.diag_end.as<u32>(), c.score_tab.as<s32>(), c.hsp_out.as<LzHspRec>(), c.hsp_count.as<u32>(), out_cap, c.dev_counters.as<u64>());
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------
// Phase B of an exact-match search (lastz --exact, lz_exact.hpp): k_settle2's sorters and one walking lane per bucket with
// diagEnd in a register.  A fast record is the drop test and dend = max(dend, extent); a SLOW record that passes the drop
// test is extended by the lane's whole wave against the real dend, 64 x 32 bases per step and side (a ballot finds the
// first block that ends the run: a run of megabases takes a few hundred steps).  No scores, no class table (sh.tab stays unused).
__global__ void __launch_bounds__(LZ_S2_TPB)
k_settle_exact(LzExactParams P, const u64* __restrict__ recs, u32 n_pp_tiles, const u32* __restrict__ hist, const u32* __restrict__ hist_part,
               const u32* __restrict__ run_addr, const u32* __restrict__ bin_base, u32* __restrict__ diag_end,
               LzHspRec* __restrict__ out, u32* __restrict__ out_count, u32 out_cap)
{
    extern __shared__ __align__(16) unsigned char lz_s2_smem[];
    LzSettle2Shared& sh = *reinterpret_cast<LzSettle2Shared*>(lz_s2_smem);
    const u32 tid = threadIdx.x, lane = tid & 63u;
    const u32 w = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));   // wave-uniform, and the compiler knows it
    const u32 part = blockIdx.x;
    const u32 r0 = bin_base[part], r1 = bin_base[part + 1];
    const u32 n = r1 - r0, ntiles = (n + LZ_S2_TILE - 1) / LZ_S2_TILE;
    if (ntiles == 0) return;                                    // (uniform: nothing of this partition in the chunk)
#include "lz_settle_sorters.inc"
    constexpr u32 BPW = LZ_NBIN / LZ_S2_WALKW;                   // buckets (= walking lanes) per walking wave
    const bool wl = lane < BPW;
    const u32 bucket = (w * BPW + lane) & (LZ_NBIN - 1);        // the lane's bucket
    const u32 h = part * LZ_NBIN + bucket;
    const u32 L = P.seed_len;
    u32 dend = wl ? diag_end[h] : 0u;
    for (u32 t = 0; t < ntiles; t++) {
        const u64* const rec = sh.rec[t & 1u];
        u32 p = wl ? sh.lbeg[t & 1u][bucket] : 0u; const u32 end = wl ? p + sh.lcnt[t & 1u][bucket] : 0u;
        for (;;) {
            // every lane settles records from their phase-A summaries, LZ_ST_BATCH at a time, until one needs an extension
            bool pending = false; u32 pp2 = 0, ppay = 0;
            while (__ballot(p < end && !pending)) {
                u64 r[LZ_ST_BATCH];
#pragma unroll
                for (int k = 0; k < LZ_ST_BATCH; k++) r[k] = rec[p + k];                // (reads past `end` stay inside rec[] and are not used)
                bool live = !pending;
                u32 np = 0;
#pragma unroll
                for (int k = 0; k < LZ_ST_BATCH; k++) {
                    const u32 p2 = LZ_REC_POS2(r[k]), pay = LZ_REC_PAYLOAD(r[k]);
                    const bool in = live && (p + (u32)k < end);
                    const bool drop = lz_exact_drops(dend, p2, L);
                    const bool slow = LZ_REC_SLOW(r[k]) != 0 && !drop;
                    const bool go = in && !slow;                               // the record is consumed here
                    dend = (go && !drop) ? lz_exact_fast_dend(dend, p2, L, pay) : dend;
                    np += go ? 1u : 0u;
                    if (in && slow) { pending = true; pp2 = p2; ppay = pay; }
                    live = go;
                }
                p += np;
            }
            u64 mask = __ballot(pending);
            if (!mask) break;
            while (mask) {                                      // the wave extends the pending hits, one at a time
                const int src = (int)__ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const u32 sp2 = (u32)__shfl((int)pp2, src), spay = (u32)__shfl((int)ppay, src), sdend = (u32)__shfl((int)dend, src);
                const u32 pos1 = sp2 + ((spay << 16) | (part * LZ_NBIN + w * BPW + (u32)src));
                const u32 room = sp2 - L - sdend;
                u32 right = 0, left = 0;
                for (u32 b = lane;; b += 64u) {                 // (b - lane is wave-uniform; a block past the sequences returns 0: the loop ends)
                    const u32 run = lz_exact_block_right(P, pos1, sp2, b);
                    const u64 stop = __ballot(run < LZ_EX_W);
                    if (stop) { const int f = (int)__ffsll((long long)stop) - 1; right = (b - lane + (u32)f) * LZ_EX_W + (u32)__shfl((int)run, f); break; }
                }
                for (u32 b = lane;; b += 64u) {                 // (a block past the room returns 0)
                    const u32 run = lz_exact_block_left(P, pos1, sp2, room, b);
                    const u64 stop = __ballot(run < LZ_EX_W);
                    if (stop) { const int f = (int)__ffsll((long long)stop) - 1; left = (b - lane + (u32)f) * LZ_EX_W + (u32)__shfl((int)run, f); break; }
                }
                if ((int)lane == src) {
                    LzHspRec o;
                    if (lz_exact_finish(P, pos1, sp2, dend, left, right, o)) {
                        const u32 oslot = atomicAdd(out_count, 1u);
                        if (oslot < out_cap) out[oslot] = o;
                    }
                    p++;
                }
            }
        }
        __syncthreads();
    }
    if (wl) diag_end[h] = dend;
}

// phase B of an exact-match search on the chunk's n records in c.keys: as lzk_settle, without counters
int lzk_settle_exact(LzCtx& c, const LzExactParams& P, u64 n, u32 out_cap)
{
    if (n == 0) return 0;
    const u32 n_pp_tiles = (u32)((n + LZ_PP_TILE - 1) / LZ_PP_TILE);
    c.timer.begin("k_settle_exact", c.stream);
    if (!c.settle_exact_attr_set) { LZ_HIP(hipFuncSetAttribute((const void*)k_settle_exact, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(LzSettle2Shared))); c.settle_exact_attr_set = true; }
    hipLaunchKernelGGL(k_settle_exact, dim3(LZ_NBIN), dim3(LZ_S2_TPB), sizeof(LzSettle2Shared), c.stream, P, c.keys.as<u64>(), n_pp_tiles,
                       c.hist.as<u32>(), c.hist_part.as<u32>(), c.run_addr.as<u32>(), c.bin_base.as<u32>(),
                       c.diag_end.as<u32>(), c.hsp_out.as<LzHspRec>(), c.hsp_count.as<u32>(), out_cap);
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------
// Phase B of an N-mismatch search (lastz --mismatch, lz_mismatch.hpp): k_settle_exact's frame -- k_settle2's sorters, one walking
// lane per bucket with diagEnd in a register, a fast record is the drop test and dend = max(dend, extent).  A SLOW record that
// passes the drop test is extended by the lane's whole wave against the real dend: per step and side 64 x 32 bases, a wave
// prefix sum of the mismatch words' popcounts says which lane's bits are the next of the K = M + 1 - E wanted positions, which
// go to the wave's two lists in LDS (sh.tab's place: no class table here); lane j then asks whether position j is a stop,
// evaluates the pairing of right mismatch j, and a wave reduction takes the longest, the earliest among equals.  An identical
// megabase takes a few hundred steps per side.
__device__ __forceinline__ void lz_mm_wave_lds_sync()           // the wave's own LDS stores before its other lanes' loads
{ __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }
// the first K mismatch positions of one side in scan order -> list[0..K) (every argument wave-uniform).  Positions are s32: the
// loop goes at most one step (2048 bases, + one block) past the scan's reach, so they stay in range as long as both sequences are
// shorter than 2^31 - 2080 bases (the library takes sequences below 2^31; an entry beyond a stop is never used in any case: the
// first stop ends its list)
template <bool RIGHT>
__device__ __forceinline__ void lz_mm_wave_collect(const LzMismatchParams& P, const LzMmHit& H, u32 K, u32 lane, volatile s32* list)
{
    u32 have = 0;
    for (u32 b0 = 0; have < K; b0 += 64u) {                     // (a block beyond the scan's reach is 32 mismatches: the loop ends)
        u32 wd = RIGHT ? lz_mm_block_right(P, H, b0 + lane) : lz_mm_block_left(P, H, b0 + lane);
        const u32 cnt = lz_mm_popc(wd);
        u32 inc = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const u32 t = __shfl_up(inc, d); if ((int)lane >= d) inc += t; }
        u32 at = have + inc - cnt;
        const s32 base = RIGHT ? (s32)((s64)H.pos2 + (s64)LZ_EX_W * (s64)(b0 + lane))
                               : (s32)((s64)H.pos2 - (s64)P.X.seed_len - (s64)LZ_EX_W * (s64)(b0 + lane)) - 1;
        for (; wd && at < K; wd &= wd - 1u) { const s32 k = (s32)__builtin_ctz(wd); list[at++] = RIGHT ? base + k : base - k; }
        have += (u32)__shfl((int)inc, 63);
    }
    lz_mm_wave_lds_sync();
}
static_assert(LZ_S2_WALKW * 2 * LZ_MM_LIST <= LZ_NCLASS * LZ_NCLASS && LZ_MM_MAX + 1 <= LZ_MM_LIST, "the walking waves' lists lie in sh.tab");
__global__ void __launch_bounds__(LZ_S2_TPB)
k_settle_mismatch(LzMismatchParams P, const u64* __restrict__ recs, u32 n_pp_tiles, const u32* __restrict__ hist, const u32* __restrict__ hist_part,
                  const u32* __restrict__ run_addr, const u32* __restrict__ bin_base, u32* __restrict__ diag_end,
                  LzHspRec* __restrict__ out, u32* __restrict__ out_count, u32 out_cap)
{
    extern __shared__ __align__(16) unsigned char lz_s2_smem[];
    LzSettle2Shared& sh = *reinterpret_cast<LzSettle2Shared*>(lz_s2_smem);
    const u32 tid = threadIdx.x, lane = tid & 63u;
    const u32 w = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));   // wave-uniform, and the compiler knows it
    const u32 part = blockIdx.x;
    const u32 r0 = bin_base[part], r1 = bin_base[part + 1];
    const u32 n = r1 - r0, ntiles = (n + LZ_S2_TILE - 1) / LZ_S2_TILE;
    if (ntiles == 0) return;                                    // (uniform: nothing of this partition in the chunk)
#include "lz_settle_sorters.inc"
    constexpr u32 BPW = LZ_NBIN / LZ_S2_WALKW;                   // buckets (= walking lanes) per walking wave
    const bool wl = lane < BPW;
    const u32 bucket = (w * BPW + lane) & (LZ_NBIN - 1);        // the lane's bucket
    const u32 h = part * LZ_NBIN + bucket;
    const u32 L = P.X.seed_len;
    volatile s32* const sl = sh.tab + (w & (LZ_S2_WALKW - 1u)) * (2u * LZ_MM_LIST);      // the wave's starts, nearest first
    volatile s32* const rl = sl + LZ_MM_LIST;                                            // ... and its right mismatches
    u32 dend = wl ? diag_end[h] : 0u;
    for (u32 t = 0; t < ntiles; t++) {
        const u64* const rec = sh.rec[t & 1u];
        u32 p = wl ? sh.lbeg[t & 1u][bucket] : 0u; const u32 end = wl ? p + sh.lcnt[t & 1u][bucket] : 0u;
        for (;;) {
            // every lane settles records from their phase-A summaries, LZ_ST_BATCH at a time, until one needs an extension
            bool pending = false; u32 pp2 = 0, ppay = 0;
            while (__ballot(p < end && !pending)) {
                u64 r[LZ_ST_BATCH];
#pragma unroll
                for (int k = 0; k < LZ_ST_BATCH; k++) r[k] = rec[p + k];                // (reads past `end` stay inside rec[] and are not used)
                bool live = !pending;
                u32 np = 0;
#pragma unroll
                for (int k = 0; k < LZ_ST_BATCH; k++) {
                    const u32 p2 = LZ_REC_POS2(r[k]), pay = LZ_REC_PAYLOAD(r[k]);
                    const bool in = live && (p + (u32)k < end);
                    const bool drop = lz_exact_drops(dend, p2, L);
                    const bool slow = LZ_REC_SLOW(r[k]) != 0 && !drop;
                    const bool go = in && !slow;                               // the record is consumed here
                    dend = (go && !drop) ? lz_exact_fast_dend(dend, p2, L, pay) : dend;
                    np += go ? 1u : 0u;
                    if (in && slow) { pending = true; pp2 = p2; ppay = pay; }
                    live = go;
                }
                p += np;
            }
            u64 mask = __ballot(pending);
            if (!mask) break;
            while (mask) {                                      // the wave extends the pending hits, one at a time
                const int src = (int)__ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const u32 sp2 = (u32)__shfl((int)pp2, src), spay = (u32)__shfl((int)ppay, src), sdend = (u32)__shfl((int)dend, src);
                const u32 pos1 = sp2 + ((spay << 16) | (part * LZ_NBIN + w * BPW + (u32)src));
                const LzMmHit H = lz_mm_hit(P, pos1, sp2, sdend);
                const u32 K = P.M + 1u - H.E;                   // (a SLOW record has E <= M)
                // the starts: the first stop among them ends the list
                lz_mm_wave_collect<false>(P, H, K, lane, sl);
                const s32 mine_l = lane < K ? sl[lane] : 0;
                const u64 hard_l = __ballot(lane < K && lz_mm_hard_left(P, H, mine_l));
                const u32 c = hard_l ? (u32)__ffsll((long long)hard_l) : K;
                if (hard_l && lane + 1u == c) sl[lane] = lz_mm_stop_start(H, mine_l);
                // the right mismatches, likewise
                lz_mm_wave_collect<true>(P, H, K, lane, rl);      // (its LDS synchronisation covers the store above)
                const s32 mine_r = lane < K ? rl[lane] : 0;
                const u64 hard_r = __ballot(lane < K && lz_mm_hard_right(P, H, mine_r));
                const u32 nr = hard_r ? (u32)__ffsll((long long)hard_r) : K;
                // lane j: the interval right mismatch j closes
                u64 key = 0;
                if (lane < nr) {
                    const int at = lz_mm_pair_start(lane, hard_r != 0 && lane + 1u == nr, c, K);
                    if (at >= 0) key = lz_mm_pair_key((u32)(mine_r - sl[at]), lane);
                }
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) { const u64 o = (u64)__shfl_xor((unsigned long long)key, d); if (o > key) key = o; }
                const u32 jbest = 255u - (u32)(key & 0xFFu);
                const s32 right = __shfl(mine_r, (int)jbest), first_right = __shfl(mine_r, 0);
                const s32 left = right - (s32)(u32)(key >> 8);
                if ((int)lane == src) {
                    LzHspRec o;
                    if (lz_mm_finish(P, H, dend, left, right, first_right, o)) {
                        const u32 oslot = atomicAdd(out_count, 1u);
                        if (oslot < out_cap) out[oslot] = o;
                    }
                    p++;
                }
                lz_mm_wave_lds_sync();                          // (the lists are free again)
            }
        }
        __syncthreads();
    }
    if (wl) diag_end[h] = dend;
}

// phase B of an N-mismatch search on the chunk's n records in c.keys: as lzk_settle_exact
int lzk_settle_mismatch(LzCtx& c, const LzMismatchParams& P, u64 n, u32 out_cap)
{
    if (n == 0) return 0;
    const u32 n_pp_tiles = (u32)((n + LZ_PP_TILE - 1) / LZ_PP_TILE);
    c.timer.begin("k_settle_mismatch", c.stream);
    if (!c.settle_mismatch_attr_set) { LZ_HIP(hipFuncSetAttribute((const void*)k_settle_mismatch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(LzSettle2Shared))); c.settle_mismatch_attr_set = true; }
    hipLaunchKernelGGL(k_settle_mismatch, dim3(LZ_NBIN), dim3(LZ_S2_TPB), sizeof(LzSettle2Shared), c.stream, P, c.keys.as<u64>(), n_pp_tiles,
                       c.hist.as<u32>(), c.hist_part.as<u32>(), c.run_addr.as<u32>(), c.bin_base.as<u32>(),
                       c.diag_end.as<u32>(), c.hsp_out.as<LzHspRec>(), c.hsp_count.as<u32>(), out_cap);
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------
// entropy inputs of the candidate HSPs: per candidate, how many aligned positions carry the
// same byte 'A' / 'C' / 'G' / 'T' in target and query (compute_entropy counts exactly these,
// src/dna_utilities.c:2899-2912).  One wave per candidate, lanes stride over the segment.
__global__ void __launch_bounds__(LZ_TPB)
k_hsp_match_counts(const LzHspRec* __restrict__ recs, const u32* __restrict__ n_rec, u32 cap,
                   const u8* __restrict__ traw, const u8* __restrict__ qraw,
                   const u8* __restrict__ tcode, const u8* __restrict__ qcode, LzSeedDev sd, u32* __restrict__ counts)
{
    const u32 wave = (blockIdx.x * LZ_TPB + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    u32 n = *n_rec; if (n > cap) n = cap;
    if (wave >= n) return;
    const LzHspRec r = recs[wave];
    const s32 diag = (s32)r.seed_pos1 - (s32)r.seed_pos2;
    const u32 s1 = r.end1 - r.length, s2 = (u32)((s32)s1 - diag);
    u32 cA = 0, cC = 0, cG = 0, cT = 0;
    for (u32 k = lane; k < r.length; k += 64) {
        const u32 a = traw[s1 + k], b = qraw[s2 + k];
        if (a == b) { cA += (a == 'A'); cC += (a == 'C'); cG += (a == 'G'); cT += (a == 'T'); }
    }
    for (int o = 32; o > 0; o >>= 1) { cA += __shfl_down(cA, o); cC += __shfl_down(cC, o); cG += __shfl_down(cG, o); cT += __shfl_down(cT, o); }
    if (lane == 0) {
        // which probe produced the seed hit (its discovery rank inside a query position): the XOR of the
        // two packed words is one of the probe masks (src/seed_search.c:522-549)
        u32 pt = 0, pq = 0, probe = 0xFFFFFFFFu;
        if (lz_window_word(tcode, r.seed_pos1, sd, pt) && lz_window_word(qcode, r.seed_pos2, sd, pq)) {
            const u32 x = pt ^ pq;
            for (int p = 0; p < sd.nprobes; p++) if (sd.probe_xor[p] == x) { probe = (u32)p; break; }
        }
        u32* o = counts + 5 * (size_t)wave;
        o[0] = cA; o[1] = cC; o[2] = cG; o[3] = cT; o[4] = probe;
    }
}

// c.hsp_mc (sized by the caller) for the first n_rec candidates of c.hsp_out, found against the query in slot q
int lzk_hsp_match_counts(LzCtx& c, u32 n_rec, const SeqSlot& q)
{
    if (n_rec == 0) return 0;
    const u64 threads = (u64)n_rec * 64;
    c.timer.begin("k_hsp_match_counts", c.stream);
    hipLaunchKernelGGL(k_hsp_match_counts, dim3((unsigned)((threads + LZ_TPB - 1) / LZ_TPB)), dim3(LZ_TPB), 0, c.stream,
                       c.hsp_out.as<LzHspRec>(), c.hsp_count.as<u32>(), n_rec,
                       c.target.raw_base(), q.raw_base(), c.target.code_base(), q.code_base(), c.seed, c.hsp_mc.as<u32>());
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    return 0;
}
