// scan_kernels.hip -- gfx950 kernels of phase A (DESIGN.md section 3, rows 4 and 5, and rows 2 + 4 and 5 of the fused form):
// every hit's two gap-free scans, independent of the diagonal hash, in three scan modes; the scans that go on as tasks; and
// the fused kernel that enumerates and scans in one launch (steps 1 and 2 of its list enumeration: the fragments lz_enum_place.inc with
// lz_enum_lists.inc, and lz_enum_owners.inc, text shared with k_fill_hits2 of enum_kernels.hip).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <type_traits>
#include "lz_ctx.hpp"
#include "lz_host.hpp"
#include "lz_lut.hpp"
#include "lz_seed_dev.hpp"

// ------------------------------------------------------------------------------------------
// B2 step 3: the hits of a chunk, which k_fill_hits (enum_kernels.hip) wrote in discovery order, are (a) scanned independently of
// the diagonal hash (phase A) and (b) stably partitioned by the high 8 bits of hashedDiag into 256 streams of
// 8-byte records (lz_lut.hpp), one stream per workgroup of phase B.  One pass that scans (k_scan_hits,
// k_scan_tasks) and one that sorts every tile of 16384 hits by partition where it lies (k_partition: 8 B + 4 B read
// and 8 B written per hit in whole tiles, where a radix sort of (key, summary) pairs moved 56); two small scans over
// the tiles' counts (k_hist_scan) give every run its rank, and phase B gathers a partition's runs (lz_tile_runs.hpp).
// (a) is this file; (b) and phase B are settle_kernels.hip.
#define LZ_SC_ROUNDS 4                               // k_scan_hits: rounds of 64 hits a wave takes per span

// ---- phase A + the partition, three kernels:
//   k_scan_hits   every hit's two scans, first window each (the heavy, branch-free code of lz_lut.hpp): a pure
//                 stream -- a wave takes 256 consecutive hits, 64 at a time, with the next 64 hits' windows in
//                 flight -- with no barrier and nothing in LDS but the 32 KiB table, so every resident wave is in
//                 this code all the time.  Output: the 4-byte summary of a hit whose scans both ended; the rare hit
//                 with a scan that goes on (~3 %) becomes a 64-byte task in a global list (one atomic per wave).
//   k_scan_tasks  one lane per task: the scans that go on, to their end or the LZ_LUT_MAXWIN cap; full waves.  <MODE, false>
//                 here; <0, true> behind the fused kernel.
//   k_partition   (settle_kernels.hip) <false>: keys + summaries -> records, every tile stably sorted by partition in place (+ the tile
//                 tables); <true>: the same on the fused kernel's tagged records.
// (One fused kernel did all of this per tile behind barriers: its workgroups spent half their time in the light
// phases -- queue drain on two waves, ranks, write-out -- while holding the LDS and the wave slots the scans need.)
struct LzScanTask { u32 idx; s32 diag; LzLutScan L, R; };
static_assert(sizeof(LzScanTask) == 64, "LzScanTask: one 64-byte line per task");
#define LZ_SC_TPB 512                                // k_scan_hits<1/2>, k_scan_tasks regions; k_scan_hits<0> picks its own size (TPB template parameter)
template <int MODE> struct LzScanShared {
    union {
        LzLutEntry lut[LZ_LUT_TOTAL];                                   // MODE 0/1: the two look-up tables (64 KiB)
        struct { s32 tab[LZ_NCLASS * LZ_NCLASS]; s32 tab8[64]; } bc;    // MODE 2: the byte-code scans' tables
    };
    s32 ctab[MODE == 1 ? LZ_NCLASS * LZ_NCLASS : 1];                    // MODE 1: the class table (a special base is scored from it)
};

// one round of k_scan_hits<0/1>: both scans' first windows of the hit `key`, whose windows (rawl, rawr) are loaded.
// MODE 0 heads run without limit tests: a side with less than 60 bases of room is left to k_scan_tasks.
template <bool SP>
__device__ __forceinline__ void lz_scan_round(const LzExtendParams& P, const LzLutParams& Q, const LzLutEntry* lut, const s32* ctab, u64 key, bool valid,
                                              const LzLutRaw<SP>& rawl, const LzLutRaw<SP>& rawr, u32 idx, u32 lane,
                                              u32& summ_out, LzScanTask* __restrict__ my_tasks, u32& my_n, u32 region_cap)
{
    constexpr bool HLIM = SP;
    s32 diag; LzLutScan L, R;
    lz_lut_init(key, P.tlen, P.qlen, diag, L, R);
    if (!valid) { L.alive = 0; R.alive = 0; }
    const bool ql = L.alive && !HLIM && L.room < (u32)LZ_LUT_WIN_B, qr = R.alive && !HLIM && R.room < (u32)LZ_LUT_WIN_B;
    lz_lut_window_pair<SP, HLIM>(Q, lut, diag, L, R, rawl, rawr, L.alive && !ql, R.alive && !qr, ctab);
    const bool more = valid && (L.alive == 1 || R.alive == 1);
    const u64 mm = __ballot(more);
    bool queued = false;
    if (mm) {                                                    // (wave-uniform)
        const u32 slot = my_n + (u32)__popcll(mm & ((1ull << lane) - 1ull));
        if (more && slot < region_cap) {                         // (a full region leaves the scan "alive": the hit becomes SLOW)
            LzScanTask t; t.idx = idx; t.diag = diag; t.L = L; t.R = R;
            my_tasks[slot] = t; queued = true;
        }
        my_n += (u32)__popcll(mm);
    }
    summ_out = queued ? 0u : lz_lut_summary(L, R, P.min_score);          // (a queued hit's summary comes from k_scan_tasks, behind this kernel)
}
// The windows of a hit: 2 x 16 bytes of the target's 2-bit codes from the half-overlapping blocks (the left window starts at byte bl,
// the right one at br = bl + 15 or 16, together at most 32 bytes: ONE line of t2x -- block bl / 32, offset bl % 32), 2 x 16 bytes of
// the query's from the plain array (the hits of a wave are in discovery order: runs of lanes ask for the same query line), and with
// special bytes about (SP) the same of the two 1-bit masks.  (Variants that were measured and lost -- query windows shared through the
// LDS crossbar, the plain target array, timing-only what-ifs without the target / with an L2-resident target -- are patches under
// tools/experiments/, applied by tools/build_variant.sh.)
template <bool SP>
__device__ __forceinline__ void lz_scan_fetch(const LzLutParams& Q, u64 key, LzLutRaw<SP>& rawl, LzLutRaw<SP>& rawr)
{
    const u32 pos2 = (u32)key, pos1 = pos2 + (u32)(key >> 32);
    const s32 diag = (s32)(u32)(key >> 32);
    const u32 stl = pos1 - 1u + (u32)LZ_PAD2, str = pos1 + (u32)LZ_PAD2;
    const u32 bl = (stl >> 2) - 15u, br = str >> 2;
    const u32 ol = bl + (bl & ~31u);
    rawl.tv = lz_load16(Q.t2x + ol); rawr.tv = lz_load16(Q.t2x + (ol + (br - bl)));
    const u32 sql = stl - (u32)diag, sqr = str - (u32)diag;
    rawl.qv = lz_load16(Q.q2 + ((sql >> 2) - 15u)); rawr.qv = lz_load16(Q.q2 + (sqr >> 2));
    if constexpr (SP) {
        const u32 ml = (stl >> 3) - 14u, mr = str >> 3;           // (mr - ml is 14 or 15: at most 31 bytes)
        const u32 oml = ml + (ml & ~31u);
        rawl.tm = lz_load16(Q.tspx + oml); rawr.tm = lz_load16(Q.tspx + (oml + (mr - ml)));
        rawl.qm = lz_load16(Q.qsp + ((sql >> 3) - 14u)); rawr.qm = lz_load16(Q.qsp + (sqr >> 3));
    }
}

// TPB lanes per workgroup, WPE waves per SIMD the register allocation must allow (two workgroups share a CU's LDS)
template <int MODE, int TPB, int WPE>      // MODE 0: LUT scans, no special bytes in either sequence; 1: LUT scans + special masks; 2: byte-code scans
__global__ void __launch_bounds__(TPB, WPE)
k_scan_hits(LzExtendParams P, LzLutParams Q, const u64* __restrict__ keys, u64 n,
            const s32* __restrict__ score_tab_g, const LzLutEntry* __restrict__ lut_g,
            u32* __restrict__ summ, u8* __restrict__ bins, LzScanTask* __restrict__ tasks, u32* __restrict__ n_tasks, u32 region_cap)
{
    __shared__ LzScanShared<MODE> sh;
    const u32 tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    if (MODE == 1) { for (u32 k = tid; k < LZ_NCLASS * LZ_NCLASS; k += TPB) sh.ctab[k] = score_tab_g[k]; }
    if (MODE < 2) { for (u32 k = tid; k < LZ_LUT_TOTAL; k += TPB) sh.lut[k] = lut_g[k]; }
    else {
        for (u32 k = tid; k < LZ_NCLASS * LZ_NCLASS; k += TPB) sh.bc.tab[k] = score_tab_g[k];
        if (tid < 64) sh.bc.tab8[tid] = score_tab_g[(tid >> 3) * LZ_NCLASS + (tid & 7)];
    }
    __syncthreads();
    const LzLutEntry* lut = sh.lut;
    const s32* const ctab = sh.ctab;
    constexpr bool SP = MODE == 1;
    constexpr u32 SPAN = 64u * LZ_SC_ROUNDS;
    static_assert(LZ_SC_ROUNDS == 4, "the round pipeline below is written out for four rounds per span");
    const u64 nspans = (n + SPAN - 1) / SPAN, wstride = (u64)gridDim.x * (TPB / 64);
    // the tasks of a wave go to the wave's own region of the list: no atomics, the count is written once at the end
    const u32 region = blockIdx.x * (TPB / 64) + w;
    LzScanTask* const my_tasks = tasks + (size_t)region * region_cap;
    u32 my_n = 0;
    u64 span = (u64)blockIdx.x * (TPB / 64) + w;
    if (MODE == 2) {
        for (; span < nspans; span += wstride) {
            const u64 base = span * SPAN;
            const u32 span_n = (n - base < (u64)SPAN) ? (u32)(n - base) : SPAN;
#pragma unroll 1
            for (u32 r = 0; r < LZ_SC_ROUNDS; r++) {
                const u32 li = r * 64u + lane;
                if (li < span_n) { const u64 kk = keys[base + li]; summ[base + li] = lz_probe_hit(P, sh.bc.tab, sh.bc.tab8, P.cls8 != 0, kk); bins[base + li] = (u8)LZ_KEY_BIN(kk); }
            }
        }
    } else if (span < nspans) {
        // A wave takes 256 consecutive hits (a span); a LANE takes four consecutive ones, one per round: its keys are two 16-byte loads,
        // its four summaries one 16-byte store, its four partition bytes one 4-byte store -- 64 consecutive bytes of a
        // span's 256 went out per round when a lane's hits were 64 apart (the partition bytes as 64 one-byte stores: +2 ms on the 50 Mbp
        // pair; the fill kernel used to write them beside its keys, in runs of ~39 bytes at random places, two partial lines each: 4-7 of
        // its 19-26 ms).  The windows of a round are requested one round ahead into two register sets that take turns (no copies), the
        // next span's keys two rounds ahead and its first windows during the span's last round: every load has a round of arithmetic to
        // hide behind.
        typedef u64 lz_u64x2 __attribute__((ext_vector_type(2)));
        auto load_keys = [&](u64 sp, u64& a0, u64& a1, u64& a2, u64& a3) {
            const u64 base = sp * SPAN;
            const u32 sn = (n - base < (u64)SPAN) ? (u32)(n - base) : SPAN;
            const u32 l4 = 4u * lane;
            const u64* kp = keys + base + l4;
            if (l4 + 3u < sn) {
                const lz_u64x2 x = LZ_NT_LD(reinterpret_cast<const lz_u64x2*>(kp)), y = LZ_NT_LD(reinterpret_cast<const lz_u64x2*>(kp + 2));
                a0 = x.x; a1 = x.y; a2 = y.x; a3 = y.y;
            } else {
                a0 = (l4 < sn) ? LZ_NT_LD(kp) : 0ull;           a1 = (l4 + 1u < sn) ? LZ_NT_LD(kp + 1) : 0ull;
                a2 = (l4 + 2u < sn) ? LZ_NT_LD(kp + 2) : 0ull;  a3 = 0ull;
            }
        };
        u64 k0, k1, k2, k3;
        load_keys(span, k0, k1, k2, k3);
        LzLutRaw<SP> al, ar, bl, br;
        lz_scan_fetch<SP>(Q, k0, al, ar);
#pragma unroll 1
        for (;;) {
            const u64 base = span * SPAN;
            const u32 span_n = (n - base < (u64)SPAN) ? (u32)(n - base) : SPAN;
            const u32 l4 = 4u * lane;
            const u32 ib = (u32)base + l4;                       // (hit indices inside a chunk are 32-bit: lzgpu_set_hit_capacity)
            const bool more_spans = span + wstride < nspans;
            u64 n0 = 0, n1 = 0, n2 = 0, n3 = 0;
            u32 s0, s1, s2, s3;
            lz_scan_fetch<SP>(Q, k1, bl, br);
            lz_scan_round<SP>(P, Q, lut, ctab, k0, l4 < span_n, al, ar, ib, lane, s0, my_tasks, my_n, region_cap);
            if (more_spans) load_keys(span + wstride, n0, n1, n2, n3);
            lz_scan_fetch<SP>(Q, k2, al, ar);
            lz_scan_round<SP>(P, Q, lut, ctab, k1, l4 + 1u < span_n, bl, br, ib + 1u, lane, s1, my_tasks, my_n, region_cap);
            lz_scan_fetch<SP>(Q, k3, bl, br);
            lz_scan_round<SP>(P, Q, lut, ctab, k2, l4 + 2u < span_n, al, ar, ib + 2u, lane, s2, my_tasks, my_n, region_cap);
            if (more_spans) lz_scan_fetch<SP>(Q, n0, al, ar);
            lz_scan_round<SP>(P, Q, lut, ctab, k3, l4 + 3u < span_n, bl, br, ib + 3u, lane, s3, my_tasks, my_n, region_cap);
            const u32 pbytes = LZ_KEY_BIN(k0) | (LZ_KEY_BIN(k1) << 8) | (LZ_KEY_BIN(k2) << 16) | (LZ_KEY_BIN(k3) << 24);       // (the keys are still in their registers)
            if (l4 + 3u < span_n) {
                typedef u32 lz_u32x4 __attribute__((ext_vector_type(4)));
                lz_u32x4 sv4; sv4.x = s0; sv4.y = s1; sv4.z = s2; sv4.w = s3;
                LZ_NT_ST(sv4, reinterpret_cast<lz_u32x4*>(summ + ib));
                LZ_NT_ST(pbytes, reinterpret_cast<u32*>(bins + ib));
            } else {
                if (l4 < span_n)      { summ[ib] = s0;      bins[ib] = (u8)pbytes; }
                if (l4 + 1u < span_n) { summ[ib + 1u] = s1; bins[ib + 1u] = (u8)(pbytes >> 8); }
                if (l4 + 2u < span_n) { summ[ib + 2u] = s2; bins[ib + 2u] = (u8)(pbytes >> 16); }
            }
            if (!more_spans) break;
            span += wstride; k0 = n0; k1 = n1; k2 = n2; k3 = n3;
        }
    }
    if (lane == 0) n_tasks[region] = my_n < region_cap ? my_n : region_cap;
}

#define LZ_ST_TPB 512                                // lanes per workgroup of k_scan_tasks: two workgroups share a CU (the tables are 64 KiB of LDS), 16 waves per CU (256: 5.3 ms per step, 512: 4.4, 1024: 4.2)
// TAGGED (MODE 0, the fused path): out takes the whole tagged record, over the provisional one the queued hit left (payload
// and SLOW flag were missing).  Otherwise the task's hit gets its summary (k_scan_hits left the slot alone).
template <int MODE, bool TAGGED>
__global__ void __launch_bounds__(LZ_ST_TPB)
k_scan_tasks(LzExtendParams P, LzLutParams Q, const LzLutEntry* __restrict__ lut_g, const s32* __restrict__ score_tab_g, const LzScanTask* __restrict__ tasks,
             const u32* __restrict__ n_tasks, u32 n_regions, u32 region_cap, std::conditional_t<TAGGED, u64, u32>* __restrict__ out)
{
    constexpr bool SP = MODE == 1;
    static_assert(!(SP && TAGGED), "pos1 is recovered from the windows a scan ran: without special bytes only");
    __shared__ LzLutEntry lut[LZ_LUT_TOTAL];
    __shared__ s32 ctab[SP ? LZ_NCLASS * LZ_NCLASS : 1];
    for (u32 k = threadIdx.x; k < LZ_LUT_TOTAL; k += LZ_ST_TPB) lut[k] = lut_g[k];
    if (SP) for (u32 k = threadIdx.x; k < LZ_NCLASS * LZ_NCLASS; k += LZ_ST_TPB) ctab[k] = score_tab_g[k];
    __syncthreads();
    for (u32 region = blockIdx.x; region < n_regions; region += gridDim.x) {
        const u32 nt = n_tasks[region];
        for (u32 k = threadIdx.x; k < nt; k += (u32)LZ_ST_TPB) {
            const LzScanTask t = tasks[(size_t)region * region_cap + k];
            LzLutScan L = t.L, R = t.R;
            // the hit's pos1 from the task (reading the provisional record back would fetch a line for 8 bytes): a side that goes on
            // (and a task has one) has moved LZ_LUT_WIN_B bases per window it ran -- without special bytes a scan goes on in no other way
            u32 pos1 = 0;
            if constexpr (TAGGED) pos1 = L.alive == 1 ? L.s + (u32)LZ_LUT_WIN_B * L.nwin : R.s - (u32)LZ_LUT_WIN_B * R.nwin;
            while (L.alive == 1 && L.nwin < (u32)LZ_LUT_MAXWIN) lz_lut_step<false, SP>(Q, lut, t.diag, L, ctab);
            while (R.alive == 1 && R.nwin < (u32)LZ_LUT_MAXWIN) lz_lut_step<true, SP>(Q, lut, t.diag, R, ctab);
            const u32 summ = lz_lut_summary(L, R, P.min_score);
            if constexpr (TAGGED) out[t.idx] = lz_hit_record_tagged(lz_hit_key(pos1, pos1 - (u32)t.diag), summ);
            else                  LZ_NT_ST(summ, out + t.idx);
        }
    }
}

static int lz_scan_tpb(int mode)
{
    return mode != 0 ? LZ_SC_TPB : 640;     // 640: five waves per SIMD at 89 VGPRs (512: 72.5, 640: 69.7, 768 with 8 spilled registers: 75.9 ms per step)
}
// The task list for n hits scanned by n_regions waves (k_scan_hits in `mode`, or k_scan_hits2 as mode 0): one region
// per wave, room for 1/32 of the wave's hits + 64; a hit that finds its region full is left to phase B.
// (64 B each; ~3 % of the hits become tasks on plain sequences: 1/32 of them fit, 2 GiB less to allocate than with 1/8.
// With special bytes that do not end a scan -- IUPAC codes -- every window that meets one goes on as a task as well:
// 1/12, or the overflow lands on phase B's slow path: 1 % of the hits there took k_settle2 from 20 to 84 ms.)
static int lz_task_regions(LzCtx& c, int mode, u64 n, u32 n_regions, u32& region_cap)
{
    region_cap = (u32)std::min<u64>(n / (mode == 1 ? 12 : 32) / n_regions + 64, 1u << 20);
    if (const u32 force = lz_settings().task_region_cap) region_cap = force;   // test hook: tiny regions, so that hits find theirs full
    int rc;
    if (mode < 2 && (rc = c.scan_tasks.ensure((size_t)n_regions * region_cap * sizeof(LzScanTask)))) return rc;
    return c.scan_ntasks.ensure((size_t)n_regions * 4);
}
// grid of k_scan_hits for n hits, and the summaries and task list
static int lz_scan_buffers(LzCtx& c, int mode, u64 n, u32& grid, u32& n_regions, u32& region_cap)
{
    const u32 wpg = (u32)lz_scan_tpb(mode) / 64u;
    const int cus = c.num_cus;
    const u64 nspans = (n + 64u * LZ_SC_ROUNDS - 1) / (64u * LZ_SC_ROUNDS), want = (nspans + wpg - 1) / wpg;
    grid = (u32)std::min<u64>(want ? want : 1, 2u * (u64)cus);                 // two workgroups per CU
    n_regions = grid * wpg;
    const int rc = c.summ.ensure((size_t)n * 4);
    return rc ? rc : lz_task_regions(c, mode, n, n_regions, region_cap);
}
// those buffers for chunks of up to max_n hits (sized once per search: chunk sizes differ a little, and a
// device buffer that grows is freed and allocated again)
int lzk_scan_reserve(LzCtx& c, int mode, u64 max_n)
{
    u32 grid, n_regions, region_cap;
    return lz_scan_buffers(c, mode, max_n, grid, n_regions, region_cap);
}

// phase A of the n hits in c.keys: summaries -> c.summ, the partition byte of every hit -> c.bins
int lzk_scan_hits(LzCtx& c, int mode, const LzExtendParams& P, const LzLutParams& Q, u64 n)
{
    if (n == 0) return 0;
    const int cus = c.num_cus;
    int rc;
    u32 grid, n_regions, task_cap;
    if ((rc = lz_scan_buffers(c, mode, n, grid, n_regions, task_cap))) return rc;
    const u64* keys = c.keys.as<u64>(); const s32* score_tab = c.score_tab.as<s32>(); const LzLutEntry* lut = c.lut.as<LzLutEntry>();
    u32* summ = c.summ.as<u32>(); u8* bins = c.bins.as<u8>(); LzScanTask* tasks = c.scan_tasks.as<LzScanTask>(); u32* ntk = c.scan_ntasks.as<u32>();
    c.timer.begin("k_scan_hits", c.stream);
#define LZ_SCAN_LAUNCH(M_, T_, W_) hipLaunchKernelGGL((k_scan_hits<M_, T_, W_>), dim3(grid), dim3(T_), 0, c.stream, P, Q, keys, n, score_tab, lut, summ, bins, tasks, ntk, task_cap)
    if (mode == 0)      LZ_SCAN_LAUNCH(0, 640, 5);              // (lz_scan_tpb)
    else if (mode == 1) LZ_SCAN_LAUNCH(1, LZ_SC_TPB, 4);
    else                LZ_SCAN_LAUNCH(2, LZ_SC_TPB, 4);
#undef LZ_SCAN_LAUNCH
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    if (mode < 2) {
        const dim3 tgrid(std::min<u32>(n_regions, 4u * (u32)cus));
        c.timer.begin("k_scan_tasks", c.stream);
        if (mode == 0) hipLaunchKernelGGL((k_scan_tasks<0, false>), tgrid, dim3(LZ_ST_TPB), 0, c.stream, P, Q, lut, score_tab, tasks, ntk, n_regions, task_cap, summ);
        else           hipLaunchKernelGGL((k_scan_tasks<1, false>), tgrid, dim3(LZ_ST_TPB), 0, c.stream, P, Q, lut, score_tab, tasks, ntk, n_regions, task_cap, summ);
        c.timer.end(c.stream);
        LZ_HIP(hipGetLastError());
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// The fused path of scan mode 0: hit enumeration and phase A in one kernel, over a context-inlined table.
//   k_build_wctx          (table_kernels.hip) the 32 bytes of the target's 2-bit array around every table entry, beside the entry
//   k_scan_hits2          k_fill_hits2's steps 1-2 (lz_enum_place.inc, lz_enum_owners.inc: the same text), then per hit: wpos[e] + wctx[e] + the query windows
//                         (which depend on pos2 alone: one line per entry), lz_scan_round<false>, ONE tagged 8-byte record at the
//                         hit's place in discovery order.  No keys, no summaries, no partition bytes.  Persistent waves (the
//                         64 KiB tables are loaded once per workgroup) that stride over the 64-entry groups of the sorted list.
//   k_scan_tasks<0, true> replaces the provisional record a queued hit left.
//   k_partition<true>     sorts the tagged records in place.
// the loads of one trip of 64 hits (issued a trip ahead of the arithmetic)
struct LzFuseTrip { u32 p1, pos2, dst; bool ok; LzWctx cx; LzVec16 ql, qr; };

template <bool SELF, int TPB, int CAP>
__global__ void __launch_bounds__(TPB)
k_scan_hits2(u32 lo, u32 i0, u32 i1, LzSeedDev sd,
             const u32* __restrict__ wstart, const u32* __restrict__ wpos, const LzWctx* __restrict__ wctx,
             const u32* __restrict__ sk, const u32* __restrict__ sv, u32 n, const u64* __restrict__ off, u64 base,
             LzExtendParams P, LzLutParams Q, const LzLutEntry* __restrict__ lut_g,
             u64* __restrict__ recs, LzScanTask* __restrict__ tasks, u32* __restrict__ n_tasks, u32 region_cap, LzSelfDev self)
{
    __shared__ LzLutEntry lut[LZ_LUT_TOTAL];
    constexpr int WORDS = CAP / 2 / 64;
    __shared__ LzListWave<CAP> shw[TPB / 64];
    for (u32 k = threadIdx.x; k < LZ_LUT_TOTAL; k += TPB) lut[k] = lut_g[k];
    __syncthreads();
    LzListWave<CAP>& sh = shw[threadIdx.x >> 6];
    unsigned short* const own = reinterpret_cast<unsigned short*>(sh.own32);
    const u32 lane = threadIdx.x & 63u;
    const u32 region = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (TPB / 64);
    LzScanTask* const my_tasks = tasks + (size_t)region * region_cap;
    u32 my_n = 0;
    const u32 ngroups = (n + 63u) / 64u;
    for (u32 grp = region; grp < ngroups; grp += nwaves) {      // wave-uniform
        const u32 j = grp * 64u + lane;                         // one sorted entry per lane
        u32 w_l = 0, i_l = 0; bool in = false;
        if (j < n) { w_l = sk[j] & ((2u << sd.weight) - 1u); i_l = sv[j]; in = !(w_l >> sd.weight) && i_l >= i0 && i_l < i1; }
        if (!__ballot(in)) continue;
        const u32 dbase = in ? (u32)(off[i_l] - base) : 0u;
        const u32 pos2 = lo + i_l + 1u;
        u32 slo = 0, shi = 0;
        if (SELF) lz_self_bounds(self, pos2, slo, shi);
        u32 carry = 0;
        for (int r = 0; r < sd.nprobes; r += LZ_FILL_GROUP) {
            // ---- 1. the lane's lists and their places in the wave's concatenation
#include "lz_enum_place.inc"
            // ---- 2. + 3., a piece of CAP hits at a time
            for (u32 cs = 0; cs < T; cs += CAP) {                // uniform
                const u32 tc = (T - cs < (u32)CAP) ? T - cs : (u32)CAP;
#include "lz_enum_owners.inc"
                // ---- 3. the hits of the piece, 64 per trip: table entry + context + query windows -> both scans' first
                // windows -> the tagged record.  Two register sets take turns: a trip's loads are issued before the
                // arithmetic of the trip before it.  (A lane beyond the end of the piece loads the last hit again.)
                auto load_trip = [&](u32 tb, LzFuseTrip& t) {
                    const u32 t0 = tb + lane;
                    t.ok = t0 < tc;
                    const u32 tt = t.ok ? t0 : tc - 1u;
                    const u32 list = (u32)own[tt] - 1u;
                    const u32 ls = sh.lsrc[list];
                    const uint2 en = sh.ent[list / LZ_FILL_GROUP];
                    const u32 tabs = cs + tt, e = ls + tabs;
                    t.p1 = wpos[e]; t.cx = wctx[e];
                    t.pos2 = en.y; t.dst = en.x + tabs;
                    const u32 sql = en.y - 1u + (u32)LZ_PAD2;     // (lz_scan_fetch: stl - diag, str - diag)
                    t.ql = lz_load16(Q.q2 + ((sql >> 2) - 15u)); t.qr = lz_load16(Q.q2 + ((sql + 1u) >> 2));
                };
                auto scan_trip = [&](const LzFuseTrip& t) {
                    const u64 key = lz_hit_key(t.p1, t.pos2);
                    LzLutRaw<false> rl, rr;
                    lz_wctx_windows(t.cx, t.p1, rl.tv, rr.tv);
                    rl.qv = t.ql; rr.qv = t.qr;
                    u32 summ;
                    lz_scan_round<false>(P, Q, lut, nullptr, key, t.ok, rl, rr, t.dst, lane, summ, my_tasks, my_n, region_cap);
                    // (a queued hit: summ == 0, the provisional record k_scan_tasks completes)
                    if (t.ok) LZ_NT_ST(lz_hit_record_tagged(key, summ), recs + t.dst);
                };
                LzFuseTrip ta, tb2;
                load_trip(0u, ta);
#pragma unroll 1
                for (u32 tb = 0;;) {                             // uniform
                    if (tb + 64u < tc) load_trip(tb + 64u, tb2);
                    scan_trip(ta);
                    tb += 64u; if (tb >= tc) break;
                    if (tb + 64u < tc) load_trip(tb + 64u, ta);
                    scan_trip(tb2);
                    tb += 64u; if (tb >= tc) break;
                }
                __atomic_signal_fence(__ATOMIC_SEQ_CST);
            }
            carry += total;
        }
    }
    if (lane == 0) n_tasks[region] = my_n < region_cap ? my_n : region_cap;
}

// LDS: the tables + a wave's own[] of CAP cells and 4.5 KiB of lists: 8 waves x 2560 cells, 12 x 1024 or 16 x 512 in 160 KiB.
// The kernel is bound by the latency of the scans' dependent table look-ups, which only other waves hide: 84.5, 67.9, 61.6 ms per
// step on the 50 Mbp pair with 8, 12, 16 waves (121 VGPRs: four waves per SIMD), however short the pieces get.  A
// self-comparison's clipping needs 177 registers: it runs with 8 waves (and so does a position filter, the same instantiation).
static u32 lz_fused_tpb(LzCtx& c)
{
    return c.self.mode != LZ_SELF_OFF ? 512u : 1024u;
}
// the fused kernel's grid (one workgroup per CU: its LDS) and the task list
static int lz_fused_buffers(LzCtx& c, u64 n_hits, u32& grid, u32& n_regions, u32& region_cap)
{
    const int cus = c.num_cus;
    grid = (u32)cus; n_regions = grid * (lz_fused_tpb(c) / 64u);
    return lz_task_regions(c, 0, n_hits, n_regions, region_cap);
}
int lzk_fused_reserve(LzCtx& c, u64 max_n)
{
    u32 grid, n_regions, region_cap;
    return lz_fused_buffers(c, max_n, grid, n_regions, region_cap);
}
// lzk_fill_hits + lzk_scan_hits of mode 0 in one launch: the hits of chunk ch as tagged records in c.keys, in discovery order
int lzk_scan_fused(LzCtx& c, u32 lo, const LzChunk& ch, u32 n, const LzExtendParams& P, const LzLutParams& Q)
{
    if (n == 0 || ch.i1 <= ch.i0 || ch.nh == 0) return 0;
    const u32* sk = c.wsk.as<u32>(); const u32* sv = c.wsv.as<u32>();
    lz_chunk_range(c, ch.i0, ch.i1, sk, sv, n);
    if (n == 0) return 0;
    int rc;
    u32 grid, n_regions, region_cap;
    if ((rc = lz_fused_buffers(c, ch.nh, grid, n_regions, region_cap))) return rc;
    const LzLutEntry* lut = c.lut.as<LzLutEntry>(); u64* tagged = c.keys.as<u64>();
    LzScanTask* tasks = c.scan_tasks.as<LzScanTask>(); u32* ntk = c.scan_ntasks.as<u32>();
    c.timer.begin("k_scan_hits", c.stream);
#define LZ_FUSED_LAUNCH(S_, T_, C_, self_) hipLaunchKernelGGL((k_scan_hits2<S_, T_, C_>), dim3(grid), dim3(T_), 0, c.stream, lo, ch.i0, ch.i1, c.seed, c.wstart.as<u32>(), c.wpos.as<u32>(), \
                           c.wctx.as<LzWctx>(), sk, sv, n, c.off.as<u64>(), ch.base, P, Q, lut, tagged, tasks, ntk, region_cap, self_)
    if (c.self.mode != LZ_SELF_OFF) LZ_FUSED_LAUNCH(true, 512, 2560, c.self);
    else                            LZ_FUSED_LAUNCH(false, 1024, 512, LzSelfDev{});
#undef LZ_FUSED_LAUNCH
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    c.timer.begin("k_scan_tasks", c.stream);
    hipLaunchKernelGGL((k_scan_tasks<0, true>), dim3(std::min<u32>(n_regions, 4u * grid)), dim3(LZ_ST_TPB), 0, c.stream, P, Q, lut, (const s32*)nullptr, tasks, ntk, n_regions, region_cap, tagged);
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    return 0;
}
