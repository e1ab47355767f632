// lz_lut.hpp -- phase A of the seed stage on 2-bit codes: the two X-drop scans of a raw hit
// (xdrop_extend_seed_hit loops 1 and 2, src/seed_search.c:2623-2632, 2684-2693) advance FOUR bases per
// step through a look-up table held in LDS, instead of one base per step.
//
// Why this is exact.  Let run / best be the reference's running and best score of one scan and
// m = run - best + xDrop >= 0 its margin (the loop test "run >= best - xDrop" is m >= 0).  For the next
// four bases with prefix sums P1..P4 (P4 = C), minP = min Pj, maxP = max Pj:
//   * the scan stops inside the group  <=>  m + minP < 0, PROVIDED no group can lose more than xDrop from a
//     prefix maximum set inside the same group (checked when the table is built: the loss over the one, two or
//     three bases after a maximum is <= xDrop; with HOXD70 it is at most 375 against xDrop 910);
//   * otherwise best' = max(best, run + maxP), run' = run + C, i.e. m' = min(m, xDrop - max(maxP,0)) + C.
// An entry holds A = max(0,-minP), B' = xDrop - max(maxP,0) and the four scores as signed bytes (C is their
// sum: one v_dot4 adds it); a step is one LDS read, two compares and a handful of integer operations for four
// bases, WITHOUT any branch: a lane whose scan has stopped keeps its state through selects, so that the wave
// executes straight-line code.  The group in which the scan stops (or which is cut by the end of the
// sequences / a byte that is not A,C,G,T) is then walked base by base with the reference's own loop.
//
// Table index.  The 2-bit codes are stored Gray-coded (A=0, C=1, G=3, T=2) so that for every matrix that is
// invariant under complementing both bases (M[a][b] == M[3-a][3-b]: every strand-symmetric DNA matrix, HOXD70
// included) the score depends on x = t ^ q and the low bit of t only: 3 bits per base, 12 bits per group of
// four, 4096 entries of 8 bytes.  Four bases are one byte of the code stream, so that a group's index is one byte
// of (t ^ q) and one nibble of the compressed low-bit plane of t.  There are TWO tables of 4096 entries: one for
// bases consumed in ascending order inside a byte (loop 2) and one for descending order (loop 1: the 16 bytes
// that END at the scan position are shifted so that the first base consumed is the top pair of byte 14 and group g
// is byte 14 - g) -- 64 KiB of LDS, two workgroups per CU on the 160 KiB of gfx950.  (Round 2 kept one table and
// turned the left window around with v_bfrev + a swap of neighbouring bits per word: 32 VALU instructions per hit
// in a kernel that is bound by VALU issue.)  Entries are 8-byte aligned: one ds_read_b64 per group (a 4-byte
// aligned struct compiled to ds_read2_b32: two banked passes per look-up).
//
// Bytes outside the 2-bit alphabet ("specials": lower case, N, the NUL between partitions, ...) are kept in a
// separate 1-bit-per-base mask; a scan that meets a mask bit consumes that base with its real score, from the byte
// codes and the class table (lz_lut_window).  (lzh_lut_eligible checks the matrix over A, C, G, T; any matrix it turns
// down runs the byte-code scans of lz_common.hpp.)
//
// The functions here are the per-lane device logic (LZ_HD: also compiled for the host by tests/emul).
#pragma once
#include "lz_common.hpp"

#define LZ_PAD2         128          // padding bases in front of base 0 in the 2-bit and mask arrays (and >= that after the end)
#define LZ_LUT_ENTRIES  4096         // 4 bases x 3 bits, per direction
#define LZ_LUT_TOTAL    (2 * LZ_LUT_ENTRIES)   // [0, 4096): ascending (right scans), [4096, 8192): descending (left scans)
#define LZ_LUT_WIN_G    15           // groups per 16-byte window
#define LZ_LUT_WIN_B    60           // bases per window
#define LZ_LUT_MAXWIN   3            // windows per scan (180 bases); a scan still alive after that makes the hit SLOW
#define LZ_GRAY(c)      ((c) ^ ((c) >> 1))      // 2-bit code as stored in the phase-A arrays

struct alignas(8) LzLutEntry { u32 ab; u32 sc; };          // ab = A (u16) | B' (s16) << 16; sc = the four scores, signed bytes, first consumed in byte 0

struct LzLutParams {
    const u8* t2; const u8* q2;                   // Gray 2-bit codes: base i at bits 2*((i+PAD2)&3) of byte (i+PAD2)>>2
    const u8* tsp; const u8* qsp;                 // special masks: base i at bit (i+PAD2)&7 of byte (i+PAD2)>>3
    const u8* t2x; const u8* tspx;                // the target's two arrays once more, in 64-byte blocks that overlap by half
                                                  // (block k = bytes [32k, 32k+64) of the plain array; scan_kernels.hip::lz_scan_fetch)
    const u8* tcode; const u8* qcode;             // the code bytes (lz_common.hpp): a special base met by a scan is scored from its class
    s32 xdrop;
};

struct LzLutScan { u32 s; s32 run, best; u32 room, used, alive, nwin; };   // alive: 0 stopped, 1 goes on, 2 undecided (-> SLOW)

#if defined(__HIP_DEVICE_COMPILE__)
LZ_HD u32 lz_alignbit(u32 hi, u32 lo, u32 sh) { return __builtin_amdgcn_alignbit(hi, lo, sh); }
LZ_HD s32 lz_sdot4(u32 a, s32 acc) { return __builtin_amdgcn_sdot4((int)a, 0x01010101, acc, false); }
LZ_HD s32 lz_sdot4m(u32 a, u32 ones, s32 acc) { return __builtin_amdgcn_sdot4((int)a, (int)ones, acc, false); }   // acc + the bytes of a that `ones` selects
LZ_HD u32 lz_byte_pair(u32 hi_src, u32 lo_src, int k)    // (byte k of hi_src) << 8 | byte k of lo_src
{ return __builtin_amdgcn_perm(hi_src, lo_src, 0x0C0C0000u | ((u32)(4 + k) << 8) | (u32)k); }
#define LZ_UNROLL_ALL _Pragma("unroll")
#else
LZ_HD u32 lz_alignbit(u32 hi, u32 lo, u32 sh) { sh &= 31u; return sh ? (lo >> sh) | (hi << (32u - sh)) : lo; }
LZ_HD s32 lz_sdot4(u32 a, s32 acc) { for (int k = 0; k < 4; k++) acc += (s32)(int8_t)(a >> (8 * k)); return acc; }
LZ_HD s32 lz_sdot4m(u32 a, u32 ones, s32 acc) { for (int k = 0; k < 4; k++) acc += (s32)(int8_t)(a >> (8 * k)) * (s32)((ones >> (8 * k)) & 0xFFu); return acc; }
LZ_HD u32 lz_byte_pair(u32 hi_src, u32 lo_src, int k) { return (((hi_src >> (8 * k)) & 0xFFu) << 8) | ((lo_src >> (8 * k)) & 0xFFu); }
#define LZ_UNROLL_ALL
#endif
LZ_HD u32 lz_ctz64(u64 x) { return (u32)__builtin_ctzll(x); }
LZ_HD u32 lz_clz64(u64 x) { return (u32)__builtin_clzll(x); }

// the raw bytes of one window: 16 bytes of each code stream (+ 16 bytes of each special mask)
template <bool SPECIAL> struct LzLutRaw { LzVec16 tv, qv, tm, qm; };
template <> struct LzLutRaw<false> { LzVec16 tv, qv; };
// group g of a window is byte g of the aligned stream with base s at bit 0 (RIGHT), resp. byte 14 - g with base s-1
// in the top pair of byte 14 (LEFT)
#define LZ_LUT_GBYTE(RIGHT_, g_) ((RIGHT_) ? (g_) : 14 - (g_))
template <bool RIGHT, bool SPECIAL>
LZ_HD void lz_lut_fetch(const LzLutParams& P, u32 s_, s32 diag, LzLutRaw<SPECIAL>& raw)
{
    // byte offsets fit 32 bits (sequences are shorter than 2^31 bases): 32-bit address arithmetic on top of the
    // array bases.  RIGHT: the 16 bytes that start with the byte of base s; LEFT: the 16 bytes that END with the
    // byte of base s-1 (lz_lut_window shifts them so that this base becomes the top pair of byte 14).
    const u32 st = RIGHT ? s_ + (u32)LZ_PAD2 : s_ - 1u + (u32)LZ_PAD2;
    const u32 sq = st - (u32)diag;
    const u32 back = RIGHT ? 0u : 15u;
    raw.tv = lz_load16(P.t2 + ((st >> 2) - back)); raw.qv = lz_load16(P.q2 + ((sq >> 2) - back));
    if constexpr (SPECIAL) {
        const u32 mback = RIGHT ? 0u : 14u;
        raw.tm = lz_load16(P.tsp + ((st >> 3) - mback)); raw.qm = lz_load16(P.qsp + ((sq >> 3) - mback));
    }
}
// 64 mask bits of one sequence from the 16 bytes lz_lut_fetch loaded: RIGHT: bit j = base s+j; LEFT: bit 63-j = base s-1-j
template <bool RIGHT>
LZ_HD u64 lz_lut_mask64(const LzVec16& v, s64 s)
{
    if (RIGHT) {
        const u32 k = (u32)((u64)(s + LZ_PAD2) & 7u);
        return ((u64)lz_alignbit(v.w[2], v.w[1], k) << 32) | lz_alignbit(v.w[1], v.w[0], k);
    }
    const u32 k = 17u + (u32)((u64)(s - 1 + LZ_PAD2) & 7u);     // base s-1 is bit 112 + k' of the loaded bits = bit 80 + k' of (v >> 32) -> bit 63
    return ((u64)lz_alignbit(v.w[3], v.w[2], k) << 32) | lz_alignbit(v.w[2], v.w[1], k);
}

// One 16-byte window (up to 60 bases = 15 groups) of one scan.  lut = both tables (lzh_lut_build).
// LIMCHK == false: the caller guarantees 60 plain bases (st.room >= 60, no special byte in reach): the limit tests
// drop out of the straight-line part and the stopping group needs no general walk.
// On return st.alive says whether the scan goes on into the next window.
// ctab (SPECIAL only): the 32 x 32 class table.  A special base inside the window -- anything that is not A, C, G, T: lower
// case, N, an IUPAC code, the NUL between partitions -- is consumed with its REAL score, as one step of the reference's
// loop: the usual special byte scores far below -xDrop and ends the scan there; one that does not (IUPAC bytes in an
// unmasked matrix: -100 against everything by default) lets the scan go on BEHIND it, as a new window from the next base
// (round 3 sent every search whose sequences held such a byte to the byte-code scans, 2.4 x slower: VERDICT r3 #6).
template <bool RIGHT, bool SPECIAL, bool LIMCHK>
LZ_HD void lz_lut_window(const LzLutParams& P, const LzLutEntry* lut, s32 diag, LzLutScan& st, const LzLutRaw<SPECIAL>& raw, const s32* ctab = nullptr)
{
    const s32 X = P.xdrop;
    const LzLutEntry* const tab = lut + (RIGHT ? 0 : LZ_LUT_ENTRIES);
    const u32 spad = RIGHT ? st.s + (u32)LZ_PAD2 : st.s - 1u + (u32)LZ_PAD2, qpad = spad - (u32)diag;
    u32 tw[4], qw[4];
    {
        // RIGHT: base s to bit 0.  LEFT: base s-1 (pair 60 + r of the 64 loaded) to pair 59, the top of byte 14: a
        // right shift of r + 1 pairs, never zero.
        const u32 a = RIGHT ? 2u * (spad & 3u) : 2u * (spad & 3u) + 2u;
        const u32 b = RIGHT ? 2u * (qpad & 3u) : 2u * (qpad & 3u) + 2u;
        tw[0] = lz_alignbit(raw.tv.w[1], raw.tv.w[0], a); tw[1] = lz_alignbit(raw.tv.w[2], raw.tv.w[1], a); tw[2] = lz_alignbit(raw.tv.w[3], raw.tv.w[2], a); tw[3] = raw.tv.w[3] >> a;
        qw[0] = lz_alignbit(raw.qv.w[1], raw.qv.w[0], b); qw[1] = lz_alignbit(raw.qv.w[2], raw.qv.w[1], b); qw[2] = lz_alignbit(raw.qv.w[3], raw.qv.w[2], b); qw[3] = raw.qv.w[3] >> b;
    }
    u32 lim = st.room < (u32)LZ_LUT_WIN_B ? st.room : (u32)LZ_LUT_WIN_B;
    bool soft = false;
    if constexpr (SPECIAL) {
        const s64 s = (s64)st.s, sq = s - (s64)diag;
        const u64 sm = lz_lut_mask64<RIGHT>(raw.tm, s) | lz_lut_mask64<RIGHT>(raw.qm, sq);
        const u32 nsp = sm ? (RIGHT ? lz_ctz64(sm) : lz_clz64(sm)) : 64u;
        if (nsp < lim) { soft = true; lim = nsp; }
    }
    // index planes: x = t ^ q (one byte per group), wc = the low bits of t's codes, four per byte in its low nibble
    u32 xw[4], wc[4];
    LZ_UNROLL_ALL
    for (int k = 0; k < 4; k++) {
        xw[k] = tw[k] ^ qw[k];
        const u32 u = (tw[k] & 0x11111111u) | ((tw[k] >> 1) & 0x22222222u);
        wc[k] = (u | (u >> 2)) & 0x0F0F0F0Fu;
    }
    // ---- the straight-line part: every group whose four bases lie inside the limit, until the margin test fails
    const u32 glim = lim >> 2;
    s32 run = st.run, m = run - st.best + X;
    u32 np = 0, fsc = 0;                                        // groups passed; the scores of the group the walk stopped in
#if !defined(LZ_LUT_NO_EARLY_EXIT) && defined(__HIP_DEVICE_COMPILE__)
    // a lane leaves the straight-line part at its first failing group (divergent exit: the lane is masked off in
    // EXEC, nothing has to be frozen with selects: 7 instead of 11 VALU instructions per group; measured
    // k_scan_hits 81 -> 77 ms per step against the select form below, which the host build keeps)
    {
        // the entries of even / odd groups in two variables that take turns: the one the walk stopped on is still
        // there after the exit (no per-group copy of it)
#define LZ_LUT_ENTRY_OF(g_) tab[lz_byte_pair(wc[LZ_LUT_GBYTE(RIGHT, g_) >> 2], xw[LZ_LUT_GBYTE(RIGHT, g_) >> 2], LZ_LUT_GBYTE(RIGHT, g_) & 3)]
        LzLutEntry ea = LZ_LUT_ENTRY_OF(0), eb = ea;
        LZ_UNROLL_ALL
        for (int g = 0; g < LZ_LUT_WIN_G; g += 2) {
            if (g + 1 < LZ_LUT_WIN_G) eb = LZ_LUT_ENTRY_OF(g + 1);
            if (m < (s32)(ea.ab & 0xFFFFu)) goto groups_done;
            if (LIMCHK && (u32)g >= glim) goto groups_done;
            { const s32 bq = (s32)ea.ab >> 16; m = lz_sdot4(ea.sc, m < bq ? m : bq); run = lz_sdot4(ea.sc, run); np = (u32)g + 1u; }
            if (g + 1 < LZ_LUT_WIN_G) {
                if (g + 2 < LZ_LUT_WIN_G) ea = LZ_LUT_ENTRY_OF(g + 2);
                if (m < (s32)(eb.ab & 0xFFFFu)) goto groups_done;
                if (LIMCHK && (u32)(g + 1) >= glim) goto groups_done;
                { const s32 bq = (s32)eb.ab >> 16; m = lz_sdot4(eb.sc, m < bq ? m : bq); run = lz_sdot4(eb.sc, run); np = (u32)g + 2u; }
            }
        }
        groups_done:
        fsc = (np & 1u) ? eb.sc : ea.sc;
#undef LZ_LUT_ENTRY_OF
    }
#else
    {
        bool dead = false;
        LZ_UNROLL_ALL
        for (int g = 0; g < LZ_LUT_WIN_G; g++) {
            const int by = LZ_LUT_GBYTE(RIGHT, g);
            const LzLutEntry e = tab[lz_byte_pair(wc[by >> 2], xw[by >> 2], by & 3)];
            if (!dead) fsc = e.sc;
            dead = dead | (m < (s32)(e.ab & 0xFFFFu));
            if (LIMCHK) dead = dead | ((u32)g >= glim);
            const s32 bq = (s32)e.ab >> 16;
            const s32 t = lz_sdot4(e.sc, m < bq ? m : bq);
            const s32 r2 = lz_sdot4(e.sc, run);
            m = dead ? m : t; run = dead ? run : r2; np += dead ? 0u : 1u;
        }
    }
#endif
    // ---- the group the straight-line part stopped in (np < 15), base by base: the reference's loop
    u32 r = 0;
    if (np < (u32)LZ_LUT_WIN_G) { r = lim - 4u * np; if (r > 4u) r = 4u; }       // 4: the margin test failed inside the limit
    s32 best = run - m + X;
    const u32 sc = fsc;
    bool stop = false; u32 j = 0;
    if (LIMCHK) {
        LZ_UNROLL_ALL
        for (u32 b = 0; b < 4; b++) {
            const bool on = !stop && b < r;
            const s32 nr = run + (s32)(int8_t)(sc >> (8u * b));
            run = on ? nr : run;
            j += on ? 1u : 0u;
            best = (on && nr > best) ? nr : best;
            stop = stop | (on && nr < best - X);
        }
    } else if (r) {
        // the margin test failed in this group: the scan stops on its first base that takes the margin below zero,
        // and its best does not move (a group cannot gain and then lose more than xDrop); run no longer matters
        const s32 p1 = lz_sdot4m(sc, 0x00000001u, m), p2 = lz_sdot4m(sc, 0x00000101u, m), p3 = lz_sdot4m(sc, 0x00010101u, m), p4 = lz_sdot4(sc, m);
        const s32 q2 = p1 | p2, q3 = q2 | p3;                   // sign bit: some prefix so far is negative
        j = 4u + (u32)(p1 >> 31) + (u32)(q2 >> 31) + (u32)(q3 >> 31);
        stop = (q3 | p4) < 0;
    }
    st.run = run; st.best = best;
    st.used += 4u * np + j;
    st.nwin++;
    if (stop) st.alive = 0;
    else if (r == 4u) st.alive = 2;                                     // cannot happen with an eligible table: "undecided", the hit becomes SLOW
    else if (soft) {                                                    // the special base: one step of the reference's loop
        if constexpr (SPECIAL) {
            const u32 p1 = RIGHT ? st.s + lim : st.s - 1u - lim;
            const s32 v = ctab[(LZ_CODE_CLASS(P.tcode[(s64)p1]) << 5) | LZ_CODE_CLASS(P.qcode[(s64)p1 - (s64)diag])];
            st.run += v; st.used += 1u;
            if (st.run > st.best) st.best = st.run;
            const u32 eaten = lim + 1u;
            if (st.run < st.best - X || eaten == st.room) st.alive = 0;       // it ends the scan (as a rule), or the sequence ends behind it
            else { st.alive = 1; st.room -= eaten; st.s = RIGHT ? st.s + eaten : st.s - eaten; }   // the scan goes on behind it
        }
    }
    else if (lim == st.room) st.alive = 0;                              // end of a sequence / the left stop
    else { st.alive = 1; st.room -= (u32)LZ_LUT_WIN_B; st.s = RIGHT ? st.s + (u32)LZ_LUT_WIN_B : st.s - (u32)LZ_LUT_WIN_B; }
}
// the first windows of both scans of a hit (do_l / do_r: which of them this lane runs).  (Stepping the two windows
// side by side in one instruction stream -- two dependent chains per lane -- was measured and lost: 138 VGPRs,
// three waves per SIMD instead of four, the fused scan + partition kernel of round 2 120 -> 167 ms per step.)
template <bool SPECIAL, bool LIMCHK>
LZ_HD void lz_lut_window_pair(const LzLutParams& P, const LzLutEntry* lut, s32 diag, LzLutScan& L, LzLutScan& R,
                              const LzLutRaw<SPECIAL>& rawl, const LzLutRaw<SPECIAL>& rawr, bool do_l, bool do_r, const s32* ctab = nullptr)
{
    if (do_l) lz_lut_window<false, SPECIAL, LIMCHK>(P, lut, diag, L, rawl, ctab);
    if (do_r) lz_lut_window<true, SPECIAL, LIMCHK>(P, lut, diag, R, rawr, ctab);
}
// fetch + window
template <bool RIGHT, bool SPECIAL>
LZ_HD void lz_lut_step(const LzLutParams& P, const LzLutEntry* lut, s32 diag, LzLutScan& st, const s32* ctab = nullptr)
{
    LzLutRaw<SPECIAL> raw;
    lz_lut_fetch<RIGHT, SPECIAL>(P, st.s, diag, raw);
    if (!SPECIAL && st.room >= (u32)LZ_LUT_WIN_B) lz_lut_window<RIGHT, SPECIAL, false>(P, lut, diag, st, raw);
    else                                           lz_lut_window<RIGHT, SPECIAL, true>(P, lut, diag, st, raw, ctab);
}

// scan set-up of one raw hit (diagEnd == 0, as in lz_probe_head)
LZ_HD void lz_lut_init(u64 key, u32 tlen, u32 qlen, s32& diag, LzLutScan& L, LzLutScan& R)
{
    const u32 pos2 = (u32)key;
    diag = (s32)(u32)(key >> 32);
    const u32 pos1 = pos2 + (u32)diag;
    const s32 stopl = diag > 0 ? diag : 0;
    const s32 stopr = ((s32)tlen <= (s32)qlen + diag) ? (s32)tlen : (s32)qlen + diag;
    L.s = R.s = pos1; L.run = L.best = R.run = R.best = 0; L.used = R.used = 0; L.nwin = R.nwin = 0;
    L.room = (u32)((s32)pos1 - stopl); R.room = (u32)(stopr - (s32)pos1);
    L.alive = ((s32)pos1 > stopl) ? 1u : 0u; R.alive = ((s32)pos1 < stopr) ? 1u : 0u;
}

// the 4-byte phase-A summary (same meaning as lz_probe_summary)
LZ_HD u32 lz_lut_summary(const LzLutScan& L, const LzLutScan& R, s32 min_score)
{
    u32 summ = (L.used & 0xFFu) | ((R.used & 0xFFu) << 8);
    if (L.alive || R.alive || L.best + R.best >= min_score) summ |= LZ_SUMM_SLOW;
    return summ;
}

template <bool SPECIAL>
LZ_HD u32 lz_lut_probe_hit(const LzLutParams& P, const LzLutEntry* lut, u32 tlen, u32 qlen, s32 min_score, u64 key, const s32* ctab = nullptr)
{
    s32 diag; LzLutScan L, R;
    lz_lut_init(key, tlen, qlen, diag, L, R);
    while (L.alive == 1 && L.nwin < (u32)LZ_LUT_MAXWIN) lz_lut_step<false, SPECIAL>(P, lut, diag, L, ctab);
    while (R.alive == 1 && R.nwin < (u32)LZ_LUT_MAXWIN) lz_lut_step<true, SPECIAL>(P, lut, diag, R, ctab);
    return lz_lut_summary(L, R, min_score);
}

// ---- the hit record that travels from phase A to phase B (one u64 per raw hit, partitioned by the high
// 8 bits of hashedDiag, in discovery order inside a partition):
//   bits  0..30  pos2 (end of the seed word in the query)
//   bits 31..38  low 8 bits of hashedDiag (the bucket inside its partition); phase B overwrites them (and bits
//                55..59) with the record's index inside its tile once the record sits in its bucket's list
//   bits 39..54  fast hits: bases the left scan consumed | bases the right scan consumed << 8
//                SLOW hits: bits 16..31 of the diagonal pos1 - pos2 (the low 16 are the bucket)
//   bit  63      SLOW
LZ_HD u64 lz_hit_record(u64 key, u32 summ)
{
    const u32 pos2 = (u32)key, diag = (u32)(key >> 32);
    const bool slow = (summ & LZ_SUMM_SLOW) != 0;
    const u64 payload = slow ? (u64)(diag >> 16) : (u64)(summ & 0xFFFFu);
    return (u64)pos2 | ((u64)(diag & 0xFFu) << 31) | (payload << 39) | (slow ? (1ull << 63) : 0ull);
}
// the record with its partition (bits 8..15 of hashedDiag) riding in the free bits 55..62: the form k_scan_hits2 stores
// and k_partition<true> reads; it clears the tag when it writes the record to its place in the sorted tile
#define LZ_REC_TAG(r)     ((u32)((r) >> 55) & 0xFFu)
#define LZ_REC_UNTAG(r)   ((r) & ~(0xFFull << 55))
LZ_HD u64 lz_hit_record_tagged(u64 key, u32 summ) { return lz_hit_record(key, summ) | ((u64)((u32)(key >> 40) & 0xFFu) << 55); }

// ---- wctx: the target context of a table entry (k_scan_hits2).  Both first windows of a hit lie in the 32 bytes of the
// plain 2-bit array that start at byte bl(pos1) -- the left window is bytes [bl, bl + 16), the right one starts at byte
// br = bl + 15 or bl + 16 (lz_scan_fetch in scan_kernels.hip reads the same bytes from the half-overlapping blocks) --
// and depend on pos1 alone: entry e of wctx holds those 32 bytes for pos1 = wpos[e].
#define LZ_WCTX_BYTES 32
struct alignas(16) LzWctx { u32 w[LZ_WCTX_BYTES / 4]; };
LZ_HD u32 lz_wctx_first_byte(u32 pos1) { return ((pos1 - 1u + (u32)LZ_PAD2) >> 2) - 15u; }
LZ_HD u32 lz_wctx_right_offset(u32 pos1) { return ((pos1 + (u32)LZ_PAD2) >> 2) - lz_wctx_first_byte(pos1); }     // 15 or 16
LZ_HD LzWctx lz_wctx_make(const u8* two, u32 pos1) { LzWctx e; __builtin_memcpy(&e, two + lz_wctx_first_byte(pos1), LZ_WCTX_BYTES); return e; }
LZ_HD void lz_wctx_windows(const LzWctx& e, u32 pos1, LzVec16& tl, LzVec16& tr)
{
    const bool at16 = lz_wctx_right_offset(pos1) == 16u;
    LZ_UNROLL_ALL
    for (int k = 0; k < 4; k++) {
        tl.w[k] = e.w[k];
        const u32 at15 = lz_alignbit(e.w[4 + k], e.w[3 + k], 24u);       // bytes 15 + 4k .. 18 + 4k
        tr.w[k] = at16 ? e.w[4 + k] : at15;
    }
}

#define LZ_REC_POS2(r)    ((u32)((r) & 0x7FFFFFFFu))
#define LZ_REC_LOW8(r)    ((u32)((r) >> 31) & 0xFFu)
#define LZ_REC_PAYLOAD(r) ((u32)((r) >> 39) & 0xFFFFu)
#define LZ_REC_SLOW(r)    ((u32)((r) >> 63))
// the tile index phase B stores in a placed record (13 bits: low 8 in the bucket field, high 5 in bits 55..59)
LZ_HD u64 lz_rec_with_index(u64 r, u32 idx)
{ return (r & ~((0xFFull << 31) | (0x1Full << 55))) | ((u64)(idx & 0xFFu) << 31) | ((u64)((idx >> 8) & 0x1Fu) << 55); }
#define LZ_REC_INDEX(r)   (((u32)((r) >> 31) & 0xFFu) | (((u32)((r) >> 55) & 0x1Fu) << 8))

// ---- phase B: one record of a bucket's stream, in discovery order, with diagEnd[h] in `dend`.
// This is process_for_simple_hit + xdrop_extend_seed_hit (src/seed_search.c:1056-1192, 2528-2959) for hit
// (pos1 = pos2 + diag, pos2): the diagEnd test (:1113), then either the phase-A summary (the unclipped scans
// scored below the threshold: a left scan clipped at diagEnd walks a prefix of the same bases -- its best can
// only be lower, still no HSP -- and the right scan does not depend on it, so only the count of bases differs,
// min(unclipped, room)) or, for SLOW records, the real extension.
template <class Emit>
LZ_HD void lz_settle_record(const LzExtendParams& P, const s32* score_tab, u64 rec, u32 h /*hashedDiag of the bucket*/,
                            u32& dend, u64& n_ext, u64& n_bp, Emit&& emit)
{
    const u32 p2 = LZ_REC_POS2(rec);
    if (dend > p2 - P.seed_len) return;                         // :1113
    n_ext++;
    const u32 pay = LZ_REC_PAYLOAD(rec);
    if (!LZ_REC_SLOW(rec)) {
        const u32 room = p2 - dend, dlo = pay & 0xFFu, dext = pay >> 8;
        const u32 extent = p2 + dext;                           // :2785
        n_bp += (dlo < room ? dlo : room) + dext;               // :2818
        if (extent > dend) dend = extent;
        return;
    }
    const s32 diag = (s32)((pay << 16) | h);
    dend = lz_reextend(P, score_tab, p2, diag, dend, n_bp, emit);
}
