// lz_mismatch.hpp -- the seed stage of `lastz --mismatch=<count>,<length>`: process_for_simple_hit with gfExtend in
// gfexMismatch_min..gfexMismatch_max (src/seed_search.c:1056-1192) and mismatch_extend_seed_hit (:3450-3778), decomposed the
// way lz_exact.hpp decomposes the exact-match extension: phase A looks at every raw hit on its own, phase B walks a bucket's
// hits in discovery order with diagEnd.  The match codes are lz_exact.hpp's: a base pair mismatches unless
// charToBits[t] == charToBits[q] >= 0; NUL, N and everything outside a sequence match nothing, that is, they are mismatches.
//
// What the reference does with the raw hit (pos1, pos2) of a seed of length L on diagonal d = pos1 - pos2, M = gfExtend, in
// query positions (the window is [pos2 - L, pos2)), once the hit has passed the drop test (:1113):
//   * the window is read right to left, E counts its mismatches.  The (M+1)-th ends the hit: no HSP,
//     diagEnd = max(diagEnd, that mismatch's position) (:3512-3525, :3754-3777).
//   * with K = M + 1 - E the left scan collects up to K mismatch positions ("starts"), nearest first (:3574-3598).  It stops
//     early in front of query position max(diagEnd, -d) -- then the position before the stop is one more start -- or on a NUL in
//     either sequence -- then the NUL is (:3605-3606).  shortfall = K - starts (:3608).
//   * the right scan skips `shortfall` mismatches; each further one closes the interval that opens at the next start, leftmost
//     start first (:3651-3666).  A NUL or the end of either sequence closes the current start's interval whatever the
//     shortfall is (:3675-3686).  The longest interval wins, the earliest among equals (strict >, :3659, :3681).
//   * the extent: the winner's right mismatch + 1 if its length >= threshold (:3703); else the leftmost mismatch of the
//     window if E > 0 (:3521); else the first mismatch or stop right of the window (:3649-3650, :3677-3678).
//
// Why phase A is exact.  Let u_1 > u_2 > ... be the mismatches left of the window and r_1 < r_2 < ... those right of it as the
// match codes show them, with no stop at all.  Every real stop is one of them or lies between two of them, so the real starts
// s_i satisfy s_i >= u_i, the real right ends are r_j themselves, and the interval the reference closes at r_j opens at
// s_(K+1-j) or, at a right stop, at a start further right still.  The longest of the K unclipped pairings (u_i, r_(K+1-i)) is
// therefore an upper bound of the length whatever diagEnd is, and below the threshold the hit is no HSP; its extent is then
// the second or third form above, which depend on neither diagEnd nor the stops.  Such a hit -- and every hit with E > M -- is
// FAST: beyond the drop test its whole effect is diagEnd = max(diagEnd, extent), and the extent travels in the record's 16
// payload bits as extent - (pos2 - L) (at most L + LZ_EX_CAP).  A hit that could reach the threshold, or one side of which
// shows fewer than K mismatches within LZ_EX_CAP bases, is SLOW and is extended in phase B against the bucket's real diagEnd.
// The bound is tried in its cheap form first (both K-th mismatches: u_K and r_K bound every pairing) and in its exact form,
// the maximum over the K pairings, only when the cheap one reaches the threshold.
//
// The functions here are the per-lane device logic (LZ_HD: also compiled for the host by tests/emul/emul_mismatch.cpp).
#pragma once
#include "lz_exact.hpp"

#define LZ_MM_MAX   50u                // gfexMismatch_max
#define LZ_MM_LIST  64u                // room for the mismatch positions of one side (K <= LZ_MM_MAX + 1)

struct LzMismatchParams {
    LzExactParams X;                   // the match codes of both sequences, their lengths, the seed's length, the threshold (:3703)
    const u8* traw; const u8* qraw;    // the bytes themselves: phase B asks of a mismatch whether it is a NUL (:3585, :3641)
    u32 M;                             // hp->gfExtend
};

LZ_HD u32 lz_mm_popc(u32 x) { return (u32)__builtin_popcount(x); }
LZ_HD u32 lz_mm_brev(u32 x)
{
#if defined(__clang__)
    return __builtin_bitreverse32(x);
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    return __builtin_bswap32(x);
#endif
}
// the even bits of x, packed
LZ_HD u32 lz_mm_even_bits(u64 x)
{
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    return (u32)(x | (x >> 16));
}
// the 32 base pairs (t + k, q + k): bit k set where they mismatch.  t, q as lz_ex_diff32 takes them
LZ_HD u32 lz_mm_word(const LzExactParams& X, s64 t, s64 q)
{
    u64 d; u32 m;
    lz_ex_diff32(X, t, q, d, m);
    return lz_mm_even_bits(d) | m;
}

// ---- one hit: what both phases know before they scan
struct LzMmHit {
    u32 pos1, pos2;
    s64 d;                             // the diagonal
    u32 win;                           // the window's mismatches: bit k <-> query position pos2 - 32 + k
    u32 E;                             // ... how many
    s64 qstop, qend;                   // the left scan reads no query position below qstop (:3545-3549), the right one none from qend on (:3625-3627)
};
LZ_HD LzMmHit lz_mm_hit(const LzMismatchParams& P, u32 pos1, u32 pos2, u32 dend)
{
    LzMmHit H;
    const u32 L = P.X.seed_len;
    H.pos1 = pos1; H.pos2 = pos2; H.d = (s64)pos1 - (s64)pos2;
    H.win = lz_mm_word(P.X, (s64)pos1 - (s64)LZ_EX_W, (s64)pos2 - (s64)LZ_EX_W) & (0xFFFFFFFFu << (LZ_EX_W - L));
    H.E = lz_mm_popc(H.win);
    H.qstop = (s64)dend > -H.d ? (s64)dend : -H.d;
    const s64 te = (s64)P.X.tlen - H.d;
    H.qend = (s64)P.X.qlen < te ? (s64)P.X.qlen : te;
    return H;
}
// block b of the left scan: the 32 query positions below pos2 - L - 32 b, bit k <-> position pos2 - L - 32 b - 1 - k (the
// nearest first).  A block that lies below qstop altogether is all mismatches, without a load.
LZ_HD u32 lz_mm_block_left(const LzMismatchParams& P, const LzMmHit& H, u32 b)
{
    const s64 top = (s64)H.pos2 - (s64)P.X.seed_len - (s64)LZ_EX_W * (s64)b;
    if (top <= H.qstop) return 0xFFFFFFFFu;
    return lz_mm_brev(lz_mm_word(P.X, top - (s64)LZ_EX_W + H.d, top - (s64)LZ_EX_W));      // (top > qstop >= max(0, -d): both >= -32)
}
// block b of the right scan: bit k <-> query position pos2 + 32 b + k; all mismatches from qend on
LZ_HD u32 lz_mm_block_right(const LzMismatchParams& P, const LzMmHit& H, u32 b)
{
    const s64 q0 = (s64)H.pos2 + (s64)LZ_EX_W * (s64)b;
    if (q0 >= H.qend) return 0xFFFFFFFFu;
    return lz_mm_word(P.X, q0 + H.d, q0);
}

// ---- phase A: the 4-byte summary of one raw hit (low 16 bits = payload of a fast hit, LZ_SUMM_SLOW)
struct LzMmMap { u64 lo, hi; };        // the mismatches of one side within LZ_EX_CAP bases: bit k <-> k bases between it and the window
LZ_HD u32 lz_mm_map_low(const LzMmMap& m) { return m.lo ? lz_ctz64(m.lo) : 64u + lz_ctz64(m.hi); }
LZ_HD u32 lz_mm_map_high(const LzMmMap& m) { return m.hi ? 127u - lz_clz64(m.hi) : 63u - lz_clz64(m.lo); }
LZ_HD void lz_mm_map_clear(LzMmMap& m, u32 k) { if (k < 64u) m.lo &= ~(1ull << k); else m.hi &= ~(1ull << (k - 64u)); }
// all but the K lowest set bits cleared (the map has K at least); returns the K-th
LZ_HD u32 lz_mm_map_keep(LzMmMap& m, u32 K)
{
    LzMmMap c = m;
    for (u32 k = 1; k < K; k++) { if (c.lo) c.lo &= c.lo - 1ull; else c.hi &= c.hi - 1ull; }
    const u32 at = lz_mm_map_low(c);
    if (at < 64u) { m.lo &= at == 63u ? ~0ull : (2ull << at) - 1ull; m.hi = 0; }
    else          { m.hi &= at == 127u ? ~0ull : (2ull << (at - 64u)) - 1ull; }
    return at;
}
static_assert(LZ_EX_CAP == 128u, "LzMmMap holds LZ_EX_CAP bits");
template <bool RIGHT>
LZ_HD u32 lz_mm_map_read(const LzMismatchParams& P, const LzMmHit& H, u32 K, LzMmMap& m)
{
    u32 n = 0;
    m.lo = m.hi = 0;
    for (u32 b = 0; b < LZ_EX_CAP / LZ_EX_W && n < K; b++) {    // (words the count does not need stay unread: zero)
        const u32 w = RIGHT ? lz_mm_block_right(P, H, b) : lz_mm_block_left(P, H, b);
        n += lz_mm_popc(w);
        if (b < 2u) m.lo |= (u64)w << (32u * b); else m.hi |= (u64)w << (32u * (b - 2u));
    }
    return n;
}
LZ_HD u32 lz_mismatch_summary(const LzMismatchParams& P, u64 key)
{
    const u32 pos2 = (u32)key, pos1 = pos2 + (u32)(key >> 32), L = P.X.seed_len;
    const LzMmHit H = lz_mm_hit(P, pos1, pos2, 0u);
    if (H.E > P.M) {                                            // the (M+1)-th mismatch from the right (:3522)
        u32 w = H.win;
        for (u32 k = 0; k < P.M; k++) w &= ~(0x80000000u >> __builtin_clz(w));
        return (31u - (u32)__builtin_clz(w)) - (LZ_EX_W - L);
    }
    const u32 K = P.M + 1u - H.E;
    LzMmMap lm, rm;
    if (lz_mm_map_read<false>(P, H, K, lm) < K) return LZ_SUMM_SLOW;
    if (lz_mm_map_read<true>(P, H, K, rm) < K) return LZ_SUMM_SLOW;
    const u32 first_right = lz_mm_map_low(rm);
    const u32 aK = lz_mm_map_keep(lm, K), bK = lz_mm_map_keep(rm, K);
    if (aK + L + bK >= P.X.thr) {                               // the cheap bound reaches the threshold: the K pairings themselves
        u32 best = 0;
        for (u32 i = 0; i < K; i++) {
            const u32 a = lz_mm_map_low(lm), b = lz_mm_map_high(rm);
            lz_mm_map_clear(lm, a); lz_mm_map_clear(rm, b);
            if (a + b > best) best = a + b;
        }
        if (best + L >= P.X.thr) return LZ_SUMM_SLOW;
    }
    return H.E ? (u32)__builtin_ctz(H.win) - (LZ_EX_W - L) : L + first_right;       // :3521, :3650
}

// ---- phase B
// Of a side's mismatch positions in scan order, the first "hard" one ends the list: a NUL in either sequence, or a position
// the scan does not reach (:3576, :3585-3587; :3634, :3641-3643)
LZ_HD bool lz_mm_is_nul(const LzMismatchParams& P, const LzMmHit& H, s32 q) { return P.qraw[q] == 0 || P.traw[(s64)q + H.d] == 0; }
LZ_HD bool lz_mm_hard_left(const LzMismatchParams& P, const LzMmHit& H, s32 q) { return (s64)q < H.qstop || lz_mm_is_nul(P, H, q); }
LZ_HD bool lz_mm_hard_right(const LzMismatchParams& P, const LzMmHit& H, s32 q) { return (s64)q >= H.qend || lz_mm_is_nul(P, H, q); }
// the start a hard left position stands for: the position in front of the stop, or the NUL itself (:3577, :3587, :3606)
LZ_HD s32 lz_mm_stop_start(const LzMmHit& H, s32 q) { return (s64)q < H.qstop ? (s32)(H.qstop - 1) : q; }
// Right mismatch j (from 0; `hard`: it is the list's last and a stop) against the c starts s[0..c) (nearest first) of the
// K wanted: the start its interval opens at, or -1 if the shortfall skips it (:3651-3656).  thisLength (:3657, :3679) is r - s[that].
LZ_HD int lz_mm_pair_start(u32 j, bool hard, u32 c, u32 K)
{
    const u32 sf = K - c;
    if (!hard && j < sf) return -1;
    return (int)(c - 1u - (j > sf ? j - sf : 0u));
}
// candidates compare as (thisLength, earliest first) in one key
LZ_HD u64 lz_mm_pair_key(u32 this_length, u32 j) { return ((u64)this_length << 8) | (u64)(255u - j); }
// what the extension leaves: `left` and `right` are the winner's two bounding positions, first_right the first entry of the right list
LZ_HD u32 lz_mm_finish(const LzMismatchParams& P, const LzMmHit& H, u32& dend, s32 left, s32 right, s32 first_right, LzHspRec& rec)
{
    const u32 length = (u32)(right - left - 1);                 // :3697
    const bool hsp = length >= P.X.thr;                         // :3703, :3733
    const u32 extent = hsp ? (u32)right + 1u                    // :3704
                     : H.E ? H.pos2 - LZ_EX_W + (u32)__builtin_ctz(H.win) : (u32)first_right;
    if (extent > dend) dend = extent;                           // :3708
    rec.seed_pos1 = H.pos1; rec.seed_pos2 = H.pos2;
    rec.end1 = (u32)((s64)right + H.d); rec.length = length; rec.score = (s32)length;     // :3695-3697, :3748
    return hsp ? 1u : 0u;
}
// one record of a bucket's stream in discovery order, one lane doing all of it (tests/emul; k_settle_mismatch deals the
// blocks of a SLOW record out to the lanes of a wave and the pairings likewise)
template <class Emit>
LZ_HD void lz_mismatch_settle_record(const LzMismatchParams& P, u64 rec, u32 h /*hashedDiag of the bucket*/, u32& dend, Emit&& emit)
{
    const u32 p2 = LZ_REC_POS2(rec), pay = LZ_REC_PAYLOAD(rec), L = P.X.seed_len;
    if (lz_exact_drops(dend, p2, L)) return;
    if (!LZ_REC_SLOW(rec)) { dend = lz_exact_fast_dend(dend, p2, L, pay); return; }
    const u32 pos1 = p2 + ((pay << 16) | h);
    const LzMmHit H = lz_mm_hit(P, pos1, p2, dend);
    const u32 K = P.M + 1u - H.E;
    s32 sl[LZ_MM_LIST], rl[LZ_MM_LIST];
    u32 n = 0;
    for (u32 b = 0; n < K; b++) {
        u32 w = lz_mm_block_left(P, H, b);
        const s32 base = (s32)((s64)p2 - (s64)L - (s64)LZ_EX_W * (s64)b) - 1;
        for (; w && n < K; w &= w - 1u) sl[n++] = base - (s32)__builtin_ctz(w);
    }
    u32 c = K;
    for (u32 j = 0; j < K; j++) if (lz_mm_hard_left(P, H, sl[j])) { sl[j] = lz_mm_stop_start(H, sl[j]); c = j + 1u; break; }
    n = 0;
    for (u32 b = 0; n < K; b++) {
        u32 w = lz_mm_block_right(P, H, b);
        const s32 base = (s32)((s64)p2 + (s64)LZ_EX_W * (s64)b);
        for (; w && n < K; w &= w - 1u) rl[n++] = base + (s32)__builtin_ctz(w);
    }
    u32 nr = K; bool stop = false;
    for (u32 j = 0; j < K; j++) if (lz_mm_hard_right(P, H, rl[j])) { nr = j + 1u; stop = true; break; }
    u64 best = 0; s32 left = 0, right = 0;
    for (u32 j = 0; j < nr; j++) {
        const int at = lz_mm_pair_start(j, stop && j + 1u == nr, c, K);
        if (at < 0) continue;
        const u64 key = lz_mm_pair_key((u32)(rl[j] - sl[at]), j);
        if (key > best) { best = key; left = sl[at]; right = rl[j]; }
    }
    LzHspRec o;
    if (lz_mm_finish(P, H, dend, left, right, rl[0], o)) emit(o);
}
