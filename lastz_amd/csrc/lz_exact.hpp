// lz_exact.hpp -- the seed stage of `lastz --exact=<length>`: process_for_simple_hit with gfExtend == gfexExact
// (src/seed_search.c:1056-1192) and match_extend_seed_hit (:3018-3254), decomposed the way lz_lut.hpp decomposes the X-drop
// extension: phase A looks at every raw hit on its own, phase B walks a bucket's hits in discovery order with diagEnd.
//
// Two bases match iff charToBits[t] == charToBits[q] >= 0 (:3068-3077, 3117-3127, 3154-3164) with hp->charToBits, which
// is nuc_to_bits: lower case matches upper case; N, IUPAC codes and NUL match nothing, not even themselves.  Both
// sequences are held once more as "match codes": 2 bits per base and a 1-bit "matches nothing" mask, in the layout of
// lz_lut.hpp's arrays (base i at bit i + LZ_PAD2; everything outside the sequence is masked), so that a run ends at
// either end of either sequence with no test of its own.  Thirty-two bases compare as the XOR of two unaligned 64-bit
// loads of the 2-bit arrays and the OR of 32 bits of both masks; the run is a count of trailing or leading zeros.
//
// Why phase A is exact.  For the raw hit (pos1, pos2) of a seed of length L on diagonal d = pos1 - pos2, with
// E = diagEnd[hashedDiag] when the hit's turn comes:
//   * E > pos2 - L: the hit is dropped (:1113) and nothing is written.
//   * Otherwise the window is checked right to left (:3066-3078).  A mismatch at query position m yields no HSP and
//     diagEnd = max(E, m) (:3230-3249).  Neither the test nor m depends on E.
//   * Otherwise the hit is extended left down to query position E at most (:3094-3129), and right to the first
//     mismatch (:3152-3165).  With l the UNCLIPPED left run (to the first mismatch or the start of a sequence) and r the
//     right run, the reference's length is min(l, pos2 - L - E) + L + r, the extent it writes is pos2 + r (:3175-3178),
//     and the hit is an HSP iff length >= (unsigned) hspThreshold (:3209).  r and the extent do not depend on E, and the
//     length is at most l + L + r: when that is below the threshold the hit is no HSP whatever E is.
// So a hit whose window is not an exact match, or whose two unclipped runs both end below the cap LZ_EX_CAP with
// l + L + r < threshold, is FAST: beyond the drop test its whole effect is diagEnd = max(diagEnd, extent), and the extent
// travels in the record's 16 payload bits as extent - (pos2 - L) (at most L + LZ_EX_CAP).  Every other hit -- it could reach
// the threshold, or a run reached the cap -- is SLOW and is extended again in phase B with the bucket's real diagEnd.
//
// The functions here are the per-lane device logic (LZ_HD: also compiled for the host by tests/emul/emul_exact.cpp).
#pragma once
#include "lz_lut.hpp"

#define LZ_EX_W    32u                 // bases per compare
#define LZ_EX_CAP  128u                // phase A measures each run up to this many bases (a multiple of LZ_EX_W)

struct LzExactParams {
    const u8* t2; const u8* tsp;       // the target's match codes: 2-bit codes, "matches nothing" mask (layout: lz_lut.hpp, LzLutParams)
    const u8* q2; const u8* qsp;       // the query's
    u32 tlen, qlen;
    u32 seed_len;
    u32 thr;                           // (unsigned) hspThreshold.s, as :3209 compares it
};

// the class table of the match codes for k_encode: byte b -> bits << 5, or LZ_CODE_INVALID when it matches nothing
// (a NUL matches nothing whatever the table says: :3122-3123, :3159-3160)
LZ_HD void lz_exact_cls(const int8_t match_bits[256], u8 cls[256])
{
    for (int b = 0; b < 256; b++) cls[b] = (b == 0 || match_bits[b] < 0) ? (u8)LZ_CODE_INVALID : (u8)((match_bits[b] & 3) << 5);
}

// 64 bits of a[] from bit `bit` on (reads 9 bytes), and 32 bits (reads 8)
LZ_HD u64 lz_ex_bits64(const u8* a, u64 bit)
{
    const u8* p = a + (bit >> 3);
    const u32 sh = (u32)bit & 7u;
    u64 lo; __builtin_memcpy(&lo, p, 8);
    const u64 hi = p[8];
    return sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
}
LZ_HD u32 lz_ex_bits32(const u8* a, u64 bit)
{
    u64 lo; __builtin_memcpy(&lo, a + (bit >> 3), 8);
    return (u32)(lo >> ((u32)bit & 7u));
}
// the 32 base pairs (t + k, q + k), k = 0..31: d has bit 2k set where the 2-bit codes differ, m bit k where either base
// matches nothing.  t, q >= -LZ_EX_W; t <= tlen, q <= qlen (the arrays' padding covers the overhang).
LZ_HD void lz_ex_diff32(const LzExactParams& P, s64 t, s64 q, u64& d, u32& m)
{
    const u64 tb = (u64)(t + LZ_PAD2), qb = (u64)(q + LZ_PAD2);
    const u64 x = lz_ex_bits64(P.t2, 2u * tb) ^ lz_ex_bits64(P.q2, 2u * qb);
    d = (x | (x >> 1)) & 0x5555555555555555ull;
    m = lz_ex_bits32(P.tsp, tb) | lz_ex_bits32(P.qsp, qb);
}
// matching base pairs (t, q), (t + 1, q + 1), ...: 32 at most
LZ_HD u32 lz_ex_run_right32(const LzExactParams& P, s64 t, s64 q)
{
    u64 d; u32 m;
    lz_ex_diff32(P, t, q, d, m);
    const u32 rd = d ? lz_ctz64(d) >> 1 : LZ_EX_W, rm = m ? (u32)__builtin_ctz(m) : LZ_EX_W;
    return rd < rm ? rd : rm;
}
// matching base pairs (t - 1, q - 1), (t - 2, q - 2), ...: 32 at most.  t, q >= 0
LZ_HD u32 lz_ex_run_left32(const LzExactParams& P, s64 t, s64 q)
{
    u64 d; u32 m;
    lz_ex_diff32(P, t - (s64)LZ_EX_W, q - (s64)LZ_EX_W, d, m);
    const u32 rd = d ? lz_clz64(d) >> 1 : LZ_EX_W, rm = m ? (u32)__builtin_clz(m) : LZ_EX_W;
    return rd < rm ? rd : rm;
}

// ---- phase A: the 4-byte summary of one raw hit (the form lz_hit_record packs: low 16 bits = payload of a fast
// hit, LZ_SUMM_SLOW).  `back` = the matching run to the left of the hit's END, the window included (:3066-3078 and
// :3112-3128 walk the same bases one after the other), measured in whole compares up to LZ_EX_BACK_CAP: below that it is
// known exactly, and with it the left run back - L; at it the left run is LZ_EX_CAP or more (L <= 31 < LZ_EX_W).
#define LZ_EX_BACK_CAP (LZ_EX_CAP + LZ_EX_W)
struct LzExactRuns { u32 back, right; };
LZ_HD LzExactRuns lz_exact_runs(const LzExactParams& P, u32 pos1, u32 pos2)
{
    LzExactRuns r;
    r.back = lz_ex_run_left32(P, (s64)pos1, (s64)pos2);
    if (r.back >= P.seed_len) {                                  // (a run of k whole compares goes on: the bases before it exist)
        for (u32 k = 1; r.back == k * LZ_EX_W && r.back < LZ_EX_BACK_CAP; k++) r.back += lz_ex_run_left32(P, (s64)pos1 - k * LZ_EX_W, (s64)pos2 - k * LZ_EX_W);
    }
    r.right = 0;
    if (r.back >= P.seed_len) {
        r.right = lz_ex_run_right32(P, (s64)pos1, (s64)pos2);
        for (u32 k = 1; r.right == k * LZ_EX_W && r.right < LZ_EX_CAP; k++) r.right += lz_ex_run_right32(P, (s64)pos1 + k * LZ_EX_W, (s64)pos2 + k * LZ_EX_W);
    }
    return r;
}
LZ_HD u32 lz_exact_summary(const LzExactParams& P, u64 key)
{
    const u32 pos2 = (u32)key, pos1 = pos2 + (u32)(key >> 32), L = P.seed_len;
    const LzExactRuns r = lz_exact_runs(P, pos1, pos2);
    if (r.back < L) return L - 1u - r.back;                     // the window's rightmost mismatch m = pos2 - 1 - back (:3075)
    const bool capped = r.back == LZ_EX_BACK_CAP || r.right == LZ_EX_CAP;
    if (capped || r.back + r.right >= P.thr) return LZ_SUMM_SLOW;
    return L + r.right;                                         // the right end pos2 + right (:3175)
}

// ---- phase B
// the drop test (:1113) and a fast record's whole effect
LZ_HD bool lz_exact_drops(u32 dend, u32 pos2, u32 L) { return dend > pos2 - L; }
LZ_HD u32 lz_exact_fast_dend(u32 dend, u32 pos2, u32 L, u32 payload) { const u32 e = pos2 - L + payload; return e > dend ? e : dend; }
// A SLOW record's extension in blocks of 32 bases that any number of lanes may take side by side: block b of the right
// run is the pairs from (pos1 + 32 b, pos2 + 32 b) on; block b of the left run those before (pos1 - L - 32 b, pos2 - L - 32 b),
// of which only `room` = pos2 - L - diagEnd count (:3094-3098).  A block returns its matching run; the whole run is
// 32 b + that of the first block b that returns less than 32.  A block beyond an end of a sequence (or beyond the room)
// returns 0 without a load.
LZ_HD u32 lz_exact_block_right(const LzExactParams& P, u32 pos1, u32 pos2, u32 b)
{
    const u64 off = (u64)b * LZ_EX_W;
    if ((u64)pos1 + off >= P.tlen || (u64)pos2 + off >= P.qlen) return 0;
    return lz_ex_run_right32(P, (s64)((u64)pos1 + off), (s64)((u64)pos2 + off));
}
LZ_HD u32 lz_exact_block_left(const LzExactParams& P, u32 pos1, u32 pos2, u32 room, u32 b)
{
    const u64 off = (u64)b * LZ_EX_W;
    const u32 e1 = pos1 - P.seed_len, e2 = pos2 - P.seed_len;
    if (off >= room || off >= e1 || off >= e2) return 0;
    return lz_ex_run_left32(P, (s64)e1 - (s64)off, (s64)e2 - (s64)off);
}
// what the extension leaves: left = the unclipped left run (or anything >= room), right = the right run
LZ_HD u32 lz_exact_finish(const LzExactParams& P, u32 pos1, u32 pos2, u32& dend, u32 left, u32 right, LzHspRec& rec)
{
    const u32 room = pos2 - P.seed_len - dend;
    if (left > room) left = room;
    const u32 extent = pos2 + right;                            // :3175
    if (extent > dend) dend = extent;
    rec.seed_pos1 = pos1; rec.seed_pos2 = pos2;
    rec.end1 = pos1 + right; rec.length = left + P.seed_len + right; rec.score = (s32)rec.length;   // :3197-3199, :3224
    return rec.length >= P.thr ? 1u : 0u;                       // :3209
}
// one record of a bucket's stream in discovery order, one lane doing all of it (tests/emul; k_settle_exact deals the
// blocks of a SLOW record out to the lanes of a wave)
template <class Emit>
LZ_HD void lz_exact_settle_record(const LzExactParams& P, u64 rec, u32 h /*hashedDiag of the bucket*/, u32& dend, Emit&& emit)
{
    const u32 p2 = LZ_REC_POS2(rec), pay = LZ_REC_PAYLOAD(rec);
    if (lz_exact_drops(dend, p2, P.seed_len)) return;
    if (!LZ_REC_SLOW(rec)) { dend = lz_exact_fast_dend(dend, p2, P.seed_len, pay); return; }
    const u32 pos1 = p2 + ((pay << 16) | h);
    const u32 room = p2 - P.seed_len - dend;
    u32 right = 0, left = 0, b = 0, r;
    do { r = lz_exact_block_right(P, pos1, p2, b++); right += r; } while (r == LZ_EX_W);
    b = 0;
    do { r = lz_exact_block_left(P, pos1, p2, room, b++); left += r; } while (r == LZ_EX_W);
    LzHspRec o;
    if (lz_exact_finish(P, pos1, p2, dend, left, right, o)) emit(o);
}
