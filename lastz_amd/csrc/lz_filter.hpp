// lz_filter.hpp -- the seed-hit filter of `lastz --filter=[<T>,]<M>` and `--filter=cares:[<T>,]<M>`:
// filter_seed_hit_by_subs (src/seed_search.c:2346-2411), which process_for_simple_hit runs after the diagEnd test (:1113) and
// before any extension, and process_for_plain_hit (:995-1029) the same way.  A hit it rejects returns having written
// nothing, and the predicate reads nothing but the bases under the seed window: the reference's result is the result of
// the same search over the raw-hit stream with the failing hits taken out, order kept.
//
// The predicate runs on the match codes an exact-match search keeps per sequence (lz_exact.hpp: 2 bits per base, Gray
// coded, and a 1-bit "matches nothing" mask; base i at bit i + LZ_PAD2, everything outside the sequence masked).  A seed is
// at most 31 bases long, so ONE compare of 32 base pairs from (pos1 - L, pos2 - L) on covers any window: two unaligned
// 64-bit loads of the 2-bit arrays and two 32-bit loads of the masks (lz_ex_diff32's loads).
//
// The coding argument.  match_bits is nuc_to_bits: A, C, G, T = 0, 1, 2, 3, the low bit tells purine from pyrimidine, and
// is_transversion(b1, b2) is ((b1 ^ b2) & 1) == 1 (:2344).  The arrays hold g(b) = b ^ (b >> 1): 00, 01, 11, 10.  For two
// codes, g(b1) ^ g(b2) = g(b1 ^ b2) (g is linear over XOR), and b1 ^ b2 = 0, 1, 2, 3 gives 00, 01, 11, 10:
//   00          b1 == b2: a match (:2376, :2394)
//   11          b1 ^ b2 == 2, the low bits agree: a transition, which counts as neither
//   01 or 10    b1 ^ b2 is odd: a transversion (:2378, :2396)
// so "exactly one bit of the pair set" is the transversion test.  A base whose mask bit is set -- match_bits < 0 or a NUL --
// makes the pair a transversion whatever the codes say (:2374, :2392; hp->charToBits[0] is -1).
//
// The functions here are the per-lane device logic (LZ_HD: also compiled for the host by tests/emul/emul_filter.cpp).
#pragma once
#include "lz_exact.hpp"

struct LzFilterParams {
    const u8* t2; const u8* tsp;       // the target's match codes (LzExactParams)
    const u8* q2; const u8* qsp;       // the query's
    u64 pos_spread;                    // bit 2k set: base k of the window counts (lz_filter_spread of lz_hit_filter.positions, made on the host)
    u32 seed_len;
    s32 min_matches;                   // hp->minMatches
    s32 max_transversions;             // hp->maxTransversions; < 0: no limit
};

// bit k of x -> bit 2k
LZ_HD u64 lz_filter_spread(u32 x)
{
    u64 v = x;
    v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
    v = (v | (v << 8))  & 0x00FF00FF00FF00FFull;
    v = (v | (v << 4))  & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v << 2))  & 0x3333333333333333ull;
    v = (v | (v << 1))  & 0x5555555555555555ull;
    return v;
}
LZ_HD u32 lz_filter_popc64(u64 x) { return (u32)__builtin_popcountll(x); }

struct LzFilterCounts { u32 matches, transversions; };
// the counted base pairs of the window [pos - L, pos) of both sequences.  pos1 >= L, pos2 >= L; pos1 <= tlen, pos2 <= qlen
LZ_HD LzFilterCounts lz_filter_counts(const LzFilterParams& F, u32 pos1, u32 pos2)
{
    const u64 tb = (u64)(pos1 - F.seed_len) + LZ_PAD2, qb = (u64)(pos2 - F.seed_len) + LZ_PAD2;
    const u64 x = lz_ex_bits64(F.t2, 2u * tb) ^ lz_ex_bits64(F.q2, 2u * qb);
    const u64 nothing = lz_filter_spread(lz_ex_bits32(F.tsp, tb) | lz_ex_bits32(F.qsp, qb)) & F.pos_spread;
    const u64 one  = (x ^ (x >> 1)) & F.pos_spread;            // exactly one bit of the pair set
    const u64 none = ~(x | (x >> 1)) & F.pos_spread;           // neither
    LzFilterCounts c;
    c.matches = lz_filter_popc64(none & ~nothing);
    c.transversions = lz_filter_popc64(one | nothing);
    return c;
}
// true: the hit is kept (:2403-2410)
LZ_HD bool lz_filter_keeps(const LzFilterParams& F, u32 pos1, u32 pos2)
{
    const LzFilterCounts c = lz_filter_counts(F, pos1, pos2);
    return (s32)c.matches >= F.min_matches && (F.max_transversions < 0 || (s32)c.transversions <= F.max_transversions);
}
LZ_HD bool lz_filter_keeps_key(const LzFilterParams& F, u64 key)
{
    const u32 pos2 = (u32)key;
    return lz_filter_keeps(F, pos2 + (u32)(key >> 32), pos2);
}
