// lz_mask.hpp -- dynamic masking (lastz --masking=<count>) of the position table: mask_seed_position_table /
// mask_seed_positions (src/pos_table.c:747-887) for a batch of intervals, as one pass over the CSR table.
//
// The reference removes, per interval [start, end) (origin 0, already widened by L - 1 on both sides and clamped,
// src/lastz.c:3797-3801), every entry p -- a word's END position -- with start + L <= p <= end that is in the table, keeps
// the order of what stays (remove_word, :1448-1460) and looks at no byte of the sequence to decide it: an entry that is in
// the table has a valid window.  So the pass is: a bitmap over the positions 0 .. tlen with the bit of every p of every
// interval's removal range set (k_mask_bits), a keep flag per table entry (k_mask_keep), an exclusive scan of the flags,
// and the move of the kept entries to their new places with wstart[] following (k_mask_move).
//
// The functions here are the per-lane device logic (LZ_HD: also compiled for the host by tests/emul/emul_mask.cpp).
#pragma once
#include "lz_common.hpp"

// The removal range of an interval, as first and last bit: false when the interval is shorter than L and removes nothing
// (src/pos_table.c:835).  start < end <= tlen (checked by the caller), L >= 1.
LZ_HD bool lz_mask_range(u32 start, u32 end, u32 L, u32& lo, u32& hi)
{
    if (end - start < L) return false;
    lo = start + L; hi = end;
    return true;
}

// Bitmap words the range [lo, hi] touches
LZ_HD u32 lz_mask_range_words(u32 lo, u32 hi) { return (hi >> 5) - (lo >> 5) + 1; }

// The ranges lie back to back in lane order: pre[r] = bitmap words of the ranges before r, pre[n] the total.  The range of
// lane j < pre[n]: the last r with pre[r] <= j (every range has at least one word, so pre[] is strictly increasing).
LZ_HD u32 lz_mask_range_of(const u32* pre, u32 n, u32 j)
{
    u32 a = 0, b = n;
    while (b - a > 1) { const u32 mid = (a + b) >> 1; if (pre[mid] <= j) a = mid; else b = mid; }
    return a;
}

// The bits of bitmap word `word` that belong to [lo, hi]; lo >> 5 <= word <= hi >> 5
LZ_HD u32 lz_mask_word_bits(u32 lo, u32 hi, u32 word)
{
    u32 m = 0xFFFFFFFFu;
    if (word == (lo >> 5)) m &= 0xFFFFFFFFu << (lo & 31u);
    if (word == (hi >> 5)) m &= 0xFFFFFFFFu >> (31u - (hi & 31u));
    return m;
}

// 1: the entry with end position p stays
LZ_HD u32 lz_mask_keeps(const u32* bits, u32 p) { return ((bits[p >> 5] >> (p & 31u)) & 1u) ^ 1u; }
