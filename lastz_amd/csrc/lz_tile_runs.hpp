// lz_tile_runs.hpp -- where a partition's records lie once every tile of hits has been sorted by partition in place.
//
// k_partition / k_partition2 sort tile t (the hits [t * LZ_PP_TILE, t * LZ_PP_TILE + tile_n) of a chunk, discovery
// order) by partition where it lies and leave two tables, both [tile][partition]:
//   hist[t][p]      records of partition p in tile t; the two k_hist_scan kernels turn it (with part[t >> 8][p]) into
//                   the partition-major rank of the run's first record: first(t, p) = part[t >> 8][p] + hist[t][p]
//   run_addr[t][p]  index of the run's first record in the record array: t * LZ_PP_TILE + records of lower partitions
// Partition p is then the concatenation of its runs, tiles ascending: rank g (bin_base[p] <= g < bin_base[p + 1]) lies in
// the run of the largest tile t with first(t, p) <= g that holds a record of p, at run_addr[t][p] + (g - first(t, p)).
//
// k_settle2's sorter waves gather 64 x LZ_S2_ROUNDS consecutive ranks at a time (a "window") through a cursor that only
// moves forward: a block of LZ_TR_BLOCK consecutive tiles' (first, run_addr), LZ_TR_K per lane, whose last entry only
// bounds the block (ranks below its `first` are covered).  The functions here are that arithmetic, per entry and per
// rank (LZ_HD: also compiled for the host by tests/emul/emul_tile_runs.cpp and emul_tile_cursor.cpp, which replay the
// wave's procedure: the first with a mark per run and a running maximum over the window, as k_settle2 did it until the
// entry cursor below, the second with that cursor).
#pragma once
#include "lz_common.hpp"

#ifndef LZ_PP_TILE_HOST
#define LZ_PP_TILE_HOST 16384       // hits per tile of k_partition (sizes the tile tables); 8192 with 512 lanes: 24.5 ms per step, 16384 with 1024: 21.7
#endif
#define LZ_TR_NBIN  256             // partitions
#define LZ_TR_K     2               // block entries per lane
#define LZ_TR_BLOCK (64 * LZ_TR_K)  // entries of a cursor block; it covers LZ_TR_BLOCK - 1 tiles and moves by as many

// partition-major rank of the first record of tile t's run of partition p (end: the partition's end, for tiles past the last)
LZ_HD u32 lz_tr_first(const u32* hist, const u32* part, u32 ntiles, u32 t, u32 p, u32 end)
{
    return t < ntiles ? part[(size_t)(t >> 8) * LZ_TR_NBIN + p] + hist[(size_t)t * LZ_TR_NBIN + p] : end;
}
// what k_partition stores in run_addr[tile][p] (tstart: records of the tile in lower partitions)
LZ_HD u32 lz_tr_run_addr(u32 tile, u32 tstart) { return tile * (u32)LZ_PP_TILE_HOST + tstart; }
// the run [first, next_first) against the window [g0, g1), g0 < g1: true if it holds ranks of the window; pos = the
// window position of the first of them (runs that do have distinct positions, ascending with the tile)
LZ_HD bool lz_tr_mark(u32 first, u32 next_first, u32 g0, u32 g1, u32& pos)
{
    const u32 s = first > g0 ? first : g0;
    pos = s - g0;
    return next_first > s && first < g1;
}
// rank -> index: the run's displacement (mod 2^32: a chunk has fewer than 2^32 hits), added to any rank of the run
LZ_HD u32 lz_tr_delta(u32 run_addr, u32 first) { return run_addr - first; }
LZ_HD u32 lz_tr_index(u32 g, u32 delta) { return g + delta; }
// a block whose bounding entry has first == block_end covers the ranks [block_first, block_end)
LZ_HD bool lz_tr_block_behind(u32 block_end, u32 g0) { return block_end <= g0; }          // nothing of [g0, ..) in it: move on
LZ_HD bool lz_tr_covers(u32 g, u32 block_first, u32 block_end, u32 g1) { return g >= block_first && g < block_end && g < g1; }

// ---- the entry cursor: inside a block that is not behind the window [g0, g1), the ranks it covers are [s, lim) with
//   s = lz_tc_start(g0, block_first), lim = lz_tc_limit(g1, block_end)          (nothing if s >= lim: a block of empty runs)
// The entries' `first` ascend, so the run that holds s is entry (block entries with lz_tc_at_or_below(first, s)) - 1: of
// equal ones (empty runs) the last, and never the bounding entry, whose first = block_end > s.  From there the wave goes
// through the window in rounds of 64 ranks with one wave-uniform cursor (entry e, its displacement, first of entry e + 1):
// while lz_tc_step(next_first, round_base, lim) it moves to entry e + 1, whose displacement the lanes with
// lz_tc_take(rank, next_first) take over; the cursor carries from round to round.  first(bounding entry) = block_end >= lim
// ends it, so the bounding entry is never taken as a run.  An empty run costs one trip.
LZ_HD u32 lz_tc_start(u32 g0, u32 block_first) { return block_first > g0 ? block_first : g0; }
LZ_HD u32 lz_tc_limit(u32 g1, u32 block_end) { return block_end < g1 ? block_end : g1; }
LZ_HD bool lz_tc_at_or_below(u32 first, u32 s) { return first <= s; }
LZ_HD bool lz_tc_step(u32 next_first, u32 round_base, u32 lim) { return next_first < lim && next_first < round_base + 64u; }
LZ_HD bool lz_tc_take(u32 g, u32 next_first) { return g >= next_first; }
