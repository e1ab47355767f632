// lz_enum_place.inc -- step 1 of the list enumeration of k_fill_hits2 (enum_kernels.hip) and k_scan_hits2 (scan_kernels.hip): a
// fragment of text, included inside `for (int r ...; r += LZ_FILL_GROUP)`, the loop over the probe groups of a wave's 64 entries.
// The two kernels compile these lines and those of lz_enum_owners.inc (step 2) where they stand: the text is written once and the
// machine code is what it was when each kernel had its own copy (profiles/enum_once_isa_diff.txt).  As shared __forceinline__
// functions the same lines compiled differently -- the marks of step 2 to predicated stores instead of branches, and k_scan_hits ran
// 1.5 % slower (profiles/seed_dedup_ab_series.json) -- hence inclusion, as dp_kernels_dev.inc does for the two builds of the DP kernel.
//
// The scheme.  Round 2's fill (DESIGN_HISTORY.md) laid the 64 lists of four positions end to end and let every lane search the running
// totals for the list holding its hit: 13 shuffles and two prefix sums per 64 hits, 150 VALU instructions per 64-hit trip for 16 bytes of
// useful traffic per hit.  Here a wave takes its 64 sorted entries at once, one per lane, 16 probes of them at a time:
//   1. every lane reads the CSR bounds of its position's probes and keeps the lengths (lz_enum_lists.inc); an exclusive wave scan
//      of the lanes' totals places the positions' runs end to end (entry-major, probe order inside an entry = the reference's
//      enumeration order inside a position);
//   2. every list marks the cell of its first hit in own[] (its id); a prefix maximum over own[] -- ids grow along the
//      concatenation -- leaves every cell with the id of the list that holds it: 16 marks and two passes over 128
//      bytes per lane instead of a search per hit (lz_enum_owners.inc);
//   3. lane t takes hits t, t + 64, ...: own[t] -> (list source - list start), (run's place in the output - run
//      start, pos2) from two small LDS tables -> one gather from wpos[].  This is where the kernels differ, and it stays with them.
// A wave's LDS traffic is its own (no barrier: LDS operations of one wave execute in program order); concatenations
// longer than CAP hits (repeats) are taken in pieces -- the kernel's loop over cs -- and seeds with more than 16 probes in groups of 16.
// SELF: a self-comparison or a position filter (lz_common.hpp, LzSelfDev): the lists are clipped to the hits that survive, before
// the wave scan (k_count_sorted_self counted the same); everything after that is the same code.
//
//   expects   what lz_enum_lists.inc expects, and: lane (0..63), sh (the wave's LzListWave<CAP>), dbase (place of the position's
//             first hit in the chunk's output), carry (hits of the position in the probe groups already done), pos2
//   defines   la[], len[], total (lz_enum_lists.inc); E, start of the lane's run in the wave's concatenation; T, the
//             concatenation's length (wave-uniform); and fills sh.lsrc[] and sh.ent[lane]
//   included  by k_fill_hits2 and k_scan_hits2, which go on with `for (cs = 0; cs < T; cs += CAP)` and add total to carry after it.
#include "lz_enum_lists.inc"
u32 inc = total;
LZ_WAVE_SCAN_U32(inc, total, lz_uadd)
const u32 E = inc - total;
const u32 T = (u32)__builtin_amdgcn_readlane((int)inc, 63);
{
    u32 S = E;
#pragma unroll
    for (int p = 0; p < LZ_FILL_GROUP; p++) { sh.lsrc[lane * LZ_FILL_GROUP + p] = la[p] - S; S += len[p]; }
}
sh.ent[lane] = make_uint2(dbase + carry - E, pos2);
