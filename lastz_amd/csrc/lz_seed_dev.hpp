// lz_seed_dev.hpp -- what more than one of the seed stage's translation units needs on the device side (seq_kernels.hip,
// table_kernels.hip, enum_kernels.hip, scan_kernels.hip, settle_kernels.hip).  Everything else lives beside its kernel.
//
// Decomposition: the only cross-hit state of the reference's HSP search is
// diagEnd[hashedDiag] (src/seed_search.c:1081-1126, 2612-2616, 2785-2789), so the exact
// parallel form is 65,536 independent, order-preserving streams.  Hits are enumerated in the
// reference's order (count -> scan -> fill gives every hit its discovery index; the table itself
// is probed in seed-word order: enum_kernels.hip), scanned independently of the hash (phase A, k_scan_hits: four bases per
// look-up in an LDS table on 2-bit codes, lz_lut.hpp: scan_kernels.hip), stably partitioned by the high 8 hash bits
// (k_partition), and each partition is then dealt out to its 256 buckets inside LDS, every bucket walked by
// one lane with diagEnd[h] in a register (phase B, k_settle2: settle_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include "lz_ctx.hpp"

#define LZ_TPB 256

// The per-hit streams of the stage -- keys, partition bytes, summaries, records: written once by one kernel, read once by the
// next, 8-21 bytes per hit and 4-62 G hits per step -- are stored and loaded NON-TEMPORALLY, so that they pass through L2 and the
// 256 MiB memory-side cache without pushing out what IS re-read: the position table's lists, the target's and the query's 2-bit
// windows.  Measured (same box, A/B against plain loads and stores): at 200 Mbp x 200 Mbp fill 360 -> 318, scans 1260 -> 1253, tasks 87 -> 80 ms
// per step (-2.1 % of the step); on the 50 Mbp pair -1 ms.  k_partition keeps plain accesses: with non-temporal ones it ran
// 10-15 % slower (its 512-byte runs per partition want to merge in L2).
#define LZ_NT_LD(p_) __builtin_nontemporal_load(p_)
#define LZ_NT_ST(v_, p_) __builtin_nontemporal_store((v_), (p_))

#define LZ_KEY_BIN(k)  ((u32)((k) >> 40) & 0xFFu)    // the partition of a hit: bits 8..15 of hashedDiag (k_scan_hits, k_partition)

// a wave's lists of k_fill_hits2 / k_scan_hits2 (enum_kernels.hip, scan_kernels.hip)
template <int CAP> struct LzListWave {               // CAP: hits per piece of a wave's concatenation
    static_assert(CAP % 512 == 0, "whole 16-byte groups of own[] per lane");
    alignas(16) u32 own32[CAP / 2];                  // own[]: u16 list ids (1 + lane * 16 + probe), 0 = no list starts here
    u32 lsrc[64 * LZ_FILL_GROUP];                    // list -> (first wpos index - start of the list in the concatenation)
    uint2 ent[64];                                   // entry -> (place of its run in the key array - start of the run, pos2)
};
template <int CTRL, int ROWM, int BANKM>
__device__ __forceinline__ u32 lz_dpp_u32(u32 ident, u32 src) { return (u32)__builtin_amdgcn_update_dpp((int)ident, (int)src, CTRL, ROWM, BANKM, false); }
// inclusive wave scans (the classic row_shr 1,2,3 / 4 / 8 / row_bcast 15 / 31 sequence; unreached lanes get the identity)
#define LZ_WAVE_SCAN_U32(v, x, OP)                                     \
    v = OP(lz_dpp_u32<0x111, 0xf, 0xf>(0u, x), v);                     \
    v = OP(lz_dpp_u32<0x112, 0xf, 0xf>(0u, x), v);                     \
    v = OP(lz_dpp_u32<0x113, 0xf, 0xf>(0u, x), v);                     \
    v = OP(lz_dpp_u32<0x114, 0xf, 0xe>(0u, v), v);                     \
    v = OP(lz_dpp_u32<0x118, 0xf, 0xc>(0u, v), v);                     \
    v = OP(lz_dpp_u32<0x142, 0xa, 0xf>(0u, v), v);                     \
    v = OP(lz_dpp_u32<0x143, 0xc, 0xf>(0u, v), v);
__device__ __forceinline__ u32 lz_uadd(u32 a, u32 b) { return a + b; }
__device__ __forceinline__ u32 lz_umax(u32 a, u32 b) { return a > b ? a : b; }

// (host) the chunk's positions [i0, i1) lie in blocks i0 >> shift .. (i1 - 1) >> shift: a contiguous range of the sorted list
static inline void lz_chunk_range(const LzCtx& c, u32 i0, u32 i1, const u32*& sk, const u32*& sv, u32& n)
{
    if (c.blk_start_host.empty()) return;
    const u32 b0 = i0 >> c.blk_shift, b1 = (i1 - 1) >> c.blk_shift;
    const u64 j0 = c.blk_start_host[b0], j1 = c.blk_start_host[std::min<u32>(b1 + 1, c.blk_count)];
    sk += j0; sv += j0; n = (u32)(j1 - j0);
}
