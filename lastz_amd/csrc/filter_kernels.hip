// filter_kernels.hip -- the seed-hit filter of lastz --filter (lz_filter.hpp) on the two-kernel path, between k_fill_hits and
// whatever phase A follows it (k_scan_hits, k_scan_exact, k_scan_mismatch, the plain-hit copy):
//   k_fill_hits -> k_filter_mark -> scan of the block counts -> k_filter_move -> phase A on the surviving keys
// A stable compaction of the chunk's keys, which stand in discovery order.  Everything downstream -- partition bytes,
// summaries, records -- is derived from the keys, and diagEnd is not touched: the rest of the chunk runs on n_kept keys as it
// would on a chunk that had held only those.
//   k_filter_mark   one lane per key (four keys per lane and block): the predicate on the match codes of both sequences; every
//                   wave ballots one 64-bit keep word per 64 keys, every block writes its survivor count
//   rocPRIM         exclusive scan of the block counts (one entry more than there are blocks: the last base is the total)
//   k_filter_move   one block's keys per block: a survivor's rank is the block's base + the popcounts of the keep words before
//                   its own + the set bits below its own; it is stored at that rank in a SECOND key buffer.  Not in place: a
//                   block's destination range may overlap the source range of an earlier block that has not read yet.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <algorithm>
#include "lz_ctx.hpp"
#include "lz_seed_dev.hpp"
#include "lz_filter.hpp"

#define LZ_FL_TPB    256
#define LZ_FL_ROUNDS 4u
#define LZ_FL_BLOCK  (LZ_FL_TPB * LZ_FL_ROUNDS)      // keys per block
#define LZ_FL_WORDS  (LZ_FL_BLOCK / 64u)             // keep words per block

// keys [1024 b, 1024 b + 1024) of block b: word r * 4 + w of the block is wave w's round r, so that the words follow the keys
__global__ void __launch_bounds__(LZ_FL_TPB)
k_filter_mark(LzFilterParams F, const u64* __restrict__ keys, u32 n, u64* __restrict__ keep, u32* __restrict__ counts)
{
    __shared__ u32 wsum[LZ_FL_TPB / 64];
    const u32 tid = threadIdx.x, lane = tid & 63u;
    const u32 base = blockIdx.x * LZ_FL_BLOCK;
    u64 kk[LZ_FL_ROUNDS];
#pragma unroll
    for (u32 r = 0; r < LZ_FL_ROUNDS; r++) {                    // (the four gathers of a lane in flight together)
        const u32 i = base + r * LZ_FL_TPB + tid;
        kk[r] = i < n ? LZ_NT_LD(keys + i) : 0ull;
    }
    u32 kept = 0;
#pragma unroll
    for (u32 r = 0; r < LZ_FL_ROUNDS; r++) {
        const u32 i = base + r * LZ_FL_TPB + tid;
        const bool k = i < n && lz_filter_keeps_key(F, kk[r]);
        const u64 word = __ballot(k);
        if (lane == 0) { keep[i >> 6] = word; kept += (u32)__popcll(word); }     // (i - lane: the wave's first key; keep[] covers whole blocks)
    }
    if (lane == 0) wsum[tid >> 6] = kept;
    __syncthreads();
    if (tid == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ void __launch_bounds__(LZ_FL_TPB)
k_filter_move(const u64* __restrict__ keys, u32 n, const u64* __restrict__ keep, const u32* __restrict__ bases, u64* __restrict__ out)
{
    __shared__ u32 before[LZ_FL_WORDS];                         // survivors of the block ahead of each keep word
    __shared__ u64 words[LZ_FL_WORDS];
    const u32 tid = threadIdx.x, lane = tid & 63u;
    const u32 base = blockIdx.x * LZ_FL_BLOCK;
    if (tid < LZ_FL_WORDS) words[tid] = keep[(base >> 6) + tid];
    __syncthreads();
    if (tid < LZ_FL_WORDS) { u32 a = 0; for (u32 k = 0; k < tid; k++) a += (u32)__popcll(words[k]); before[tid] = a; }
    __syncthreads();
    const u32 first = bases[blockIdx.x];
#pragma unroll
    for (u32 r = 0; r < LZ_FL_ROUNDS; r++) {
        const u32 i = base + r * LZ_FL_TPB + tid;
        const u32 wi = (r * LZ_FL_TPB + tid) >> 6;
        const u64 word = words[wi];
        if (i < n && ((word >> lane) & 1ull))
            LZ_NT_ST(LZ_NT_LD(keys + i), out + first + before[wi] + (u32)__popcll(word & ((1ull << lane) - 1ull)));
    }
}

// what lzk_filter_hits needs beside c.keys for a chunk of max_n hits: the second key buffer, the keep words, the block counts and bases
int lzk_filter_reserve(LzCtx& c, u64 max_n)
{
    const size_t nblocks = (size_t)((max_n + LZ_FL_BLOCK - 1) / LZ_FL_BLOCK);
    int rc;
    if ((rc = c.keys2.ensure((size_t)max_n * 8))) return rc;
    if ((rc = c.filter_keep.ensure(nblocks * LZ_FL_WORDS * 8))) return rc;
    if ((rc = c.filter_counts.ensure((nblocks + 1) * 4))) return rc;
    return c.filter_bases.ensure((nblocks + 1) * 4);
}

// the n hits in c.keys -> those the filter keeps, in order, in c.keys (the two key buffers change places); *n_kept their number.
// Synchronises c.stream.
int lzk_filter_hits(LzCtx& c, const LzFilterParams& F, u64 n, u64* n_kept)
{
    *n_kept = 0;
    if (n == 0) return 0;
    if (n > (1ull << 31)) return LZGPU_ERR_ARG;                 // (hit indices inside a chunk are 32-bit)
    const u32 nblocks = (u32)((n + LZ_FL_BLOCK - 1) / LZ_FL_BLOCK);
    if (!c.keys2.p || c.keys2.cap < (size_t)n * 8 || c.filter_keep.cap < (size_t)nblocks * LZ_FL_WORDS * 8 ||
        c.filter_counts.cap < ((size_t)nblocks + 1) * 4 || c.filter_bases.cap < ((size_t)nblocks + 1) * 4) return LZGPU_ERR_ARG;
    u32* const counts = c.filter_counts.as<u32>(); u32* const bases = c.filter_bases.as<u32>();
    LZ_HIP(hipMemsetAsync(counts + nblocks, 0, 4, c.stream));
    c.timer.begin("k_filter_mark", c.stream);
    hipLaunchKernelGGL(k_filter_mark, dim3(nblocks), dim3(LZ_FL_TPB), 0, c.stream, F, c.keys.as<u64>(), (u32)n, c.filter_keep.as<u64>(), counts);
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    size_t tmp = 0;
    LZ_HIP(rocprim::exclusive_scan(nullptr, tmp, counts, bases, 0u, (size_t)nblocks + 1, rocprim::plus<u32>(), c.stream));
    int rc = c.scan_tmp.ensure(tmp);
    if (rc) return rc;
    c.timer.begin("rocprim_scan_filter", c.stream);
    LZ_HIP(rocprim::exclusive_scan(c.scan_tmp.p, tmp, counts, bases, 0u, (size_t)nblocks + 1, rocprim::plus<u32>(), c.stream));
    c.timer.end(c.stream);
    c.timer.begin("k_filter_move", c.stream);
    hipLaunchKernelGGL(k_filter_move, dim3(nblocks), dim3(LZ_FL_TPB), 0, c.stream, c.keys.as<u64>(), (u32)n, c.filter_keep.as<u64>(), bases, c.keys2.as<u64>());
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    u32 total = 0;
    LZ_HIP(hipMemcpyAsync(&total, bases + nblocks, 4, hipMemcpyDeviceToHost, c.stream));
    LZ_HIP(hipStreamSynchronize(c.stream));
    if (total > n) return lz_fail(LZGPU_ERR_STATE, "internal: the hit filter kept %u of %llu hits", total, (unsigned long long)n);
    std::swap(c.keys, c.keys2);
    *n_kept = total;
    return 0;
}
