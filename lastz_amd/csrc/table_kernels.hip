// table_kernels.hip -- gfx950 kernels of the position table (the table whose lists rows 1-2 probe;
// k_build_wctx of row 2 + 4 of the fused form): build by one radix sort, export in the reference's last[] / prev[] form,
// and the context-inlined copy the fused scan reads.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include "lz_ctx.hpp"
#include "lz_lut.hpp"
#include "lz_seed_dev.hpp"

// ------------------------------------------------------------------------------------------
// B1: position table.  One (word, end position) pair per target position, positions emitted in
// DESCENDING order so that the stable radix sort by word leaves every word's list in the order
// the reference's chain walk yields it (most recent first, src/pos_table.c:1341-1344).
__global__ void __launch_bounds__(LZ_TPB)
k_table_words(const u8* __restrict__ tcode, u32 start, u32 end, u32 step, LzSeedDev sd,
              u32* __restrict__ keys, u32* __restrict__ vals, u32 n)
{
    u32 j = blockIdx.x * LZ_TPB + threadIdx.x;
    if (j >= n) return;
    u32 p = end - j;                                    // window is [p-L, p)
    u32 key = 1u << sd.weight;                          // "no word": sorts after every real word
    if (p >= start + (u32)sd.length && (p % step) == 0) {
        u32 packed;
        if (lz_window_word(tcode, p, sd, packed)) key = packed;
    }
    keys[j] = key; vals[j] = p;
}

// wstart[w] = index of the first sorted entry with key >= w, for w in [0, nwords]
__global__ void __launch_bounds__(LZ_TPB)
k_key_bounds_u32(const u32* __restrict__ keys, u32 n, u32 nwords, u32* __restrict__ wstart)
{
    u32 i = blockIdx.x * LZ_TPB + threadIdx.x;
    if (i > n) return;
    s64 kp = (i == 0) ? -1 : (s64)keys[i - 1];
    s64 k  = (i == n) ? (s64)nwords : (s64)keys[i];
    if (k > (s64)nwords) k = nwords;
    if (kp > (s64)nwords) kp = nwords;
    for (s64 w = kp + 1; w <= k; w++) wstart[w] = i;
}

int lzk_table_build(LzCtx& c)
{
    const lz_table_geom& g = c.geom;
    const u32 n = g.end - g.start;
    const u32 nwords = 1u << c.seed.weight;
    int rc;
    if ((rc = c.tb_keys.ensure((size_t)n * 4))) return rc;
    if ((rc = c.tb_vals.ensure((size_t)n * 4))) return rc;
    if ((rc = c.tb_keys2.ensure((size_t)n * 4))) return rc;
    if ((rc = c.tb_vals2.ensure((size_t)n * 4))) return rc;
    if ((rc = c.wstart.ensure(((size_t)nwords + 1) * 4))) return rc;

    c.timer.begin("k_table_words", c.stream);
    hipLaunchKernelGGL(k_table_words, dim3((n + LZ_TPB - 1) / LZ_TPB), dim3(LZ_TPB), 0, c.stream,
                       c.target.code_base(), g.start, g.end, g.step, c.seed,
                       c.tb_keys.as<u32>(), c.tb_vals.as<u32>(), n);
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());

    size_t tmp = 0;
    LZ_HIP(rocprim::radix_sort_pairs(nullptr, tmp, c.tb_keys.as<u32>(), c.tb_keys2.as<u32>(),
                                     c.tb_vals.as<u32>(), c.tb_vals2.as<u32>(), (size_t)n, 0u,
                                     (unsigned)c.seed.weight + 1u, c.stream));
    if ((rc = c.sort_tmp.ensure(tmp))) return rc;
    c.timer.begin("rocprim_sort_table", c.stream);
    LZ_HIP(rocprim::radix_sort_pairs(c.sort_tmp.p, tmp, c.tb_keys.as<u32>(), c.tb_keys2.as<u32>(),
                                     c.tb_vals.as<u32>(), c.tb_vals2.as<u32>(), (size_t)n, 0u,
                                     (unsigned)c.seed.weight + 1u, c.stream));
    c.timer.end(c.stream);

    c.timer.begin("k_key_bounds_u32", c.stream);
    hipLaunchKernelGGL(k_key_bounds_u32, dim3((n + 1 + LZ_TPB - 1) / LZ_TPB), dim3(LZ_TPB), 0, c.stream,
                       c.tb_keys2.as<u32>(), n, nwords, c.wstart.as<u32>());
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());

    u32 nw = 0;
    LZ_HIP(hipMemcpyAsync(&nw, c.wstart.as<u32>() + nwords, 4, hipMemcpyDeviceToHost, c.stream));
    LZ_HIP(hipStreamSynchronize(c.stream));
    c.timer.resolve();
    c.num_words = nw;
    c.table_gen++;                                       // (wctx follows wpos: lzk_wctx_build)
    if ((rc = c.wpos.ensure((size_t)(nw ? nw : 1) * 4))) return rc;
    LZ_HIP(hipMemcpyAsync(c.wpos.p, c.tb_vals2.p, (size_t)nw * 4, hipMemcpyDeviceToDevice, c.stream));
    LZ_HIP(hipStreamSynchronize(c.stream));
    return 0;                                            // scratch stays allocated for the next rebuild
}

// CSR -> the reference's last[]/prev[] (src/pos_table.h:126-165): one thread per word
__global__ void __launch_bounds__(LZ_TPB)
k_table_export(const u32* __restrict__ wstart, const u32* __restrict__ wpos, u32 nwords,
               u32 adj_start, u32 step, u32* __restrict__ last, u32* __restrict__ prev)
{
    u32 w = blockIdx.x * LZ_TPB + threadIdx.x;
    if (w >= nwords) return;
    u32 a = wstart[w], b = wstart[w + 1];
    if (a == b) return;
    if (last) last[w] = (wpos[a] - adj_start) / step;
    if (prev)
        for (u32 j = a; j < b; j++)
            prev[(wpos[j] - adj_start) / step] = (j + 1 < b) ? (wpos[j + 1] - adj_start) / step : 0xFFFFFFFFu;
}

int lzk_table_export(LzCtx& c, u32* last_dev, u32* prev_dev, u32 prev_entries)
{
    const u32 nwords = 1u << c.seed.weight;
    if (last_dev) LZ_HIP(hipMemsetAsync(last_dev, 0, (size_t)nwords * 4, c.stream));
    if (prev_dev) LZ_HIP(hipMemsetAsync(prev_dev, 0, (size_t)prev_entries * 4, c.stream));
    u32 adj = c.geom.start - (c.geom.start % c.geom.step);
    hipLaunchKernelGGL(k_table_export, dim3((nwords + LZ_TPB - 1) / LZ_TPB), dim3(LZ_TPB), 0, c.stream,
                       c.built_wstart().as<u32>(), c.built_wpos().as<u32>(), nwords, adj, c.geom.step, last_dev, prev_dev);   // (not a limited copy)
    LZ_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------
// The table context of the fused path (scan_kernels.hip, k_scan_hits2): wctx[e] = the 32 bytes of the target's 2-bit array
// that hold both first windows of pos1 = wpos[e] (lz_lut.hpp, lz_wctx_make).  k_scan_hits gathers one random 64-byte line per
// hit for these; here they sit beside the table entry and are read where k_fill_hits2 reads wpos[] -- in ascending runs, one
// per list.
__global__ void __launch_bounds__(LZ_TPB)
k_build_wctx(const u32* __restrict__ wpos, u64 num_words, const u8* __restrict__ two, LzVec16* __restrict__ wctx)
{
    const u64 j = (u64)blockIdx.x * LZ_TPB + threadIdx.x;       // one 16-byte half of an entry per lane
    if (j >= 2 * num_words) return;
    const u32 pos1 = wpos[j >> 1];
    wctx[j] = lz_load16(two + lz_wctx_first_byte(pos1) + 16u * (u32)(j & 1u));
}

int lzk_wctx_build(LzCtx& c)
{
    const u64 nw = c.num_words;
    if (nw == 0) return 0;
    c.timer.begin("k_build_wctx", c.stream);
    hipLaunchKernelGGL(k_build_wctx, dim3((unsigned)((2 * nw + LZ_TPB - 1) / LZ_TPB)), dim3(LZ_TPB), 0, c.stream,
                       c.wpos.as<u32>(), nw, c.target.two.as<u8>(), c.wctx.as<LzVec16>());
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    return 0;
}
