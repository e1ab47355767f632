// mask_kernels.hip -- gfx950 kernels of dynamic masking (lastz --masking=<count>; DESIGN.md section 1, "Dynamic masking"):
// mask_seed_position_table (src/pos_table.c:747-887) for all the intervals of one (query, strand) in one pass over the
// resident CSR table.  lz_mask.hpp has the argument and the per-lane logic.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <algorithm>
#include <utility>
#include <vector>
#include "lz_ctx.hpp"
#include "lz_seed_dev.hpp"
#include "lz_mask.hpp"

// bits[] (cleared by the caller): bit p set for every p of every range [lo[r], hi[r]].  One lane per 32-bit bitmap word of
// a range, the ranges back to back (pre[]: lz_mask_range_of), so that a workgroup serves 256 short ranges or 8192 positions
// of a long one alike.  A word that lies wholly inside its range is stored; the two end words of a range are OR-ed in
// (another range may share them).  A store racing with an OR on the same word leaves all ones either way.
__global__ void __launch_bounds__(LZ_TPB)
k_mask_bits(const u32* __restrict__ lo, const u32* __restrict__ hi, const u32* __restrict__ pre, u32 n, u32 total,
            u32* __restrict__ bits)
{
    const u32 j = blockIdx.x * LZ_TPB + threadIdx.x;
    if (j >= total) return;
    const u32 r = lz_mask_range_of(pre, n, j);
    const u32 a = lo[r], b = hi[r];
    const u32 word = (a >> 5) + (j - pre[r]);
    const u32 m = lz_mask_word_bits(a, b, word);
    if (m == 0xFFFFFFFFu) bits[word] = m; else atomicOr(&bits[word], m);
}

// keep[e] = 1 for an entry that stays, e < num_words; keep[num_words] = 0: the exclusive scan of the num_words + 1 flags
// gives every entry's new place, its last value the entries that stay
__global__ void __launch_bounds__(LZ_TPB)
k_mask_keep(const u32* __restrict__ wpos, u32 num_words, const u32* __restrict__ bits, u32 tlen, u32* __restrict__ keep)
{
    const u32 e = blockIdx.x * LZ_TPB + threadIdx.x;
    if (e > num_words) return;
    u32 k = 0;
    if (e < num_words) { const u32 p = wpos[e]; k = p <= tlen ? lz_mask_keeps(bits, p) : 1u; }   // (an entry past the bitmap is in no interval)
    keep[e] = k;
}

// The kept entries at their new places (the order inside every list is the old one), and wstart[] after them: a list
// starts where its first entry, kept or not, would have gone.  wstart[] is rewritten in place (lane w reads and writes
// wstart[w] only); npos is scratch.
__global__ void __launch_bounds__(LZ_TPB)
k_mask_move(const u32* __restrict__ wpos, const u32* __restrict__ keep, const u32* __restrict__ idx, u32 num_words,
            u32* __restrict__ wstart, u32 nwords, u32* __restrict__ npos)
{
    const u32 e = blockIdx.x * LZ_TPB + threadIdx.x;
    if (e < num_words && keep[e]) npos[idx[e]] = wpos[e];
    if (e <= nwords) wstart[e] = idx[wstart[e]];
}

int lzk_table_mask(LzCtx& c, const lz_interval* iv, u32 n, u32 tlen)
{
    const u32 L = (u32)c.seed.length;
    const u32 nwords = 1u << c.seed.weight;
    const u32 nw = (u32)c.num_words;
    std::vector<u32> host;                                       // lo[nr] | hi[nr] | pre[nr + 1]
    std::vector<u32> lo, hi, pre;
    // the removal ranges, sorted and merged where they overlap or abut (their union is what goes): disjoint ranges touch
    // at most tlen / 32 + 2 nr bitmap words in all, so the lane count fits 32 bits whatever the caller sends
    std::vector<std::pair<u32, u32>> rg;
    for (u32 k = 0; k < n; k++) {
        u32 a, b;
        if (lz_mask_range(iv[k].start, iv[k].end, L, a, b)) rg.push_back({ a, b });
    }
    std::sort(rg.begin(), rg.end());
    u32 total = 0;
    for (size_t k = 0; k < rg.size(); k++) {
        if (!hi.empty() && rg[k].first <= hi.back() + 1) { if (rg[k].second > hi.back()) hi.back() = rg[k].second; continue; }
        lo.push_back(rg[k].first); hi.push_back(rg[k].second);
    }
    for (size_t r = 0; r < lo.size(); r++) { pre.push_back(total); total += lz_mask_range_words(lo[r], hi[r]); }
    const u32 nr = (u32)lo.size();
    if (nr == 0 || nw == 0) return 0;
    pre.push_back(total);
    host.reserve(3 * (size_t)nr + 1);
    host.insert(host.end(), lo.begin(), lo.end()); host.insert(host.end(), hi.begin(), hi.end()); host.insert(host.end(), pre.begin(), pre.end());

    const size_t bit_words = (size_t)(tlen >> 5) + 1;            // bits 0 .. tlen
    int rc;
    if ((rc = c.mask_bits.ensure(bit_words * 4))) return rc;
    if ((rc = c.mask_ranges.ensure(host.size() * 4))) return rc;
    if ((rc = c.tb_keys.ensure(((size_t)nw + 1) * 4))) return rc;      // the keep flags
    if ((rc = c.tb_keys2.ensure(((size_t)nw + 1) * 4))) return rc;     // their exclusive scan
    if ((rc = c.tb_vals2.ensure((size_t)nw * 4))) return rc;           // the kept entries
    u32* const bits = c.mask_bits.as<u32>();
    u32* const d_lo = c.mask_ranges.as<u32>(); u32* const d_hi = d_lo + nr; u32* const d_pre = d_hi + nr;
    u32* const keep = c.tb_keys.as<u32>(); u32* const idx = c.tb_keys2.as<u32>(); u32* const npos = c.tb_vals2.as<u32>();

    LZ_HIP(hipMemsetAsync(bits, 0, bit_words * 4, c.stream));
    LZ_HIP(hipMemcpyAsync(d_lo, host.data(), host.size() * 4, hipMemcpyHostToDevice, c.stream));
    c.timer.begin("k_mask_bits", c.stream);
    hipLaunchKernelGGL(k_mask_bits, dim3((unsigned)((total + LZ_TPB - 1) / LZ_TPB)), dim3(LZ_TPB), 0, c.stream,
                       d_lo, d_hi, d_pre, nr, total, bits);
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    c.timer.begin("k_mask_keep", c.stream);
    hipLaunchKernelGGL(k_mask_keep, dim3((nw + 1 + LZ_TPB - 1) / LZ_TPB), dim3(LZ_TPB), 0, c.stream,
                       c.wpos.as<u32>(), nw, bits, tlen, keep);
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    size_t tmp = 0;
    LZ_HIP(rocprim::exclusive_scan(nullptr, tmp, keep, idx, 0u, (size_t)nw + 1, rocprim::plus<u32>(), c.stream));
    if ((rc = c.scan_tmp.ensure(tmp))) return rc;
    c.timer.begin("rocprim_scan_mask", c.stream);
    LZ_HIP(rocprim::exclusive_scan(c.scan_tmp.p, tmp, keep, idx, 0u, (size_t)nw + 1, rocprim::plus<u32>(), c.stream));
    c.timer.end(c.stream);
    u32 kept = 0;
    LZ_HIP(hipMemcpyAsync(&kept, idx + nw, 4, hipMemcpyDeviceToHost, c.stream));
    LZ_HIP(hipStreamSynchronize(c.stream));                      // (also: `host` was read)
    c.timer.resolve();
    if (kept == nw) return 0;                                    // nothing goes: the table and its generation as they are

    const u32 lanes = nw > nwords + 1 ? nw : nwords + 1;
    c.timer.begin("k_mask_move", c.stream);
    hipLaunchKernelGGL(k_mask_move, dim3((lanes + LZ_TPB - 1) / LZ_TPB), dim3(LZ_TPB), 0, c.stream,
                       c.wpos.as<u32>(), keep, idx, nw, c.wstart.as<u32>(), nwords, npos);
    c.timer.end(c.stream);
    hipError_t e = hipGetLastError();                            // from here on wstart[] is being rewritten: an error leaves no table
    if (e == hipSuccess && kept) e = hipMemcpyAsync(c.wpos.p, npos, (size_t)kept * 4, hipMemcpyDeviceToDevice, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    c.timer.resolve();
    if (e != hipSuccess) { c.have_table = false; return lz_fail(LZGPU_ERR_HIP, "lzgpu_table_mask: %s (the table is lost)", hipGetErrorString(e)); }
    c.num_words = kept; c.geom.num_words = kept;
    c.table_gen++;                                               // (wctx follows wpos)
    return 0;
}
