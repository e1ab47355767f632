// limit_kernels.hip -- gfx950 kernels of the word-count limit (lastz --maxwordcount; DESIGN.md section 1, "Word-count limit"):
// limit_position_table with maxChasm / step == 0 (src/pos_table.c:1763-1948) as a second, smaller CSR table made from the one
// that was built, and the list lengths' distribution that find_position_table_limit walks (src/pos_table.c:2000-2034, 2064-2140).
// The table as it was built is only read here.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <utility>
#include "lz_ctx.hpp"
#include "lz_seed_dev.hpp"

// len[w] = entries of word w's list, w < nwords; with a limit (limit_position_table, :1907-1923: a list of more than `limit`
// entries goes as a whole, every other list stays) 0 for a list that goes.  len[nwords] = 0: the exclusive scan of the
// nwords + 1 values is the limited wstart[], its last value the entries that stay.
__global__ void __launch_bounds__(LZ_TPB)
k_limit_lengths(const u32* __restrict__ wstart, u32 nwords, u32 limit, u32* __restrict__ len)
{
    const u32 w = blockIdx.x * LZ_TPB + threadIdx.x;
    if (w > nwords) return;
    u32 n = 0;
    if (w < nwords) { n = wstart[w + 1] - wstart[w]; if (n > limit) n = 0; }
    len[w] = n;
}

// The lists that stay, each in its order (descending pos1: the discovery order of the hits), at their new places.  A workgroup
// takes LZ_TPB neighbouring words: their lists lie back to back in the new table, so it copies that one stretch, lane after
// lane -- the stores are contiguous whatever the lists' lengths, the loads contiguous inside a list.  The word of an entry of
// the stretch is found by bisection over the words' new starts (LDS): the last word that starts at or before it (the words
// after it that start at the same place are empty or removed).
__global__ void __launch_bounds__(LZ_TPB)
k_limit_copy(const u32* __restrict__ wstart, const u32* __restrict__ wpos, const u32* __restrict__ nstart, u32 nwords,
             u32* __restrict__ npos)
{
    __shared__ u32 dst[LZ_TPB + 1], src[LZ_TPB];
    const u32 w0 = blockIdx.x * LZ_TPB;                          // (w0 < nwords: the grid covers the words)
    const u32 cnt = nwords - w0 < (u32)LZ_TPB ? nwords - w0 : (u32)LZ_TPB;
    const u32 t = threadIdx.x;
    if (t < cnt) { dst[t] = nstart[w0 + t]; src[t] = wstart[w0 + t]; }
    if (t == 0) dst[cnt] = nstart[w0 + cnt];                     // (nstart has nwords + 1 entries)
    __syncthreads();
    const u32 d0 = dst[0], d1 = dst[cnt];
    for (u32 k = d0 + t; k < d1; k += LZ_TPB) {
        u32 lo = 0, hi = cnt;                                    // the last l in [0, cnt) with dst[l] <= k (dst[0] <= k < dst[cnt])
        while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (dst[mid] <= k) lo = mid; else hi = mid; }
        npos[k] = wpos[src[lo] + (k - dst[lo])];
    }
}

namespace {
struct Scratch : DevBuf { ~Scratch() { release(); } };          // a device buffer for the time of one call (hipFree waits for the device)
}

// the table as it was built, in the searches' place again
void lz_limit_lift(LzCtx& c)
{
    c.limit = 0;
    if (!c.limited()) return;
    (void)hipStreamSynchronize(c.stream);
    std::swap(c.wstart, c.full_wstart); std::swap(c.wpos, c.full_wpos);
    c.full_wstart.release(); c.full_wpos.release();              // (the limited copy)
    c.num_words = c.full_num_words; c.full_num_words = 0;
    c.table_gen++;
}

int lzk_table_limit(LzCtx& c, u32 limit)
{
    const u32 nwords = 1u << c.seed.weight;
    const size_t n1 = (size_t)nwords + 1;
    DevBuf nws, nwp;
    Scratch kept_len;                                            // a length per word, 0 for a list that goes
    int rc;
    if ((rc = kept_len.ensure(n1 * 4))) return rc;
    if ((rc = nws.ensure(n1 * 4))) return rc;
    c.timer.begin("k_limit_lengths", c.stream);
    hipLaunchKernelGGL(k_limit_lengths, dim3((unsigned)((n1 + LZ_TPB - 1) / LZ_TPB)), dim3(LZ_TPB), 0, c.stream,
                       c.wstart.as<u32>(), nwords, limit, kept_len.as<u32>());
    c.timer.end(c.stream);
    size_t tmp = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, tmp, kept_len.as<u32>(), nws.as<u32>(), 0u, n1, rocprim::plus<u32>(), c.stream);
    if (e == hipSuccess && !(rc = c.scan_tmp.ensure(tmp))) {
        c.timer.begin("rocprim_scan_limit", c.stream);
        e = rocprim::exclusive_scan(c.scan_tmp.p, tmp, kept_len.as<u32>(), nws.as<u32>(), 0u, n1, rocprim::plus<u32>(), c.stream);
        c.timer.end(c.stream);
    }
    u32 kept = 0;
    if (e == hipSuccess && !rc) e = hipMemcpyAsync(&kept, nws.as<u32>() + nwords, 4, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess && !rc) e = hipStreamSynchronize(c.stream);
    c.timer.resolve();
    if (e == hipSuccess && !rc && kept == c.num_words) { nws.release(); c.limit = limit; return 0; }   // nothing goes: the table as it is
    if (e == hipSuccess && !rc) rc = nwp.ensure((size_t)(kept ? kept : 1) * 4);
    if (e == hipSuccess && !rc && kept) {
        c.timer.begin("k_limit_copy", c.stream);
        hipLaunchKernelGGL(k_limit_copy, dim3((nwords + LZ_TPB - 1) / LZ_TPB), dim3(LZ_TPB), 0, c.stream,
                           c.wstart.as<u32>(), c.wpos.as<u32>(), nws.as<u32>(), nwords, nwp.as<u32>());
        c.timer.end(c.stream);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
        c.timer.resolve();
    }
    if (e != hipSuccess || rc) {
        nws.release(); nwp.release();
        return rc ? rc : lz_fail(LZGPU_ERR_HIP, "lzgpu_table_limit: %s", hipGetErrorString(e));
    }
    c.full_wstart = c.wstart; c.full_wpos = c.wpos; c.full_num_words = c.num_words;
    c.wstart = nws; c.wpos = nwp; c.num_words = kept;
    c.limit = limit;
    c.table_gen++;                                               // (wctx follows wpos)
    return 0;
}

// position_table_count_distribution (src/pos_table.c:2064-2140) of the table as it was built: the lists' lengths sorted and
// run-length encoded; the length 0 (the words that do not occur) is left out, as the reference leaves it out (:2094)
int lzk_table_count_distribution(LzCtx& c, std::vector<u32>& count, std::vector<u32>& words)
{
    const u32 nwords = 1u << c.seed.weight;
    const u64 entries = c.built_num_words();
    const size_t n1 = (size_t)nwords + 1;                          // (k_limit_lengths' closing 0 is sorted along: one more word of length 0)
    count.clear(); words.clear();
    Scratch buf;                                                 // the lengths, the same sorted, the runs' lengths and sizes, their number
    int rc;
    if ((rc = buf.ensure(4 * n1 * 4 + 4))) return rc;            // (as many runs as words at worst, whatever wstart[] holds)
    u32* const len = buf.as<u32>(); u32* const sorted = len + n1;
    u32* const uniq = sorted + n1;        u32* const runs = uniq + n1; u32* const nruns_dev = runs + n1;
    hipLaunchKernelGGL(k_limit_lengths, dim3((unsigned)((n1 + LZ_TPB - 1) / LZ_TPB)), dim3(LZ_TPB), 0, c.stream,
                       c.built_wstart().as<u32>(), nwords, 0xFFFFFFFFu, len);
    LZ_HIP(hipGetLastError());
    unsigned bits = 1; while (bits < 32 && (entries >> bits)) bits++;
    size_t tmp = 0;
    LZ_HIP(rocprim::radix_sort_keys(nullptr, tmp, len, sorted, n1, 0u, bits, c.stream));
    if ((rc = c.sort_tmp.ensure(tmp))) return rc;
    LZ_HIP(rocprim::radix_sort_keys(c.sort_tmp.p, tmp, len, sorted, n1, 0u, bits, c.stream));
    LZ_HIP(rocprim::run_length_encode(nullptr, tmp, sorted, (unsigned)n1, uniq, runs, nruns_dev, c.stream));
    if ((rc = c.scan_tmp.ensure(tmp))) return rc;
    LZ_HIP(rocprim::run_length_encode(c.scan_tmp.p, tmp, sorted, (unsigned)n1, uniq, runs, nruns_dev, c.stream));
    u32 nruns = 0;
    LZ_HIP(hipMemcpyAsync(&nruns, nruns_dev, 4, hipMemcpyDeviceToHost, c.stream));
    LZ_HIP(hipStreamSynchronize(c.stream));
    std::vector<u32> u(nruns), r(nruns);
    if (nruns) {
        LZ_HIP(hipMemcpyAsync(u.data(), uniq, (size_t)nruns * 4, hipMemcpyDeviceToHost, c.stream));
        LZ_HIP(hipMemcpyAsync(r.data(), runs, (size_t)nruns * 4, hipMemcpyDeviceToHost, c.stream));
        LZ_HIP(hipStreamSynchronize(c.stream));
    }
    for (u32 k = 0; k < nruns; k++) if (u[k]) { count.push_back(u[k]); words.push_back(r[k]); }
    return 0;
}
