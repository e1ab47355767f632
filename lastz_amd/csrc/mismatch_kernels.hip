// mismatch_kernels.hip -- phase A of an N-mismatch search (lastz --mismatch; lz_mismatch.hpp): in the place of k_scan_exact on
// the two-kernel path:
//   k_fill_hits -> k_scan_mismatch -> k_partition<false> -> k_hist_scan -> k_settle_mismatch (settle_kernels.hip)
// One lane per hit, independent of the diagonal hash: from the key the fill kernel wrote it counts the window's mismatches and
// reads both sides' mismatch maps up to LZ_EX_CAP bases, on the match codes of both sequences, 32 bases per load pair and no
// more words than the K-th mismatch needs.  The output is the 4-byte summary k_partition<false> packs into the hit's record.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "lz_ctx.hpp"
#include "lz_seed_dev.hpp"
#include "lz_mismatch.hpp"

#define LZ_MM_TPB 256
__global__ void __launch_bounds__(LZ_MM_TPB)
k_scan_mismatch(LzMismatchParams P, const u64* __restrict__ keys, u64 n, u32* __restrict__ summ)
{
    for (u64 i = (u64)blockIdx.x * LZ_MM_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * LZ_MM_TPB)
        LZ_NT_ST(lz_mismatch_summary(P, LZ_NT_LD(keys + i)), summ + i);
}

// phase A of the n hits in c.keys: summaries -> c.summ (n * 4 bytes, reserved by the caller)
int lzk_scan_mismatch(LzCtx& c, const LzMismatchParams& P, u64 n)
{
    if (n == 0) return 0;
    if (!c.summ.p || c.summ.cap < (size_t)n * 4) return LZGPU_ERR_ARG;
    const u64 want = (n + LZ_MM_TPB - 1) / LZ_MM_TPB;
    const u32 grid = (u32)std::min<u64>(want, 32u * (u64)c.num_cus);       // (as k_scan_exact: the gathers are latency-bound)
    c.timer.begin("k_scan_mismatch", c.stream);
    hipLaunchKernelGGL(k_scan_mismatch, dim3(grid), dim3(LZ_MM_TPB), 0, c.stream, P, c.keys.as<u64>(), n, c.summ.as<u32>());
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    return 0;
}
