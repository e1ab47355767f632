// enum_kernels.hip -- gfx950 kernels of hit enumeration: the query's seed words sorted
// inside blocks of positions, raw-hit counts per position and their scan, and the two fill kernels that materialise a
// chunk's hits in discovery order.  Steps 1 and 2 of k_fill_hits2's list enumeration are text it shares with k_scan_hits2
// (scan_kernels.hip): the fragments lz_enum_lists.inc, lz_enum_place.inc and lz_enum_owners.inc, included inside the kernel.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include "lz_ctx.hpp"
#include "lz_host.hpp"
#include "lz_seed_dev.hpp"

// ------------------------------------------------------------------------------------------
// B2 step 1: raw hits per query position (private_hit_search + find_table_matches,
// src/seed_search.c:491-571, 810-875, without calling the processor yet).
//
// The table probes are random 4-byte reads into a 64 MiB + 4*Tlen byte structure: taken in query order
// every probe costs a whole cache line from the fabric (measured: 290 GB per step for k_fill_hits alone).
// The query positions are therefore visited in the order of their seed words: (word, position) pairs are
// radix-sorted once per search, and both the count and the fill kernels walk that list, so that each of
// the 13 probe streams (word ^ flip) moves through wstart[] / wpos[] front to back.  What is written --
// cnt[position] and the hits at off[position] -- is indexed by position, so the discovery order of the
// hits is untouched.
// The sort key of a query position is (block of the position) << kbits | word, kbits = weight + 1: the list is word-sorted INSIDE blocks of
// 2^bshift consecutive positions (at most 16 blocks).  What the fill kernel writes goes to off[position]: with one word order over the
// whole query a wave's 64 positions scatter their runs of keys over the whole key array of the chunk (15.5 GB for a 50 Mbp strand),
// three new pages per position -- and k_fill_hits2 took 18 or 28 ms from one process to the next on the same box, depending on what
// physical pages its buffers got.  Inside a block the destinations stay within 1/16 of the arrays, the probes still move front to back
// through the table (3-4 words between neighbouring entries: the lines of wstart[] are still shared), and a chunk of query positions is a
// contiguous range of blocks, hence of the sorted list: its launch covers that range only (a 200 Mbp strand has 29 chunks; every one of
// their launches used to read the whole list to find its 1/29).
__global__ void __launch_bounds__(LZ_TPB)
k_pack_words(const u8* __restrict__ qcode, u32 lo, u32 hi, LzSeedDev sd, u32* __restrict__ pk, u32* __restrict__ iv, u32 bshift, u32 kbits)
{
    // the block's LZ_TPB windows overlap in all but one byte: the codes go through LDS once
    __shared__ u8 win[LZ_TPB + 32];
    const u32 i = blockIdx.x * LZ_TPB + threadIdx.x;
    const u32 L = (u32)sd.length;
    const s64 first = (s64)lo + (s64)blockIdx.x * LZ_TPB + 1 - (s64)L;     // window start of the block's first position (>= -31: inside the padding)
    for (u32 k = threadIdx.x; k < LZ_TPB + L - 1; k += LZ_TPB) win[k] = (first + (s64)k < (s64)hi) ? qcode[first + (s64)k] : (u8)LZ_CODE_INVALID;
    __syncthreads();
    if (i < hi - lo) {
        const u32 pos2 = lo + i + 1;
        u64 w = 0; u32 bad = 0;
        for (u32 k = 0; k < L; k++) { const u32 c = win[threadIdx.x + k]; bad |= c; w = (w << 2) | LZ_CODE_BITS(c); }
        const bool valid = pos2 >= lo + L && !(bad & LZ_CODE_INVALID);     // window inside the interval, only ACGT
        pk[i] = ((i >> bshift) << kbits) | (valid ? lz_apply_seed(sd, w) : (1u << sd.weight));   // "no word" sorts after every real word of its block
        iv[i] = i;
    }
}
// where the blocks begin in the sorted list: bs[b] = first entry whose key's block is >= b, b in [0, nblk]; and "words in seq 2" (the
// reference's counter): inside a block the entries without a word (key's word field == none) sort behind those with one
__global__ void k_block_starts(const u32* __restrict__ sk, u32 n, u32 kbits, u32 none, u32 nblk, u64* __restrict__ bs, u64* __restrict__ n_words)
{
    const u32 b = threadIdx.x;
    if (b > nblk) return;
    auto first_at_least = [&](u64 key) { u32 lo = 0, hi = n; while (lo < hi) { const u32 m = lo + ((hi - lo) >> 1); if ((u64)sk[m] < key) lo = m + 1; else hi = m; } return lo; };
    const u32 start = first_at_least((u64)b << kbits);
    bs[b] = start;
    if (b < nblk) atomicAdd((unsigned long long*)n_words, (unsigned long long)(first_at_least(((u64)b << kbits) | none) - start));
}

__global__ void __launch_bounds__(LZ_TPB)
k_count_sorted(const u32* __restrict__ sk, const u32* __restrict__ sv, u32 n, LzSeedDev sd,
               const u32* __restrict__ wstart, u32* __restrict__ cnt)
{
    const u32 j = blockIdx.x * LZ_TPB + threadIdx.x;
    if (j >= n) return;
    const u32 w0 = sk[j] & ((2u << sd.weight) - 1u);            // (the key's low weight + 1 bits: the word, or "no word")
    if (w0 >> sd.weight) return;                                // no word at this position: cnt stays 0
    u32 c = 0;
    for (int p = 0; p < sd.nprobes; p++) { const u32 w = w0 ^ sd.probe_xor[p]; c += wstart[w + 1] - wstart[w]; }
    cnt[sv[j]] = c;
}

// bucket ownership (lzgpu_set_bucket_owner): only the hits whose hashed diagonal belongs to this process
// count; that needs the positions, so the lists are read here as well (front to back, like the fill)
__device__ __forceinline__ bool lz_owned(u32 pos1, u32 pos2, u32 n_owners, u32 owner)
{ return (((pos1 - pos2) & (LZ_DIAG_SIZE - 1)) % n_owners) == owner; }

__global__ void __launch_bounds__(LZ_TPB)
k_count_sorted_owned(const u32* __restrict__ sk, const u32* __restrict__ sv, u32 n, u32 lo, LzSeedDev sd,
                     const u32* __restrict__ wstart, const u32* __restrict__ wpos, u32* __restrict__ cnt,
                     u32 n_owners, u32 owner)
{
    const u32 j = blockIdx.x * LZ_TPB + threadIdx.x;
    if (j >= n) return;
    const u32 w0 = sk[j] & ((2u << sd.weight) - 1u);
    if (w0 >> sd.weight) return;
    const u32 i = sv[j], pos2 = lo + i + 1;
    u32 c = 0;
    for (int p = 0; p < sd.nprobes; p++) {
        const u32 w = w0 ^ sd.probe_xor[p];
        for (u32 k = wstart[w]; k < wstart[w + 1]; k++) c += lz_owned(wpos[k], pos2, n_owners, owner) ? 1u : 0u;
    }
    cnt[i] = c;
}

// self-comparison (lz_common.hpp, LzSelfDev): only the hits in [lo, hi) of pos1 count, and every list is clipped to them
// with two binary searches over its (descending) positions -- so, unlike k_count_sorted, the positions are read.  The 16
// probes of a group go through their searches in lock step (lz_clip_runs): their bounds and then each step's 16 loads are
// in flight together.  A position filter (LZ_SELF_WINDOW, lzgpu_seed_hit_search_within) is the same clip with constant bounds.
// The group loop is the statement of lz_enum_lists.inc (every position takes part here, and the lists are always clipped); it
// is written out and not included because with the fragment's text this kernel's machine code changes (as many instructions, another
// body), and the fill kernels' fragments are held to the code they had.
#define LZ_SELF_GROUP 16
__global__ void __launch_bounds__(LZ_TPB)
k_count_sorted_self(const u32* __restrict__ sk, const u32* __restrict__ sv, u32 n, u32 lo, LzSeedDev sd,
                    const u32* __restrict__ wstart, const u32* __restrict__ wpos, u32* __restrict__ cnt, LzSelfDev self)
{
    const u32 j = blockIdx.x * LZ_TPB + threadIdx.x;
    if (j >= n) return;
    const u32 w0 = sk[j] & ((2u << sd.weight) - 1u);
    if (w0 >> sd.weight) return;
    const u32 i = sv[j], pos2 = lo + i + 1;
    u32 blo, bhi;
    lz_self_bounds(self, pos2, blo, bhi);
    u32 c = 0;
    for (int r = 0; r < sd.nprobes; r += LZ_SELF_GROUP) {
        u32 a[LZ_SELF_GROUP], len[LZ_SELF_GROUP];
#pragma unroll
        for (int p = 0; p < LZ_SELF_GROUP; p++) {
            const bool on = r + p < sd.nprobes;
            const u32 w = on ? (w0 ^ sd.probe_xor[(r + p) & (LZ_MAX_PROBES - 1)]) : 0u;
            a[p] = wstart[w]; len[p] = wstart[w + 1];
        }
#pragma unroll
        for (int p = 0; p < LZ_SELF_GROUP; p++) { const bool on = r + p < sd.nprobes; len[p] = on ? len[p] - a[p] : 0u; }
        lz_clip_runs<LZ_SELF_GROUP>(wpos, a, len, blo, bhi);
#pragma unroll
        for (int p = 0; p < LZ_SELF_GROUP; p++) c += len[p];
    }
    cnt[i] = c;
}

// c.cnt, c.pk, c.wiv, c.wsk, c.wsv (sized by the caller) for the query positions [lo, hi); "words in seq 2" -> c.dev_counters[2]
int lzk_count_hits(LzCtx& c, const u8* qcode, u32 lo, u32 hi)
{
    const u32 n = hi - lo;
    u32* const cnt = c.cnt.as<u32>(); u32* const pk = c.pk.as<u32>(); u32* const iv = c.wiv.as<u32>();
    u32* const sk = c.wsk.as<u32>(); u32* const sv = c.wsv.as<u32>();
    LZ_HIP(hipMemsetAsync(cnt, 0, (size_t)n * 4, c.stream));
    // blocks of positions (k_pack_words): at most 16, fewer for the heaviest seeds (the key is 32 bits)
    const u32 kbits = (u32)c.seed.weight + 1u;
    // ... and only for a search that will need several chunks (measured: with one chunk per strand the blocks buy nothing -- the fill
    // kernel's 18-or-28 ms do not come from the range of its scatter -- and cost k_count_hits 0.8 ms of shared wstart[] lines; at 200 Mbp,
    // 29 chunks per strand, the launches' ranges take the fill from 292 to 232 ms per step): twice as many blocks as expected chunks
    const double est_hits = (double)n * (double)c.num_words * (double)c.seed.nprobes / (double)(1ull << c.seed.weight);
    u32 want_bits = 0;
    while (want_bits < 5 && est_hits > (double)c.hit_capacity * (double)(1u << want_bits) * 0.5) want_bits++;
    if (est_hits <= (double)c.hit_capacity) want_bits = 0;
    u32 bbits = std::min<u32>(want_bits, 32u - kbits);
    u32 bshift = 0;
    const u64 nm1 = n ? (u64)n - 1 : 0;
    while (bshift < 32 && (nm1 >> bshift) >= (1ull << bbits)) bshift++;
    c.blk_shift = bshift; c.blk_count = (u32)((nm1 >> bshift) + 1);
    c.timer.begin("k_pack_words", c.stream);
    hipLaunchKernelGGL(k_pack_words, dim3((n + LZ_TPB - 1) / LZ_TPB), dim3(LZ_TPB), 0, c.stream,
                       qcode, lo, hi, c.seed, pk, iv, bshift, kbits);
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    size_t tmp = 0;
    const unsigned bits = kbits + bbits;
    LZ_HIP(rocprim::radix_sort_pairs(nullptr, tmp, pk, sk, iv, sv, (size_t)n, 0u, bits, c.stream));
    int rc = c.sort_tmp.ensure(tmp);
    if (rc) return rc;
    c.timer.begin("rocprim_sort_words", c.stream);
    LZ_HIP(rocprim::radix_sort_pairs(c.sort_tmp.p, tmp, pk, sk, iv, sv, (size_t)n, 0u, bits, c.stream));
    c.timer.end(c.stream);
    if ((rc = c.blk_start.ensure(130 * 8))) return rc;
    hipLaunchKernelGGL(k_block_starts, dim3(1), dim3(192), 0, c.stream, sk, n, kbits, 1u << c.seed.weight, c.blk_count, c.blk_start.as<u64>(), c.dev_counters.as<u64>() + 2);
    c.timer.begin("k_count_hits", c.stream);
    if (c.self.mode != LZ_SELF_OFF)
        hipLaunchKernelGGL(k_count_sorted_self, dim3((n + LZ_TPB - 1) / LZ_TPB), dim3(LZ_TPB), 0, c.stream,
                           sk, sv, n, lo, c.seed, c.wstart.as<u32>(), c.wpos.as<u32>(), cnt, c.self);
    else if (c.n_owners > 1)
        hipLaunchKernelGGL(k_count_sorted_owned, dim3((n + LZ_TPB - 1) / LZ_TPB), dim3(LZ_TPB), 0, c.stream,
                           sk, sv, n, lo, c.seed, c.wstart.as<u32>(), c.wpos.as<u32>(), cnt, c.n_owners, c.owner);
    else
        hipLaunchKernelGGL(k_count_sorted, dim3((n + LZ_TPB - 1) / LZ_TPB), dim3(LZ_TPB), 0, c.stream,
                           sk, sv, n, c.seed, c.wstart.as<u32>(), cnt);
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    return 0;
}

struct U32ToU64 { __host__ __device__ u64 operator()(u32 x) const { return (u64)x; } };

// c.off = exclusive scan of c.cnt
int lzk_scan_counts(LzCtx& c, u32 n)
{
    const u32* const cnt = c.cnt.as<u32>(); u64* const off = c.off.as<u64>();
    auto in = rocprim::make_transform_iterator(cnt, U32ToU64());
    size_t tmp = 0;
    LZ_HIP(rocprim::exclusive_scan(nullptr, tmp, in, off, (u64)0, (size_t)n, rocprim::plus<u64>(), c.stream));
    int rc = c.scan_tmp.ensure(tmp);
    if (rc) return rc;
    c.timer.begin("rocprim_scan_counts", c.stream);
    LZ_HIP(rocprim::exclusive_scan(c.scan_tmp.p, tmp, in, off, (u64)0, (size_t)n, rocprim::plus<u64>(), c.stream));
    c.timer.end(c.stream);
    return 0;
}

// total number of hits and every stride-th prefix sum, written straight into pinned host memory:
// out[0] = total, out[1 + k] = off[k * stride]
__global__ void __launch_bounds__(LZ_TPB)
k_sample_offsets(const u64* __restrict__ off, const u32* __restrict__ cnt, u32 n, u32 stride, u32 ns, u64* __restrict__ out)
{
    const u32 k = blockIdx.x * LZ_TPB + threadIdx.x;
    if (k < ns) out[1 + k] = off[(size_t)k * stride];
    if (k == 0) out[0] = off[n - 1] + cnt[n - 1];
}

int lzk_sample_offsets(LzCtx& c, u32 n, u32 stride, u32 ns)      // -> c.pinned
{
    hipLaunchKernelGGL(k_sample_offsets, dim3((ns + LZ_TPB - 1) / LZ_TPB), dim3(LZ_TPB), 0, c.stream, c.off.as<u64>(), c.cnt.as<u32>(), n, stride, ns, c.pinned);
    LZ_HIP(hipGetLastError());
    return 0;
}

// B2 step 2: materialise the hits of query positions [i0,i1) in discovery order.
// k_fill_hits is the fill of a process that owns a share of the buckets (lzgpu_set_bucket_owner); every other search
// goes through k_fill_hits2 below or k_scan_hits2 (scan_kernels.hip).
// A wave takes 64 entries of the word-sorted list, keeps those whose position lies in [i0,i1) (the hit
// arrays hold one chunk of positions at a time) and serves them four at a time: 16 lanes per position, one
// probe (exact word / transition flip) per lane.  Each lane reads its word's CSR range and counts the hits it owns, a
// 16-lane prefix sum places the probes' lists back to back in probe order (= the reference's enumeration order within a
// position, src/seed_search.c:522-549), and every lane writes its list's owned hits from off[position] on.
__global__ void __launch_bounds__(LZ_TPB)
k_fill_hits(u32 lo, u32 i0, u32 i1, LzSeedDev sd,
            const u32* __restrict__ wstart, const u32* __restrict__ wpos,
            const u32* __restrict__ sk, const u32* __restrict__ sv, u32 n, const u64* __restrict__ off,
            u64 base, u64* __restrict__ keys, u32 n_owners, u32 owner)
{
    const u32 lane = threadIdx.x & 63u, p = lane & (LZ_FILL_GROUP - 1), g = lane >> 4;
    const u32 j = (blockIdx.x * LZ_TPB + threadIdx.x);         // one sorted entry per lane (sk / sv: the chunk's range of the list)
    u32 w_l = 0, i_l = 0; bool in = false;
    if (j < n) { w_l = sk[j] & ((2u << sd.weight) - 1u); i_l = sv[j]; in = !(w_l >> sd.weight) && i_l >= i0 && i_l < i1; }
    u64 todo = __ballot(in);
    while (todo) {                                              // wave-uniform
        // the next four entries of the wave, one per 16-lane group
        int src = -1;
        u64 m = todo;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int s_q = m ? (int)__ffsll((long long)m) - 1 : -1;
            if (m) m &= m - 1;
            if ((int)g == q) src = s_q;
        }
        todo = m;
        const bool have = src >= 0;
        const u32 packed = __shfl(w_l, have ? src : 0);
        const u32 i = __shfl(i_l, have ? src : 0);
        const u32 pos2 = lo + i + 1;
        u64* out = have ? keys + (off[i] - base) : keys;
        u32 carry = 0;
        for (int r = 0; r < sd.nprobes; r += LZ_FILL_GROUP) {   // uniform trip count
            u32 a = 0, len = 0, full = 0;
            if (have && r + (int)p < sd.nprobes) {
                const u32 w = packed ^ sd.probe_xor[r + p];
                a = wstart[w]; full = wstart[w + 1] - a;
                for (u32 jj = 0; jj < full; jj++) len += lz_owned(wpos[a + jj], pos2, n_owners, owner) ? 1u : 0u;
            }
            u32 incl = len;                                  // inclusive prefix over the 16-lane group
#pragma unroll
            for (int d = 1; d < LZ_FILL_GROUP; d <<= 1) {
                u32 v = __shfl_up(incl, d, LZ_FILL_GROUP);
                if ((int)p >= d) incl += v;
            }
            const u32 total = __shfl(incl, LZ_FILL_GROUP - 1, LZ_FILL_GROUP);
            u64* o = out + carry + (incl - len);
            for (u32 jj = 0; jj < full; jj++) { const u32 p1 = wpos[a + jj]; if (lz_owned(p1, pos2, n_owners, owner)) *o++ = lz_hit_key(p1, pos2); }
            carry += total;
        }
    }
}

// ---- k_fill_hits2 (round 4): the same hits at the same places, the lists found through LDS instead of shuffles.
// The scheme, steps 1 to 3, is told in lz_enum_place.inc.  Steps 1 and 2 are text that this kernel and k_scan_hits2 (the fused path,
// scan_kernels.hip) include -- lz_enum_place.inc with lz_enum_lists.inc, and lz_enum_owners.inc; step 3 is the kernel's own: here one
// gather from wpos[] and one key stored per hit.  The stores of a wave are runs of consecutive keys (one run per position), as before.
#define LZ_F2_CAP   2560                             // k_fill_hits2's CAP: own[] 5 KiB + 4.5 KiB of tables per wave = four workgroups per CU (the 64 positions of a wave have 2.5 k hits on the 50 Mbp pair)
#define LZ_F2_WORDS (LZ_F2_CAP / 2 / 64)             // 32-bit words of own[] per lane
// SELF: a self-comparison (lz_common.hpp, LzSelfDev): step 1 clips every list to the hits that survive.  Also the instantiation of a
// position filter (LZ_SELF_WINDOW): lz_self_bounds gives its constant window.
template <bool SELF>
__global__ void __launch_bounds__(LZ_TPB)
k_fill_hits2(u32 lo, u32 i0, u32 i1, LzSeedDev sd,
             const u32* __restrict__ wstart, const u32* __restrict__ wpos,
             const u32* __restrict__ sk, const u32* __restrict__ sv, u32 n, const u64* __restrict__ off,
             u64 base, u64* __restrict__ keys, LzSelfDev self)
{
    constexpr int CAP = LZ_F2_CAP, WORDS = LZ_F2_WORDS;         // (the fragments' names, as in k_scan_hits2)
    __shared__ LzListWave<CAP> shw[LZ_TPB / 64];
    LzListWave<CAP>& sh = shw[threadIdx.x >> 6];
    unsigned short* const own = reinterpret_cast<unsigned short*>(sh.own32);
    const u32 lane = threadIdx.x & 63u;
    const u32 j = blockIdx.x * LZ_TPB + threadIdx.x;           // one sorted entry per lane (sk / sv: the chunk's range of the list)
    u32 w_l = 0, i_l = 0; bool in = false;
    if (j < n) { w_l = sk[j] & ((2u << sd.weight) - 1u); i_l = sv[j]; in = !(w_l >> sd.weight) && i_l >= i0 && i_l < i1; }
    if (!__ballot(in)) return;                                  // (wave-uniform: nothing of this chunk among the wave's entries)
    const u32 dbase = in ? (u32)(off[i_l] - base) : 0u;         // (hit indices inside a chunk are 32-bit)
    const u32 pos2 = lo + i_l + 1u;
    u32 slo = 0, shi = 0;
    if (SELF) lz_self_bounds(self, pos2, slo, shi);
    u32 carry = 0;                                              // hits of the lane's position in the probe groups already done
    for (int r = 0; r < sd.nprobes; r += LZ_FILL_GROUP) {       // uniform trip count
        // ---- 1. the lane's lists and their places in the wave's concatenation
#include "lz_enum_place.inc"
        // ---- 2. + 3., a piece of CAP hits at a time
        for (u32 cs = 0; cs < T; cs += CAP) {                   // uniform
            const u32 tc = (T - cs < (u32)CAP) ? T - cs : (u32)CAP;
#include "lz_enum_owners.inc"
            // ---- 3. the hits of the piece, 64 per trip, consecutive lanes = consecutive hits; four trips' gathers in flight
            // (a lane beyond the end of the piece reads the last hit again and stores nothing: no branch around the loads)
            for (u32 tb = 0; tb < tc; tb += 256u) {
                u32 p1[4], p2[4], dst[4]; bool ok[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const u32 t0 = tb + 64u * (u32)k + lane;
                    ok[k] = t0 < tc;
                    const u32 t = ok[k] ? t0 : tc - 1u;
                    const u32 list = (u32)own[t] - 1u;
                    const u32 ls = sh.lsrc[list];
                    const uint2 en = sh.ent[list / LZ_FILL_GROUP];
                    const u32 tabs = cs + t;
                    p1[k] = wpos[ls + tabs]; p2[k] = en.y; dst[k] = en.x + tabs;
                }
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (ok[k]) LZ_NT_ST(lz_hit_key(p1[k], p2[k]), keys + dst[k]);
            }
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
        }
        carry += total;
    }
}

// the hits of chunk ch -- query positions lo + [ch.i0, ch.i1) of the n that c.wsk / c.wsv hold sorted -- at c.off[position] - ch.base in c.keys
int lzk_fill_hits(LzCtx& c, u32 lo, const LzChunk& ch, u32 n)
{
    if (n == 0 || ch.i1 <= ch.i0) return 0;
    const u32* sk = c.wsk.as<u32>(); const u32* sv = c.wsv.as<u32>();
    lz_chunk_range(c, ch.i0, ch.i1, sk, sv, n);
    if (n == 0) return 0;
    const u64* const off = c.off.as<u64>(); u64* const keys = c.keys.as<u64>();
    const dim3 grid((unsigned)(((u64)n + LZ_TPB - 1) / LZ_TPB));
    c.timer.begin("k_fill_hits", c.stream);
    if (c.self.mode != LZ_SELF_OFF)                             // (lzgpu_seed_hit_search_self / _within decline bucket owners: only k_fill_hits2 clips)
        hipLaunchKernelGGL(k_fill_hits2<true>, grid, dim3(LZ_TPB), 0, c.stream,
                           lo, ch.i0, ch.i1, c.seed, c.wstart.as<u32>(), c.wpos.as<u32>(), sk, sv, n, off, ch.base, keys, c.self);
    else if (c.n_owners > 1)
        hipLaunchKernelGGL(k_fill_hits, grid, dim3(LZ_TPB), 0, c.stream,
                           lo, ch.i0, ch.i1, c.seed, c.wstart.as<u32>(), c.wpos.as<u32>(), sk, sv, n, off, ch.base, keys, c.n_owners, c.owner);
    else
        hipLaunchKernelGGL(k_fill_hits2<false>, grid, dim3(LZ_TPB), 0, c.stream,
                           lo, ch.i0, ch.i1, c.seed, c.wstart.as<u32>(), c.wpos.as<u32>(), sk, sv, n, off, ch.base, keys, LzSelfDev{});
    c.timer.end(c.stream);
    LZ_HIP(hipGetLastError());
    return 0;
}
