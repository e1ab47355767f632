// emul_exact.cpp -- the exact-match extension of seed hits (lastz --exact) on the CPU, twice: a plain serial statement of what
// the reference does per raw hit, on the bytes; and the GPU's decomposition -- lz_exact.hpp's summaries of every hit on its
// own, then every bucket's records settled in order -- on the match codes.  tests/test_exact_cases.py compares the two.
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../lastz_amd/csrc/lz_exact.hpp"

namespace {

bool same_base(const int8_t* mb, u8 a, u8 b) { return a != 0 && b != 0 && mb[a] >= 0 && mb[a] == mb[b]; }

// the match codes of one sequence as the library lays them out (k_pack2): base i at bit i + LZ_PAD2, everything else masked
struct Codes {
    std::vector<u8> two, spc;
    Codes(const u8* s, u32 len, const int8_t* mb)
    {
        u8 cls[256];
        lz_exact_cls(mb, cls);
        const size_t nmask = ((size_t)len + 2 * LZ_PAD2 + 7) / 8 + 16;
        two.assign(nmask * 2 + 96, 0); spc.assign(nmask + 96, 0xFF);
        for (u32 i = 0; i < len; i++) {
            const u8 c = cls[s[i]];
            if (c & LZ_CODE_INVALID) continue;
            const size_t b = (size_t)i + LZ_PAD2;
            spc[b >> 3] &= (u8)~(1u << (b & 7));
            two[b >> 2] |= (u8)(LZ_GRAY(LZ_CODE_BITS(c)) << (2 * (b & 3)));
        }
    }
};

}

// counters: [0] windows that are not exact matches, [1] left ends stopped by diagEnd while the bases went on matching,
// [2] hits dropped by diagEnd, [3] of [1] and [2] those whose diagEnd was written from another diagonal, [4] hits with a
// run of at least LZ_EX_CAP bases on either side
extern "C" int emul_exact_serial(const u8* t, u32 tlen, const u8* q, u32 qlen, const int8_t* mb, u32 L, s32 thr,
                                 const u32* pos1s, const u32* pos2s, u64 nhits, u32* rows /*[4 * nhits]*/, u64* n_rows, u64* counters /*[5]*/)
{
    std::vector<u32> dend(LZ_DIAG_SIZE, 0);
    std::vector<s32> from(LZ_DIAG_SIZE, 0);
    u64 n = 0;
    memset(counters, 0, 5 * sizeof(u64));
    for (u64 i = 0; i < nhits; i++) {
        const u32 pos1 = pos1s[i], pos2 = pos2s[i];
        const s32 diag = (s32)(pos1 - pos2);
        const u32 h = (u32)diag & (LZ_DIAG_SIZE - 1);
        const bool other = dend[h] != 0 && from[h] != diag;
        if (dend[h] > pos2 - L) { counters[2]++; if (other) counters[3]++; continue; }
        // the window, from its last base to its first
        u32 k = 0;
        while (k < L && same_base(mb, t[pos1 - 1 - k], q[pos2 - 1 - k])) k++;
        if (k < L) {
            counters[0]++;
            const u32 m = pos2 - 1 - k;
            if (m > dend[h]) { dend[h] = m; from[h] = diag; }
            continue;
        }
        // to the left of the window, no further than the old diagEnd in the query and the start of either sequence
        u32 left = 0;
        while (pos2 - L - left > dend[h] && pos1 - L - left > 0 && same_base(mb, t[pos1 - L - left - 1], q[pos2 - L - left - 1])) left++;
        u32 more = left;                                        // ... and where the bases themselves would have stopped
        while (pos2 - L - more > 0 && pos1 - L - more > 0 && same_base(mb, t[pos1 - L - more - 1], q[pos2 - L - more - 1])) more++;
        if (more > left) { counters[1]++; if (other) counters[3]++; }
        // to the right, to the end of either sequence
        u32 right = 0;
        while (pos1 + right < tlen && pos2 + right < qlen && same_base(mb, t[pos1 + right], q[pos2 + right])) right++;
        if (more >= LZ_EX_CAP || right >= LZ_EX_CAP) counters[4]++;
        if (pos2 + right > dend[h]) { dend[h] = pos2 + right; from[h] = diag; }
        const u32 length = left + L + right;
        if (length >= (u32)thr) { u32* r = rows + 4 * n++; r[0] = pos1 + right; r[1] = pos2 + right; r[2] = length; r[3] = length; }
    }
    *n_rows = n;
    return 0;
}

extern "C" int emul_exact_decomposed(const u8* t, u32 tlen, const u8* q, u32 qlen, const int8_t* mb, u32 L, s32 thr,
                                     const u32* pos1s, const u32* pos2s, u64 nhits, u32* rows /*[4 * nhits]*/, u64* n_rows, u64* n_slow)
{
    const Codes tc(t, tlen, mb), qc(q, qlen, mb);
    LzExactParams P;
    P.t2 = tc.two.data(); P.tsp = tc.spc.data(); P.q2 = qc.two.data(); P.qsp = qc.spc.data();
    P.tlen = tlen; P.qlen = qlen; P.seed_len = L; P.thr = (u32)thr;
    // phase A: every hit on its own
    std::vector<u64> rec(nhits);
    *n_slow = 0;
    for (u64 i = 0; i < nhits; i++) {
        const u64 key = lz_hit_key(pos1s[i], pos2s[i]);
        const u32 summ = lz_exact_summary(P, key);
        if (summ & LZ_SUMM_SLOW) ++*n_slow;
        rec[i] = lz_hit_record(key, summ);
    }
    // phase B: the buckets one after the other, each one's records in discovery order
    std::vector<u64> order(nhits);
    for (u64 i = 0; i < nhits; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](u64 a, u64 b) { return ((pos1s[a] - pos2s[a]) & 0xFFFFu) < ((pos1s[b] - pos2s[b]) & 0xFFFFu); });
    struct Found { u64 at; LzHspRec r; };
    std::vector<Found> found;
    u32 dend = 0, cur = 0xFFFFFFFFu;
    for (u64 k = 0; k < nhits; k++) {
        const u64 i = order[k];
        const u32 h = (pos1s[i] - pos2s[i]) & 0xFFFFu;
        if (h != cur) { cur = h; dend = 0; }
        lz_exact_settle_record(P, rec[i], h, dend, [&](const LzHspRec& r) { found.push_back({ i, r }); });
    }
    std::sort(found.begin(), found.end(), [](const Found& a, const Found& b) { return a.at < b.at; });
    u64 n = 0;
    for (const Found& f : found) {
        const s32 diag = (s32)f.r.seed_pos1 - (s32)f.r.seed_pos2;
        u32* r = rows + 4 * n++;
        r[0] = f.r.end1; r[1] = (u32)((s32)f.r.end1 - diag); r[2] = f.r.length; r[3] = (u32)f.r.score;
    }
    *n_rows = n;
    return 0;
}
