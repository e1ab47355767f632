// emul_mismatch.cpp -- the N-mismatch extension of seed hits (lastz --mismatch) on the CPU, twice: a plain serial transcription
// of what the reference does per raw hit (src/seed_search.c:1113, :3450-3778), on the bytes, with counters of its branches; and
// the GPU's decomposition -- lz_mismatch.hpp's summaries of every hit on its own, then every bucket's records settled in order
// -- on the match codes, every array of the size the library gives it.  tests/test_mismatch_cases.py compares the two;
// emul_mismatch_main.cpp runs the decomposition alone under the sanitizers.
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../lastz_amd/csrc/lz_mismatch.hpp"

namespace {

bool mismatch(const int8_t* mb, u8 a, u8 b) { return mb[a] != mb[b] || mb[a] < 0 || mb[b] < 0; }     // :3517-3519

// the match codes of one sequence as the library lays them out (k_pack2): base i at bit i + LZ_PAD2, everything else masked;
// and its bytes as a SeqSlot holds them (LZ_SEQ_PAD bytes on either side)
struct Codes {
    std::vector<u8> two, spc, raw;
    Codes(const u8* s, u32 len, const int8_t* mb)
    {
        u8 cls[256];
        lz_exact_cls(mb, cls);
        const size_t nmask = ((size_t)len + 2 * LZ_PAD2 + 7) / 8 + 16;
        two.assign(nmask * 2 + 96, 0); spc.assign(nmask + 96, 0xFF);
        raw.assign((size_t)len + 2 * LZ_SEQ_PAD, 0);
        if (len) memcpy(raw.data() + LZ_SEQ_PAD, s, len);
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

// counters: [0] too_many: E > M; [1] seed_mm: 0 < E <= M; [2] clipped: the left scan ended at diagEnd; [3] nul_left: ... at a
// NUL; [4] start: ... at the start of a sequence; [5] shortfall: right mismatches were skipped; [6] right_stop: the right scan
// ended at a NUL or an end of a sequence; [7] dropped: the hit failed the drop test; [8] other_diagonal: of [2] those whose
// diagEnd was written from another diagonal of the bucket (the left stop came from that diagonal's extent); [9] past_cap: a scan read LZ_EX_CAP bases or more; [10] past_step: ... more
// than 2048.  dend_out: diagEnd as the search leaves it.
#define EMUL_MM_COUNTERS 11
extern "C" int emul_mismatch_serial(const u8* t, u32 tlen, const u8* q, u32 qlen, const int8_t* mb, u32 L, u32 M, s32 thr,
                                    const u32* pos1s, const u32* pos2s, u64 nhits, u32* rows /*[4 * nhits]*/, u64* n_rows,
                                    u64* counters /*[EMUL_MM_COUNTERS]*/, u32* dend_out /*[LZ_DIAG_SIZE]*/)
{
    std::vector<u32> dend(LZ_DIAG_SIZE, 0);
    std::vector<s32> from(LZ_DIAG_SIZE, 0);
    const s64 NONE = -(1ll << 40);                                                           // (a start may be -1: the position in front of base 0)
    u64 n = 0;
    memset(counters, 0, EMUL_MM_COUNTERS * sizeof(u64));
    for (u64 i = 0; i < nhits; i++) {
        const u32 pos1 = pos1s[i], pos2 = pos2s[i];
        const s64 diag = (s64)pos1 - (s64)pos2;
        const u32 h = (u32)diag & (LZ_DIAG_SIZE - 1);
        const bool other = dend[h] != 0 && from[h] != (s32)diag;
        if (dend[h] > pos2 - L) { counters[7]++; continue; }                                     // :1113
        // the window, from its last base to its first (:3512-3525); positions are the query's
        u32 E = 0;
        s64 extent = NONE;
        bool too_many = false;
        for (s64 s = (s64)pos2 - 1; s >= (s64)pos2 - (s64)L; s--)
            if (mismatch(mb, t[s + diag], q[s])) { extent = s; if (++E > M) { too_many = true; break; } }
        if (too_many) {                                                                          // :3754-3777
            counters[0]++;
            if ((u32)extent > dend[h]) { dend[h] = (u32)extent; from[h] = (s32)diag; }
            continue;
        }
        if (E) counters[1]++;
        const u32 K = M + 1 - E;
        // to the left (:3535-3608): starts, the nearest first
        std::vector<s64> starts;
        s64 s = (s64)pos2 - (s64)L;
        const s64 stopl = (s64)dend[h] + diag > 0 ? (s64)dend[h] : -diag;
        while (s >= stopl) {
            if (s == stopl) {
                s--;
                if (dend[h] != 0 && (s64)dend[h] + diag > 0) { counters[2]++; if (other) counters[8]++; } else counters[4]++;
                break;
            }
            s--;
            const u8 n1 = t[s + diag], n2 = q[s];
            if (n1 == 0 || n2 == 0) { counters[3]++; break; }
            if (mismatch(mb, n1, n2)) { starts.push_back(s); if (starts.size() == K) break; }
        }
        const u64 read_left = (u64)((s64)pos2 - (s64)L - s);
        if (starts.size() < K) starts.push_back(s);
        u32 shortfall = K - (u32)starts.size();
        if (shortfall) counters[5]++;
        // to the right (:3616-3686): the byte at the end of a sequence is its terminating NUL
        s = (s64)pos2 - 1;
        const s64 stopr = (s64)tlen - diag < (s64)qlen ? (s64)tlen - diag : (s64)qlen;
        size_t at = starts.size() - 1;                                                           // the leftmost start
        s64 best = 0, left = NONE, right = NONE;
        bool enough = false;
        while (s < stopr) {
            s++;
            const u8 n1 = s + diag == (s64)tlen ? 0 : t[s + diag], n2 = s == (s64)qlen ? 0 : q[s];
            if (n1 == 0 || n2 == 0) break;
            if (mismatch(mb, n1, n2)) {
                if (extent == NONE) extent = s;
                if (shortfall > 0) { shortfall--; continue; }
                const s64 len = s - starts[at];
                if (len > best) { best = len; left = starts[at]; right = s; }
                if (at-- == 0) { enough = true; break; }
            }
        }
        if (!enough) {
            counters[6]++;
            if (extent == NONE) extent = s;
            const s64 len = s - starts[at];
            if (len > best) { left = starts[at]; right = s; }                                    // (bestLength stays: :3681-3685)
        }
        const u64 read_right = (u64)(s - (s64)pos2 + 1);
        if (read_left >= LZ_EX_CAP || read_right >= LZ_EX_CAP) counters[9]++;
        if (read_left > 2048 || read_right > 2048) counters[10]++;
        if (left == NONE) return 1;                                                              // :3688
        const u32 length = (u32)(right - left - 1);
        if (length >= (u32)thr) extent = right + 1;                                              // :3703
        if ((u32)extent > dend[h]) { dend[h] = (u32)extent; from[h] = (s32)diag; }
        if (length >= (u32)thr) { u32* r = rows + 4 * n++; r[0] = (u32)(right + diag); r[1] = (u32)right; r[2] = length; r[3] = length; }
    }
    *n_rows = n;
    if (dend_out) memcpy(dend_out, dend.data(), (size_t)LZ_DIAG_SIZE * 4);
    return 0;
}

// form[i]: the summary of hit i -- 0 FAST with E > M, 1 FAST with E <= M, 2 SLOW
extern "C" int emul_mismatch_decomposed(const u8* t, u32 tlen, const u8* q, u32 qlen, const int8_t* mb, u32 L, u32 M, s32 thr,
                                        const u32* pos1s, const u32* pos2s, u64 nhits, u32* rows /*[4 * nhits]*/, u64* n_rows,
                                        u8* form /*[nhits]*/, u32* dend_out /*[LZ_DIAG_SIZE]*/)
{
    const Codes tc(t, tlen, mb), qc(q, qlen, mb);
    LzMismatchParams P;
    P.X.t2 = tc.two.data(); P.X.tsp = tc.spc.data(); P.X.q2 = qc.two.data(); P.X.qsp = qc.spc.data();
    P.X.tlen = tlen; P.X.qlen = qlen; P.X.seed_len = L; P.X.thr = (u32)thr;
    P.traw = tc.raw.data() + LZ_SEQ_PAD; P.qraw = qc.raw.data() + LZ_SEQ_PAD; P.M = M;
    // phase A: every hit on its own
    std::vector<u64> rec(nhits);
    for (u64 i = 0; i < nhits; i++) {
        const u64 key = lz_hit_key(pos1s[i], pos2s[i]);
        const u32 summ = lz_mismatch_summary(P, key);
        if (!(summ & LZ_SUMM_SLOW) && summ > L + LZ_EX_CAP) return 2;                           // the payload's stated range
        form[i] = (summ & LZ_SUMM_SLOW) ? 2 : lz_mm_hit(P, pos1s[i], pos2s[i], 0u).E > M ? 0 : 1;
        rec[i] = lz_hit_record(key, summ);
    }
    // phase B: the buckets one after the other, each one's records in discovery order
    std::vector<u64> order(nhits);
    for (u64 i = 0; i < nhits; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](u64 a, u64 b) { return ((pos1s[a] - pos2s[a]) & 0xFFFFu) < ((pos1s[b] - pos2s[b]) & 0xFFFFu); });
    struct Found { u64 at; LzHspRec r; };
    std::vector<Found> found;
    if (dend_out) memset(dend_out, 0, (size_t)LZ_DIAG_SIZE * 4);
    u32 dend = 0, cur = 0xFFFFFFFFu;
    for (u64 k = 0; k < nhits; k++) {
        const u64 i = order[k];
        const u32 h = (pos1s[i] - pos2s[i]) & 0xFFFFu;
        if (h != cur) { cur = h; dend = 0; }
        lz_mismatch_settle_record(P, rec[i], h, dend, [&](const LzHspRec& r) { found.push_back({ i, r }); });
        if (dend_out) dend_out[h] = dend;
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
