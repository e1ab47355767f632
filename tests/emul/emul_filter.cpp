// emul_filter.cpp -- the seed-hit filter of lastz --filter on the CPU, for tests/filter_cases.py:
//   * filter_seed_hit_by_subs (src/seed_search.c:2346-2411) transcribed byte by byte;
//   * lz_filter.hpp's predicate, the one k_filter_mark compiles, on match codes laid out as the library lays them out
//     (emul_exact.cpp's Codes: arrays of exactly the sizes the device allocations have);
//   * a serial X-drop pass over a given hit list: per hit, in order, the drop test (:1113), then lz_reextend with the bucket's
//     diagEnd; entropy, threshold and the reporter's order by lzh_finish_hsps, as for every X-drop search.
// Never linked into liblzgpu.so.
#include <string.h>
#include <vector>
#include "../../lastz_amd/csrc/lz_filter.hpp"
#include "../../lastz_amd/csrc/lz_host.hpp"
#include "emul_exact.cpp"                           // Codes

// verdict[i]: 0 kept, 1 not enough matches (:2403), 2 too many transversions (:2405); counts[2 i], counts[2 i + 1]: the hit's
// matches and transversions.  positions: lz_hit_filter's; `cares`: hp->filterPattern is set (the loop that walks the pattern,
// :2361-2383), otherwise the whole window right to left (:2384-2399; positions must then be the L low bits).
extern "C" int emul_filter_bytes(const u8* t, const u8* q, const int8_t* mb, u32 L, u32 positions, int cares, s32 min_matches, s32 max_tv,
                                 const u32* pos1s, const u32* pos2s, u64 nhits, u8* verdict, u8* counts)
{
    if (!cares && positions != (L >= 32 ? 0xFFFFFFFFu : (1u << L) - 1u)) return 1;
    for (u64 i = 0; i < nhits; i++) {
        const u8* scan1 = t + pos1s[i];
        const u8* scan2 = q + pos2s[i];
        int matches = 0, transversions = 0;
        if (cares) {
            scan1 -= L; scan2 -= L;
            for (u32 k = 0; k < L; k++) {
                if ((positions >> k) & 1u) {                    // *(pScan++) != '0'
                    // (a NUL counts as a transversion: hp->charToBits[0] is -1 in the reference; lz_hit_filter says so whatever the table holds)
                    const int8_t bits1 = *scan1 ? mb[*scan1] : -1, bits2 = *scan2 ? mb[*scan2] : -1;
                    if (bits1 < 0 || bits2 < 0) transversions++;
                    else if (bits1 == bits2) matches++;
                    else if (((bits1 ^ bits2) & 1) == 1) transversions++;
                }
                scan1++; scan2++;
            }
        } else {
            for (u32 remaining = L; remaining > 0; remaining--) {
                --scan1; --scan2;
                const int8_t bits1 = *scan1 ? mb[*scan1] : -1, bits2 = *scan2 ? mb[*scan2] : -1;
                if (bits1 < 0 || bits2 < 0) transversions++;
                else if (bits1 == bits2) matches++;
                else if (((bits1 ^ bits2) & 1) == 1) transversions++;
            }
        }
        counts[2 * i] = (u8)matches; counts[2 * i + 1] = (u8)transversions;
        verdict[i] = matches < min_matches ? 1 : (max_tv >= 0 && transversions > max_tv) ? 2 : 0;
    }
    return 0;
}

// the same through lz_filter_counts / lz_filter_keeps; keeps[i]: 1 kept, 0 rejected
extern "C" int emul_filter_codes(const u8* t, u32 tlen, const u8* q, u32 qlen, const int8_t* mb, u32 L, u32 positions, s32 min_matches, s32 max_tv,
                                 const u32* pos1s, const u32* pos2s, u64 nhits, u8* keeps, u8* counts)
{
    const Codes tc(t, tlen, mb), qc(q, qlen, mb);
    LzFilterParams F;
    F.t2 = tc.two.data(); F.tsp = tc.spc.data(); F.q2 = qc.two.data(); F.qsp = qc.spc.data();
    F.pos_spread = lz_filter_spread(positions); F.seed_len = L; F.min_matches = min_matches; F.max_transversions = max_tv;
    for (u64 i = 0; i < nhits; i++) {
        if (pos1s[i] < L || pos2s[i] < L || pos1s[i] > tlen || pos2s[i] > qlen) return 1;
        const LzFilterCounts c = lz_filter_counts(F, pos1s[i], pos2s[i]);
        counts[2 * i] = (u8)c.matches; counts[2 * i + 1] = (u8)c.transversions;
        keeps[i] = lz_filter_keeps_key(F, lz_hit_key(pos1s[i], pos2s[i])) ? 1 : 0;
    }
    return 0;
}

// process_for_simple_hit with gfExtend == gfexXDrop over the hits given, one after the other (src/seed_search.c:1056-1192):
// rows [4 * n_rows] = pos1, pos2, length, score of the HSPs in the reporter's order; counters: [0] extensions, [1] bp extended
extern "C" int emul_filter_xdrop(const u8* t, u32 tlen, const u8* q, u32 qlen, const int8_t* ctb, const s32* sub, s32 xdrop, s32 thr, int entropic,
                                 const char* pattern, int with_trans, const u32* pos1s, const u32* pos2s, u64 nhits,
                                 u32* rows /*[4 * nhits]*/, u64* n_rows, u64* counters /*[2]*/)
{
    lz_seed_desc desc; LzSeedDev sd;
    int rc = lzgpu_seed_from_pattern(pattern, with_trans, &desc); if (rc) return rc;
    if ((rc = lzh_seed_to_dev(&desc, sd))) return rc;
    u8 rowc[256], colc[256], cls[256]; s32 tab[LZ_NCLASS * LZ_NCLASS];
    if ((rc = lzh_score_classes(sub, rowc, colc, tab))) return rc;
    std::vector<u8> tcode((size_t)tlen + 2 * LZ_SEQ_PAD, LZ_CODE_INVALID), qcode((size_t)qlen + 2 * LZ_SEQ_PAD, LZ_CODE_INVALID);
    lzh_make_cls(rowc, ctb, cls); for (u32 i = 0; i < tlen; i++) tcode[LZ_SEQ_PAD + i] = cls[t[i]];
    lzh_make_cls(colc, ctb, cls); for (u32 i = 0; i < qlen; i++) qcode[LZ_SEQ_PAD + i] = cls[q[i]];
    LzExtendParams P; memset(&P, 0, sizeof(P));
    P.tcode = tcode.data() + LZ_SEQ_PAD; P.tlen = tlen; P.qcode = qcode.data() + LZ_SEQ_PAD; P.qlen = qlen;
    P.xdrop = xdrop; P.min_score = thr; P.seed_len = (u32)sd.length;
    std::vector<u32> dend(LZ_DIAG_SIZE, 0);
    std::vector<LzHspRec> recs;
    u64 n_ext = 0, n_bp = 0;
    for (u64 i = 0; i < nhits; i++) {
        const u32 pos2 = pos2s[i];
        const s32 diag = (s32)(pos1s[i] - pos2);
        const u32 h = (u32)diag & (LZ_DIAG_SIZE - 1);
        if (dend[h] > pos2 - P.seed_len) continue;              // :1113
        n_ext++;
        dend[h] = lz_reextend(P, tab, pos2, diag, dend[h], n_bp, [&](const LzHspRec& r) { recs.push_back(r); });
    }
    std::vector<lz_hsp> fin;
    if ((rc = lzh_finish_hsps(recs.data(), (u32)recs.size(), t, q, sd, ctb, thr, entropic, fin, nullptr, nullptr))) return rc;
    for (size_t k = 0; k < fin.size(); k++) { u32* r = rows + 4 * k; r[0] = fin[k].pos1; r[1] = fin[k].pos2; r[2] = fin[k].length; r[3] = (u32)fin[k].score; }
    *n_rows = fin.size(); counters[0] = n_ext; counters[1] = n_bp;
    return 0;
}
