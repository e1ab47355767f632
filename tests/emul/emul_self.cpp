// emul_self.cpp -- TEST INFRASTRUCTURE: the self-comparison filter of the seed stage (lz_common.hpp: lz_self_bounds,
// lz_clip_run(s), lz_count_hits_self_at, lz_fill_hits_self_at) run on the CPU, for tests/test_self_bounds.py.
// Never linked into liblzgpu.so.
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../lastz_amd/csrc/lz_common.hpp"

static LzSelfDev make_self(u32 mode, u32 L, u32 len2, u32 band, const u32* sep1, u32 n1, const u32* sep2, u32 n2)
{
    LzSelfDev s = {};
    s.mode = mode; s.L = L; s.len2 = len2; s.band = band;
    s.sep1 = sep1; s.n_sep1 = n1; s.sep2 = sep2; s.n_sep2 = n2;
    return s;
}

// [lo[k], hi[k]) for every pos2[k]
extern "C" void emul_self_bounds(u32 mode, u32 L, u32 len2, u32 band, const u32* sep1, u32 n1, const u32* sep2, u32 n2,
                                 const u32* pos2, u32 n, u32* lo, u32* hi)
{
    const LzSelfDev s = make_self(mode, L, len2, band, sep1, n1, sep2, n2);
    for (u32 k = 0; k < n; k++) lz_self_bounds(s, pos2[k], lo[k], hi[k]);
}

extern "C" void emul_clip_run(const u32* wpos, u32 a, u32 b, u32 lo, u32 hi, u32* out /*[2]: start, length*/)
{
    lz_clip_run(wpos, a, b, lo, hi, out[0], out[1]);
}

// A whole self search's raw hits on code bytes (bits 5-6 the base, bit 7 "not a seed byte"), for a contiguous seed of
// length L (2L bits) with the exact word and the L single-transition probes:
//   the table as k_table_words + the stable sort build it (descending positions inside a word);
//   cnt[pos2]  = lz_count_hits_self_at,  cnt_grp[pos2] = the kernels' way: the text k_fill_hits2 / k_scan_hits2 compile
//                (lz_enum_lists.inc: 16 lists clipped together), one probe group after the other;
//   keys       = lz_fill_hits_self_at for pos2 = L .. len, one after the other (at most cap);
//   all_keys   = lz_fill_hits_at (no filter), likewise.
// Returns the number of keys (clipped) and sets *n_all.
extern "C" long long emul_self_hits(const u8* tcode, const u8* qcode, u32 len, u32 L, u32 mode, u32 band,
                                    const u32* sep1, u32 n1, const u32* sep2, u32 n2,
                                    u32* cnt, u32* cnt_grp, u64* keys, u64* all_keys, u64 cap, long long* n_all)
{
    LzSeedDev sd;
    memset(&sd, 0, sizeof(sd));
    sd.length = (s32)L; sd.weight = (s32)(2 * L); sd.nparts = 1; sd.shift[0] = 0; sd.mask[0] = (u32)((1ull << (2 * L)) - 1);
    sd.nprobes = (s32)L + 1; sd.probe_xor[0] = 0;
    for (u32 k = 0; k < L; k++) sd.probe_xor[k + 1] = 2u << (2 * k);          // transitions: A<->G, C<->T
    const u32 nwords = 1u << sd.weight;
    std::vector<std::pair<u32, u32>> kv;
    for (u32 p = len; p >= L; p--) {
        u32 packed;
        if (lz_window_word(tcode, p, sd, packed)) kv.push_back({ packed, p });
        if (p == 0) break;
    }
    std::stable_sort(kv.begin(), kv.end(), [](const std::pair<u32, u32>& a, const std::pair<u32, u32>& b) { return a.first < b.first; });
    std::vector<u32> wstart_v(nwords + 1, 0), wpos_v(kv.size() + 1, 0);
    for (size_t i = 0; i < kv.size(); i++) { wstart_v[kv[i].first + 1]++; wpos_v[i] = kv[i].second; }
    for (u32 w = 0; w < nwords; w++) wstart_v[w + 1] += wstart_v[w];
    const LzSelfDev s = make_self(mode, L, len, band, sep1, n1, sep2, n2);
    const u32* const wstart = wstart_v.data(); const u32* const wpos = wpos_v.data();   // (the fragment's names)
    long long nk = 0, na = 0;
    std::vector<u64> buf;
    for (u32 pos2 = 0; pos2 <= len; pos2++) {
        bool valid; u32 packed;
        cnt[pos2] = lz_count_hits_self_at(qcode, pos2, 0, sd, s, wstart, wpos, valid, packed);
        u32 g = 0;
        if (valid) {
            const bool in = true, SELF = true; const u32 w_l = packed;
            u32 slo, shi; lz_self_bounds(s, pos2, slo, shi);
            for (int r = 0; r < sd.nprobes; r += LZ_FILL_GROUP) {
#include "../../lastz_amd/csrc/lz_enum_lists.inc"
                g += total;
            }
        }
        cnt_grp[pos2] = g;
        if (!valid) continue;
        buf.assign(cnt[pos2], 0);
        lz_fill_hits_self_at(qcode, pos2, sd, s, wstart, wpos, buf.data());
        for (u64 k : buf) { if ((u64)nk < cap) keys[nk] = k; nk++; }
        u32 full = lz_count_hits_at(qcode, pos2, 0, sd, wstart, valid, packed);
        buf.assign(full, 0);
        lz_fill_hits_at(qcode, pos2, sd, wstart, wpos, buf.data());
        for (u64 k : buf) { if ((u64)na < cap) all_keys[na] = k; na++; }
    }
    *n_all = na;
    return nk;
}
