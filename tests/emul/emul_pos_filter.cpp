// emul_pos_filter.cpp -- TEST INFRASTRUCTURE: the position filter of the seed stage (lastz --chores; lz_common.hpp:
// lz_window_self, lz_self_bounds in LZ_SELF_WINDOW mode, lz_clip_run(s), lz_count_hits_self_at, lz_fill_hits_self_at) run
// on the CPU, for tests/test_pos_filter_bounds.py.  Never linked into liblzgpu.so.
#include <string.h>
#include <vector>
#include "../../lastz_amd/csrc/lz_common.hpp"

// The raw hits of a whole query against the table (wstart / wpos: CSR, descending positions inside a word) under the
// target interval [t_start, t_end), or with filter == 0 every hit (lz_count_hits_at / lz_fill_hits_at):
//   cnt[pos2]     = the LZ_HD count of the position;  cnt_grp[pos2] = the kernels' way: the text k_fill_hits2 / k_scan_hits2
//                   compile (lz_enum_lists.inc: 16 lists clipped together);
//   keys          = the LZ_HD fill for pos2 = 0 .. qlen, one after the other (at most cap are written).
// Returns the number of keys; *survives = what lz_window_self said (0: nothing was clipped, nothing can survive).
extern "C" long long emul_pos_filter_hits(const u8* qcode, u32 qlen, u32 tlen, s32 length, s32 weight, s32 nparts, const s32* shift,
                                          const u32* mask, s32 nprobes, const u32* probe_xor, const u32* wstart, const u32* wpos,
                                          int filter, u32 t_start, u32 t_end, u32* cnt, u32* cnt_grp, u64* keys, u64 cap, int* survives)
{
    LzSeedDev sd;
    memset(&sd, 0, sizeof(sd));
    sd.length = length; sd.weight = weight; sd.nparts = nparts; sd.nprobes = nprobes;
    for (int k = 0; k < nparts; k++) { sd.shift[k] = shift[k]; sd.mask[k] = mask[k]; }
    for (int k = 0; k < nprobes; k++) sd.probe_xor[k] = probe_xor[k];
    LzSelfDev s = {};
    *survives = 1;
    if (filter) *survives = lz_window_self(t_start, t_end, (u32)length, tlen, s) ? 1 : 0;
    long long nk = 0;
    std::vector<u64> buf;
    for (u32 pos2 = 0; pos2 <= qlen; pos2++) {
        cnt[pos2] = cnt_grp[pos2] = 0;
        if (!*survives) continue;
        bool valid; u32 packed;
        if (!filter) {
            cnt[pos2] = cnt_grp[pos2] = lz_count_hits_at(qcode, pos2, 0, sd, wstart, valid, packed);
            if (!valid) continue;
            buf.assign(cnt[pos2], 0);
            lz_fill_hits_at(qcode, pos2, sd, wstart, wpos, buf.data());
        } else {
            cnt[pos2] = lz_count_hits_self_at(qcode, pos2, 0, sd, s, wstart, wpos, valid, packed);
            if (!valid) continue;
            const bool in = true, SELF = true; const u32 w_l = packed;
            u32 slo, shi, g = 0; lz_self_bounds(s, pos2, slo, shi);
            for (int r = 0; r < sd.nprobes; r += LZ_FILL_GROUP) {
#include "../../lastz_amd/csrc/lz_enum_lists.inc"
                g += total;
            }
            cnt_grp[pos2] = g;
            buf.assign(cnt[pos2], 0);
            lz_fill_hits_self_at(qcode, pos2, sd, s, wstart, wpos, buf.data());
        }
        for (u64 k : buf) { if ((u64)nk < cap) keys[nk] = k; nk++; }
    }
    return nk;
}
