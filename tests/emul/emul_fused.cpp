// emul_fused.cpp -- TEST INFRASTRUCTURE: the per-entry target context of the fused scan kernel (lz_lut.hpp: lz_wctx_make,
// lz_wctx_windows) and the tagged hit record, run on the CPU, for tests/test_fused_scan_windows.py.
// Never linked into liblzgpu.so.
#include <string.h>
#include "../../lastz_amd/csrc/lz_lut.hpp"

// for every pos1[k]: the wctx entry as k_build_wctx makes it from the plain 2-bit array, and the two 16-byte windows
// k_scan_hits2 takes out of it
extern "C" void emul_wctx_windows(const u8* two, const u32* pos1, u32 n, u8* entries /*[n][32]*/, u8* left /*[n][16]*/, u8* right /*[n][16]*/)
{
    for (u32 k = 0; k < n; k++) {
        const LzWctx e = lz_wctx_make(two, pos1[k]);
        LzVec16 tl, tr;
        lz_wctx_windows(e, pos1[k], tl, tr);
        memcpy(entries + 32 * (size_t)k, &e, 32);
        memcpy(left + 16 * (size_t)k, &tl, 16);
        memcpy(right + 16 * (size_t)k, &tr, 16);
    }
}

// tagged[k] = the record k_scan_hits2 stores, plain[k] = lz_hit_record, tag[k] / untagged[k] = what k_hist2 / k_partition<true> make of it
extern "C" void emul_tagged_records(const u64* key, const u32* summ, u32 n, u64* tagged, u64* plain, u32* tag, u64* untagged)
{
    for (u32 k = 0; k < n; k++) {
        tagged[k] = lz_hit_record_tagged(key[k], summ[k]);
        plain[k] = lz_hit_record(key[k], summ[k]);
        tag[k] = LZ_REC_TAG(tagged[k]);
        untagged[k] = LZ_REC_UNTAG(tagged[k]);
    }
}
