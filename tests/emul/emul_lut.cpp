// emul_lut.cpp -- TEST INFRASTRUCTURE: the host routines that decide whether a search may scan through the look-up
// tables and that fill them (lz_host.cpp: lzh_lut_eligible, lzh_lut_build), callable from tests/test_scorings.py, which
// checks every entry against a plain statement of lz_lut.hpp's header comment.  Never linked into liblzgpu.so.
#include "../../lastz_amd/csrc/lz_lut.hpp"
#include "../../lastz_amd/csrc/lz_host.hpp"

extern "C" int emul_lut_eligible(const s32* sub, const int8_t* ctb, const u8* tocc, const u8* qocc, s32 xdrop, s32* M4 /*[16]*/)
{
    return lzh_lut_eligible(sub, ctb, tocc, qocc, xdrop, M4);
}

// out[2 * e] = ab, out[2 * e + 1] = sc of entry e (LZ_LUT_TOTAL entries: ascending, then descending)
extern "C" u32 emul_lut_build(const s32* M4, s32 xdrop, u32* out)
{
    static LzLutEntry tab[LZ_LUT_TOTAL];
    lzh_lut_build(M4, xdrop, tab);
    for (u32 e = 0; e < LZ_LUT_TOTAL; e++) { out[2 * e] = tab[e].ab; out[2 * e + 1] = tab[e].sc; }
    return LZ_LUT_TOTAL;
}
