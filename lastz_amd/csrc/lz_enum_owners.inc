// lz_enum_owners.inc -- step 2 of the list enumeration of k_fill_hits2 and k_scan_hits2 (the scheme: lz_enum_place.inc): a fragment
// of text, included at the top of `for (u32 cs = 0; cs < T; cs += CAP)`, the loop over the pieces of a wave's concatenation.
//   expects   lane, sh, own (sh.own32 as unsigned short*), len[], E (lz_enum_place.inc), cs, tc (the piece is hits [cs, cs + tc) of
//             the concatenation), CAP (only through sh) and WORDS = CAP / 2 / 64, the 32-bit words of own[] per lane
//   defines   nothing the kernels use; leaves own[t], t < tc, = 1 + the id (lane * LZ_FILL_GROUP + probe) of the list holding hit cs + t
//   included  by k_fill_hits2 and k_scan_hits2, which go on with step 3 and end the piece with a fence of their own.
uint4* const mine = reinterpret_cast<uint4*>(sh.own32 + lane * WORDS);
#pragma unroll
for (int k = 0; k < WORDS / 4; k++) mine[k] = make_uint4(0u, 0u, 0u, 0u);
__atomic_signal_fence(__ATOMIC_SEQ_CST);
{
    u32 S = E;
#pragma unroll
    for (int p = 0; p < LZ_FILL_GROUP; p++) {
        const u32 l = len[p];
        if (l && S < cs + tc && S + l > cs) own[(S > cs ? S : cs) - cs] = (unsigned short)(1u + lane * LZ_FILL_GROUP + (u32)p);
        S += l;
    }
}
__atomic_signal_fence(__ATOMIC_SEQ_CST);
// prefix maximum over own[]: the lane's 2 * WORDS cells, then the lanes' last values, then the cells again
u32 wv[WORDS];
#pragma unroll
for (int k = 0; k < WORDS / 4; k++) { const uint4 v = mine[k]; wv[4 * k] = v.x; wv[4 * k + 1] = v.y; wv[4 * k + 2] = v.z; wv[4 * k + 3] = v.w; }
u32 segmax = 0;
#pragma unroll
for (int k = 0; k < WORDS; k++) { const u32 m2 = lz_umax(wv[k] & 0xFFFFu, wv[k] >> 16); segmax = lz_umax(segmax, m2); }
u32 sinc = segmax;
LZ_WAVE_SCAN_U32(sinc, segmax, lz_umax)
u32 run = lz_dpp_u32<0x138, 0xf, 0xf>(0u, sinc);    // wave_shr:1: the maximum of the lanes below
#pragma unroll
for (int k = 0; k < WORDS; k++) {
    const u32 a0 = lz_umax(wv[k] & 0xFFFFu, run), a1 = lz_umax(wv[k] >> 16, a0);
    wv[k] = a0 | (a1 << 16); run = a1;
}
#pragma unroll
for (int k = 0; k < WORDS / 4; k++) mine[k] = make_uint4(wv[4 * k], wv[4 * k + 1], wv[4 * k + 2], wv[4 * k + 3]);
__atomic_signal_fence(__ATOMIC_SEQ_CST);
