// emul_mask.cpp -- the masking pass of mask_kernels.hip on the CPU, for tests/table_mask_cases.py: the three kernels' per-lane
// logic (lz_mask.hpp, the functions the kernels compile) run as plain loops, one iteration per lane, over CSR arrays; the
// scan between them is a serial one.  Never linked into liblzgpu.so.
#include <stddef.h>
#include <vector>
#include "../../lastz_amd/csrc/lz_mask.hpp"

// wstart[nwords + 1] and wpos[num_words] are rewritten in place; iv: n pairs (start, end).  -> 0 and *kept, the entries that
// stay; 1 for an interval the library refuses (end <= start or end > tlen); 2 when a lane would leave its arrays
extern "C" int emul_table_mask(u32* wstart, u32 nwords, u32* wpos, u32 num_words, const u32* iv, u32 n, u32 L, u32 tlen, u32* kept)
{
    std::vector<u32> lo, hi, pre;
    u32 total = 0;
    for (u32 k = 0; k < n; k++) {
        const u32 s = iv[2 * k], e = iv[2 * k + 1];
        if (e <= s || e > tlen) return 1;
        u32 a, b;
        if (!lz_mask_range(s, e, L, a, b)) continue;
        lo.push_back(a); hi.push_back(b); pre.push_back(total);
        total += lz_mask_range_words(a, b);
    }
    pre.push_back(total);
    const u32 nr = (u32)lo.size();
    *kept = num_words;
    if (nr == 0 || num_words == 0) return 0;
    const size_t bit_words = (size_t)(tlen >> 5) + 1;
    std::vector<u32> bits(bit_words, 0u);
    for (u32 j = 0; j < total; j++) {                            // k_mask_bits
        const u32 r = lz_mask_range_of(pre.data(), nr, j);
        if (r >= nr || j < pre[r] || j >= pre[r + 1]) return 2;
        const u32 word = (lo[r] >> 5) + (j - pre[r]);
        if (word >= bit_words || word > (hi[r] >> 5)) return 2;
        bits[word] |= lz_mask_word_bits(lo[r], hi[r], word);     // (a whole word is stored, an end word OR-ed in: the same on one thread)
    }
    std::vector<u32> keep((size_t)num_words + 1), idx((size_t)num_words + 1), npos(num_words);
    for (u32 e = 0; e <= num_words; e++) {                       // k_mask_keep
        if (e < num_words && wpos[e] > tlen) return 2;
        keep[e] = e < num_words ? lz_mask_keeps(bits.data(), wpos[e]) : 0u;
    }
    u32 sum = 0;
    for (u32 e = 0; e <= num_words; e++) { idx[e] = sum; sum += keep[e]; }
    *kept = idx[num_words];
    if (*kept == num_words) return 0;
    const u32 lanes = num_words > nwords + 1 ? num_words : nwords + 1;
    for (u32 e = 0; e < lanes; e++) {                            // k_mask_move
        if (e < num_words && keep[e]) npos[idx[e]] = wpos[e];
        if (e <= nwords) { if (wstart[e] > num_words) return 2; wstart[e] = idx[wstart[e]]; }
    }
    for (u32 e = 0; e < *kept; e++) wpos[e] = npos[e];
    return 0;
}
