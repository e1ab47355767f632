// emul_mismatch_main.cpp -- emul_mismatch_decomposed in a program of its own, for a build with -fsanitize=address,undefined
// (tests/test_mismatch_cases.py compiles and runs it): lz_mismatch.hpp on arrays of exactly the sizes the library allocates
// on the device (emul_mismatch.cpp's Codes), every input in a heap block of its own length.
//   emul_mismatch_main t.bin q.bin match_bits.bin pos1.bin pos2.bin L M thr   ->   one HSP per line: pos1 pos2 length score
#include <stdio.h>
#include <stdlib.h>
#include "emul_mismatch.cpp"

static std::vector<u8> slurp(const char* path)
{
    std::vector<u8> v;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    u8 buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
    v.shrink_to_fit();
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 9) { fprintf(stderr, "usage: %s t q match_bits pos1 pos2 L M thr\n", argv[0]); return 2; }
    const std::vector<u8> t = slurp(argv[1]), q = slurp(argv[2]), mb = slurp(argv[3]), b1 = slurp(argv[4]), b2 = slurp(argv[5]);
    if (mb.size() != 256 || b1.size() != b2.size() || b1.size() % 4) { fprintf(stderr, "bad input sizes\n"); return 2; }
    const u64 nhits = b1.size() / 4;
    std::vector<u32> p1(nhits), p2(nhits), rows(4 * (nhits ? nhits : 1)), dend(LZ_DIAG_SIZE);
    if (nhits) { memcpy(p1.data(), b1.data(), b1.size()); memcpy(p2.data(), b2.data(), b2.size()); }
    std::vector<u8> form(nhits ? nhits : 1);
    u64 n = 0;
    const int rc = emul_mismatch_decomposed(t.data(), (u32)t.size(), q.data(), (u32)q.size(), (const int8_t*)mb.data(),
                                            (u32)atoi(argv[6]), (u32)atoi(argv[7]), (s32)atoi(argv[8]),
                                            p1.data(), p2.data(), nhits, rows.data(), &n, form.data(), dend.data());
    if (rc) { fprintf(stderr, "emul_mismatch_decomposed: %d\n", rc); return 1; }
    for (u64 k = 0; k < n; k++) printf("%u %u %u %u\n", rows[4 * k], rows[4 * k + 1], rows[4 * k + 2], rows[4 * k + 3]);
    return 0;
}
