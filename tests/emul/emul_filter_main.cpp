// emul_filter_main.cpp -- emul_filter_codes in a program of its own, for a build with -fsanitize=address,undefined
// (tests/test_filter_cases.py compiles and runs it): lz_filter.hpp's 9-byte loads on arrays of exactly the sizes the library
// allocates on the device (emul_exact.cpp's Codes), every input in a heap block of its own length.
//   emul_filter_main t.bin q.bin match_bits.bin pos1.bin pos2.bin L positions min_matches max_transversions
//     ->   one hit per line: kept matches transversions
#include <stdio.h>
#include <stdlib.h>
#include "emul_filter.cpp"

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
    if (argc != 10) { fprintf(stderr, "usage: %s t q match_bits pos1 pos2 L positions min_matches max_transversions\n", argv[0]); return 2; }
    const std::vector<u8> t = slurp(argv[1]), q = slurp(argv[2]), mb = slurp(argv[3]), b1 = slurp(argv[4]), b2 = slurp(argv[5]);
    if (mb.size() != 256 || b1.size() != b2.size() || b1.size() % 4) { fprintf(stderr, "bad input sizes\n"); return 2; }
    const u64 nhits = b1.size() / 4;
    std::vector<u32> p1(nhits), p2(nhits);
    if (nhits) { memcpy(p1.data(), b1.data(), b1.size()); memcpy(p2.data(), b2.data(), b2.size()); }
    std::vector<u8> keeps(nhits ? nhits : 1), counts(2 * (nhits ? nhits : 1));
    const int rc = emul_filter_codes(t.data(), (u32)t.size(), q.data(), (u32)q.size(), (const int8_t*)mb.data(), (u32)atoi(argv[6]),
                                     (u32)strtoul(argv[7], nullptr, 0), (s32)atoi(argv[8]), (s32)atoi(argv[9]), p1.data(), p2.data(), nhits,
                                     keeps.data(), counts.data());
    if (rc) { fprintf(stderr, "emul_filter_codes: %d\n", rc); return 1; }
    for (u64 k = 0; k < nhits; k++) printf("%u %u %u\n", keeps[k], counts[2 * k], counts[2 * k + 1]);
    return 0;
}
