// exif_fuzz <cases.bin> <valid.bin>... -- the EXIF orientation parser (jpezy_amd/csrc/jpezy_exif.h: plain C++, reads untrusted offsets)
// as a stand-alone CPU program, built with -fsanitize=address,undefined by tests/test_orient_abi.py.  cases.bin: records of
// [u32 length][u32 expected orientation][bytes], little-endian; every further file is a valid tagged stream (orientation 6) that is
// run whole, cut at every length, and with every byte replaced by every value.  Every input is copied into a heap block of exactly its
// size, so a read outside data[0, len) is a heap-buffer-overflow.  Exit 0: every expectation held and every answer was in 1..8.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../jpezy_amd/csrc/jpezy_exif.h"

static std::vector<uint8_t> slurp(const char* p)
{
    std::vector<uint8_t> v;
    if (FILE* f = std::fopen(p, "rb")) { int c; while ((c = std::fgetc(f)) != EOF) v.push_back((uint8_t)c); std::fclose(f); }
    return v;
}
static int run(const uint8_t* d, size_t n)
{
    uint8_t* h = n ? (uint8_t*)std::malloc(n) : nullptr;
    if (n) std::memcpy(h, d, n);
    const int o = jpezy_exif::jpeg_orientation(h, n);
    std::free(h);
    if (o < 1 || o > 8) { std::printf("out of range: %d\n", o); std::exit(2); }
    return o;
}
int main(int argc, char** argv)
{
    long calls = 0, wrong = 0;
    const std::vector<uint8_t> cases = slurp(argv[1]);
    for (size_t at = 0; at + 8 <= cases.size();) {
        uint32_t len, want;
        std::memcpy(&len, &cases[at], 4); std::memcpy(&want, &cases[at + 4], 4);
        at += 8;
        if ((uint32_t)run(cases.data() + at, len) != want) ++wrong;
        ++calls;
        at += len;
    }
    std::printf("%ld recorded cases, %ld wrong\n", calls, wrong);
    if (run(nullptr, 0) != 1 || jpezy_exif::jpeg_orientation(nullptr, 100) != 1) ++wrong;
    for (int k = 2; k < argc; ++k) {
        const std::vector<uint8_t> v = slurp(argv[k]);
        if (run(v.data(), v.size()) != 6) ++wrong;
        long tagged = 0;
        for (size_t n = 0; n <= v.size(); ++n) { tagged += run(v.data(), n) != 1; ++calls; }          // every truncation
        std::vector<uint8_t> m = v;
        for (size_t i = 0; i < v.size(); ++i)                                                         // every single-byte mutation
            for (int b = 0; b < 256; ++b) { m[i] = (uint8_t)b; tagged += run(m.data(), m.size()) != 1; ++calls; m[i] = v[i]; }
        std::printf("%s: %zu bytes, every truncation and every single-byte mutation; %ld of them still carry a tag\n", argv[k], v.size(), tagged);
    }
    std::printf("%ld calls, %ld wrong\n", calls, wrong);
    return wrong ? 1 : 0;
}
