// A stand-alone program (its own main) over jpezy_amd/csrc/jpezy_tensor_layout.h -- the host arithmetic of the tensor output (the placement
// rule of four element strides, the band of scale / bias values, scale / bias from mean / std) -- for a sanitizer run on the CPU:
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I jpezy_amd/csrc tools/sanitize/tensor_layout_program.cpp \
//         -o /tmp/tensor_layout && /tmp/tensor_layout          # "N checks, 0 wrong" and no sanitizer report
//
// The cases are the refusals of tests/test_tensor_abi.py, extents of 65535 in both axes with n = 2^31 - 1, strides at the edge of 63 bits
// and sums beyond 64, and every stride quadruple in 0..7 for a [2, 3, 2, 3] tensor against a brute-force count of distinct offsets.
#include "jpezy_tensor_layout.h"

#include <cstdio>
#include <limits>
#include <set>

using namespace jpezy_host;

static int checks = 0, wrong = 0;

static void expect(bool ok, const char* what)
{
    ++checks;
    if (!ok) { ++wrong; std::printf("WRONG: %s\n", what); }
}

static TensorLayoutVerdict lay(long long n, long long c, long long h, long long w, long long sn, long long sc, long long sh, long long sw, size_t cap)
{
    const long long e[4] = { n, c, h, w }, s[4] = { sn, sc, sh, sw };
    return tensor_layout_check(e, s, cap);
}

int main()
{
    // [2, 3, 4, 5]: the cases of the CPU test
    expect(lay(2, 3, 4, 5, 60, 20, 5, 1, 120) == kTensorFits, "NCHW tight");
    expect(lay(2, 3, 4, 5, 60, 1, 15, 3, 120) == kTensorFits, "NHWC tight");
    expect(lay(2, 3, 4, 5, 3, 1, 30, 6, 120) == kTensorFits, "[H, W, n, C]");
    expect(lay(2, 3, 4, 5, 64, 21, 5, 1, 126) == kTensorFits, "padded, at equality");
    expect(lay(2, 3, 4, 5, 64, 21, 5, 1, 125) == kTensorNoSpace, "padded, one short");
    expect(lay(2, 3, 4, 5, 60, 20, 5, 1, 119) == kTensorNoSpace, "one short");
    expect(lay(2, 3, 4, 5, 60, 20, 5, 1, 0) == kTensorNoSpace, "cap 0");
    expect(lay(2, 3, 4, 5, 60, 20, 5, -1, 120) == kTensorNegative, "negative sw");
    expect(lay(2, 3, 4, 5, std::numeric_limits<long long>::min(), 20, 5, 1, 120) == kTensorNegative, "most negative sn");
    expect(lay(2, 3, 4, 5, 60, 20, 4, 1, 120) == kTensorOverlap, "sh = out_w - 1");
    expect(lay(2, 3, 4, 5, 60, 20, 5, 0, 120) == kTensorOverlap, "sw = 0");
    expect(lay(2, 3, 4, 5, 0, 20, 5, 1, 120) == kTensorOverlap, "sn = 0");
    expect(lay(2, 3, 4, 5, 59, 20, 5, 1, 120) == kTensorOverlap, "sn one short");
    expect(lay(2, 3, 4, 5, 1, 1, 1, 1, 120) == kTensorOverlap, "all one");
    expect(lay(1, 1, 1, 1, 0, 0, 0, 0, 1) == kTensorFits, "one element, strides not looked at");
    expect(lay(1, 1, 1, 1, 7, 7, 7, 7, 0) == kTensorNoSpace, "one element, no room");
    // sums beyond 64 bits, strides at the edge of 63
    const long long big = std::numeric_limits<long long>::max();
    const size_t all = std::numeric_limits<size_t>::max();
    expect(lay(2, 3, 4, 5, 12, 4, 1, 1ll << 62, all) == kTensorNoSpace, "4 * 2^62");
    expect(lay(2, 3, 4, 5, big, 20, 5, 1, all) == kTensorFits, "sn = 2^63 - 1");
    expect(lay(2147483647, 3, 65535, 65535, big, big, big, big, all) == kTensorOverlap, "every stride 2^63 - 1");
    expect(lay(2147483647, 3, 65535, 65535, 1, 2147483647ll, 3 * 2147483647ll, 3 * 2147483647ll * 65535, all) == kTensorNoSpace,
           "n innermost, extents of 65535: distinct, and beyond 64 bits");
    // extents of 65535, n = 2
    const long long E = 65535;
    expect(lay(2, 3, E, E, 3 * E * E, E * E, E, 1, (size_t)(6 * E * E)) == kTensorFits, "65535 x 65535 NCHW");
    expect(lay(2, 3, E, E, 3 * E * E, E * E, E, 1, (size_t)(6 * E * E - 1)) == kTensorNoSpace, "65535 x 65535 NCHW, one short");
    expect(lay(2, 3, E, E, 3 * E * E, 1, 3 * E, 3, (size_t)(6 * E * E)) == kTensorFits, "65535 x 65535 NHWC");
    expect(lay(2, 3, E, E, 3 * E * E, E * E, E - 1, 1, (size_t)(6 * E * E)) == kTensorOverlap, "65535 x 65535, sh = out_w - 1");
    // brute force: the rule never admits two index tuples at one offset, and its fit is the largest offset + 1
    const long long ext[4] = { 2, 3, 2, 3 };
    for (long long a = 0; a < 8; ++a)
        for (long long b = 0; b < 8; ++b)
            for (long long c = 0; c < 8; ++c)
                for (long long d = 0; d < 8; ++d) {
                    const long long st[4] = { a, b, c, d };
                    std::set<long long> offs;
                    long long top = 0;
                    for (long long i = 0; i < ext[0]; ++i)
                        for (long long j = 0; j < ext[1]; ++j)
                            for (long long k = 0; k < ext[2]; ++k)
                                for (long long l = 0; l < ext[3]; ++l) {
                                    const long long o = i * a + j * b + k * c + l * d;
                                    offs.insert(o);
                                    if (o > top) top = o;
                                }
                    const TensorLayoutVerdict v = tensor_layout_check(ext, st, (size_t)top + 1);
                    expect(v != kTensorFits || offs.size() == 36, "an admitted overlap");
                    expect(v != kTensorNoSpace, "fit at the largest offset + 1");
                    if (v == kTensorFits) expect(tensor_layout_check(ext, st, (size_t)top) == kTensorNoSpace, "fit one short");
                }
    // the band
    expect(tensor_value_in_band(0.0f) && tensor_value_in_band(-0.0f) && tensor_value_in_band(0x1p-100f) && tensor_value_in_band(-0x1p100f), "band: inside");
    expect(!tensor_value_in_band(0x1p-101f) && !tensor_value_in_band(0x1p101f) && !tensor_value_in_band(1e-45f), "band: outside");
    expect(!tensor_value_in_band(std::numeric_limits<float>::infinity()) && !tensor_value_in_band(std::numeric_limits<float>::quiet_NaN()), "band: inf, nan");
    // normalisation
    const double mean[3] = { 0.485, 0.456, 0.406 }, sd[3] = { 0.229, 0.224, 0.225 };
    float scale[3] = { -7, -7, -7 }, bias[3] = { -7, -7, -7 };
    expect(tensor_normalization(3, mean, sd, scale, bias), "normalisation");
    for (int c = 0; c < 3; ++c) expect(scale[c] == (float)(1.0 / (255.0 * sd[c])) && bias[c] == (float)(-mean[c] / sd[c]), "normalisation values");
    const double zero[3] = { 0.229, 0.0, 0.225 }, inf[3] = { 0.229, std::numeric_limits<double>::infinity(), 0.225 },
                 nan[3] = { std::numeric_limits<double>::quiet_NaN(), 0.224, 0.225 };
    float s2[3] = { -7, -7, -7 }, b2[3] = { -7, -7, -7 };
    expect(!tensor_normalization(3, mean, zero, s2, b2) && !tensor_normalization(3, mean, inf, s2, b2) && !tensor_normalization(3, mean, nan, s2, b2) &&
               !tensor_normalization(3, nan, sd, s2, b2) && !tensor_normalization(3, inf, sd, s2, b2),
           "normalisation refusals");
    expect(s2[0] == -7 && s2[2] == -7 && b2[0] == -7 && b2[2] == -7, "a refused normalisation writes nothing");
    const double tiny[1] = { 1e-320 }, huge[1] = { 1e300 }, m1[1] = { 1e300 };
    expect(tensor_normalization(1, m1, tiny, s2, b2) && tensor_normalization(1, m1, huge, s2, b2), "normalisation at the ends of binary64");
    std::printf("%d checks, %d wrong\n", checks, wrong);
    return wrong ? 1 : 0;
}
