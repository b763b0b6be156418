// jpezy_resize_taps.h -- the tap tables of the resized batch of windows (include/jpezy_hip.h, BATCH OF WINDOWS, RESIZED and its FILTERS): plain
// host C++, no HIP, so that a stand-alone program can run it under a host sanitizer.  This is the only floating-point part of the
// resampling; every operation is a separate binary64 operation in the order the header states (no contraction into fused multiply-adds).
// Of the four filters only Lanczos calls the C library (sin); the others are plain arithmetic.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace jpezy_host {

// the values of enum jpezy_filter (include/jpezy_hip.h)
enum { kFilterBilinear = 0, kFilterBox = 1, kFilterBicubic = 2, kFilterLanczos = 3 };
inline bool resize_filter_known(int filter) { return filter >= kFilterBilinear && filter <= kFilterLanczos; }

struct ResizeTaps {
    int ksize = 0;                      // weights per output index
    std::vector<int> first, count;      // [out_size]
    std::vector<int32_t> weight;        // [out_size][ksize], zero behind count
    bool fits = true;                   // the 32-bit accumulator condition holds for every output index
};

// fsup: the filter's support at ratio 1
inline double resize_filter_support(int filter)
{
    return filter == kFilterBox ? 0.5 : filter == kFilterBicubic ? 2.0 : filter == kFilterLanczos ? 3.0 : 1.0;
}

inline double resize_sinc(double x)
{
#pragma clang fp contract(off)
    if (x == 0.0) return 1.0;
    const double px = x * 3.14159265358979323846;
    return std::sin(px) / px;
}

// f(x) of the filter
inline double resize_filter_value(int filter, double x)
{
#pragma clang fp contract(off)
    switch (filter) {
    case kFilterBox: return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
    case kFilterBicubic: {
        const double a = -0.5;
        if (x < 0.0) x = -x;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
        if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
        return 0.0;
    }
    case kFilterLanczos: return -3.0 <= x && x < 3.0 ? resize_sinc(x) * resize_sinc(x / 3.0) : 0.0;
    default:
        if (x < 0.0) x = -x;
        return x < 1.0 ? 1.0 - x : 0.0;
    }
}

// 2 * ceil(support) + 1; sizes in 1..65535, a known filter (the callers check)
inline int resize_ksize(int filter, int in_size, int out_size)
{
#pragma clang fp contract(off)
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale > 1.0 ? scale : 1.0;
    const double support = resize_filter_support(filter) * fs;
    return 2 * (int)std::ceil(support) + 1;
}

// weight == null: first and count only.  false: the weights of some output index break the accumulator condition
// 255 * sum(K+) + 2^21 < 2^31, 255 * sum(K-) <= 2^31 - 2^21 (the tables are complete all the same)
inline bool resize_taps_into(int filter, int in_size, int out_size, int ksize, int* first, int* count, int32_t* weight)
{
#pragma clang fp contract(off)
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale > 1.0 ? scale : 1.0;
    const double support = resize_filter_support(filter) * fs;
    const double ss = 1.0 / fs;
    bool fits = true;
    std::vector<double> w((size_t)ksize);
    for (int i = 0; i < out_size; ++i) {
        const double center = ((double)i + 0.5) * scale;
        int lo = (int)(center - support + 0.5);
        if (lo < 0) lo = 0;
        int hi = (int)(center + support + 0.5);
        if (hi > in_size) hi = in_size;
        const int n = hi - lo;
        first[i] = lo;
        count[i] = n;
        if (!weight) continue;
        double sum = 0.0;
        for (int j = 0; j < n; ++j) {
            w[(size_t)j] = resize_filter_value(filter, ((double)(j + lo) - center + 0.5) * ss);
            sum += w[(size_t)j];
        }
        int32_t* row = weight + (size_t)i * (size_t)ksize;
        long long pos = 0, neg = 0;
        for (int j = 0; j < ksize; ++j) {
            if (j >= n) { row[j] = 0; continue; }
            const double k = sum != 0.0 ? w[(size_t)j] / sum : w[(size_t)j];
            row[j] = k < 0.0 ? (int32_t)(-0.5 + k * 4194304.0) : (int32_t)(0.5 + k * 4194304.0);
            if (row[j] < 0) neg -= row[j];
            else pos += row[j];
        }
        if (255 * pos + (1ll << 21) >= (1ll << 31) || 255 * neg > (1ll << 31) - (1ll << 21)) fits = false;
    }
    return fits;
}

inline ResizeTaps resize_taps(int filter, int in_size, int out_size)
{
    ResizeTaps t;
    t.ksize = resize_ksize(filter, in_size, out_size);
    t.first.resize((size_t)out_size);
    t.count.resize((size_t)out_size);
    t.weight.resize((size_t)out_size * (size_t)t.ksize);
    t.fits = resize_taps_into(filter, in_size, out_size, t.ksize, t.first.data(), t.count.data(), t.weight.data());
    return t;
}

// The largest number of source rows a tile of `tile` consecutive output indices spans: first[i0] .. first[i1] + count[i1], i0 a multiple
// of tile, i1 the tile's last index (first and first + count never decrease with the index).  What decides, per file, whether the two-pass
// tile of resample_kernel can hold the file's rows (jpezy_resample_core.h)
inline int resize_tile_span(const int* first, const int* count, int out_size, int tile)
{
    int span = 0;
    for (int i0 = 0; i0 < out_size; i0 += tile) {
        const int i1 = i0 + tile - 1 < out_size - 1 ? i0 + tile - 1 : out_size - 1;
        const int s = first[i1] + count[i1] - first[i0];
        if (s > span) span = s;
    }
    return span;
}

}  // namespace jpezy_host
