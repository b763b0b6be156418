// jpezy_resize_taps.h -- the tap tables of the resized batch of windows (include/jpezy_hip.h, BATCH OF WINDOWS, RESIZED): plain host C++, no
// HIP, so that a stand-alone program can run it under a host sanitizer.  This is the only floating-point part of the resampling; every
// operation is a separate binary64 operation in the order the header states (no contraction into fused multiply-adds).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace jpezy_host {

struct ResizeTaps {
    int ksize = 0;                      // weights per output index
    std::vector<int> first, count;      // [out_size]
    std::vector<int32_t> weight;        // [out_size][ksize], zero behind count
};

// 2 * ceil(support) + 1; sizes in 1..65535 (the callers check)
inline int resize_ksize(int in_size, int out_size)
{
#pragma clang fp contract(off)
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale > 1.0 ? scale : 1.0;
    return 2 * (int)std::ceil(fs) + 1;
}

// weight == null: first and count only
inline void resize_taps_into(int in_size, int out_size, int ksize, int* first, int* count, int32_t* weight)
{
#pragma clang fp contract(off)
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale > 1.0 ? scale : 1.0;
    const double support = fs;
    const double ss = 1.0 / fs;
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
            double a = ((double)(j + lo) - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            w[(size_t)j] = a < 1.0 ? 1.0 - a : 0.0;
            sum += w[(size_t)j];
        }
        int32_t* row = weight + (size_t)i * (size_t)ksize;
        for (int j = 0; j < ksize; ++j) {
            if (j >= n) { row[j] = 0; continue; }
            const double k = sum != 0.0 ? w[(size_t)j] / sum : w[(size_t)j];
            row[j] = (int32_t)(0.5 + k * 4194304.0);
        }
    }
}

inline ResizeTaps resize_taps(int in_size, int out_size)
{
    ResizeTaps t;
    t.ksize = resize_ksize(in_size, out_size);
    t.first.resize((size_t)out_size);
    t.count.resize((size_t)out_size);
    t.weight.resize((size_t)out_size * (size_t)t.ksize);
    resize_taps_into(in_size, out_size, t.ksize, t.first.data(), t.count.data(), t.weight.data());
    return t;
}

}  // namespace jpezy_host
