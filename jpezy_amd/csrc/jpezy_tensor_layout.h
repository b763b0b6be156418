// jpezy_tensor_layout.h -- the host arithmetic of the tensor output of the resized batch of windows (include/jpezy_hip.h, BATCH OF WINDOWS,
// TENSOR OUTPUT): the placement rule of four element strides, the band of scale / bias values, and scale / bias from mean / std.  Plain host
// C++, no HIP, so that a stand-alone program can run it under a host sanitizer.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace jpezy_host {

enum TensorLayoutVerdict { kTensorFits = 0, kTensorNegative = 1, kTensorOverlap = 2, kTensorNoSpace = 3 };

// extents {n, C, out_h, out_w} (all >= 1) with strides {sn, sc, sh, sw} in elements.  The dimensions of extent > 1, sorted by stride: the
// smallest stride is >= 1 and every other one >= the stride before it times that dimension's extent -- then no two index tuples name one
// element.  Fit: sum (extent - 1) * stride + 1 <= cap_elems.  128-bit sums: a stride may be anything up to 2^63 - 1.
inline TensorLayoutVerdict tensor_layout_check(const long long extent[4], const long long stride[4], size_t cap_elems)
{
    for (int d = 0; d < 4; ++d)
        if (stride[d] < 0) return kTensorNegative;
    int order[4], m = 0;
    for (int d = 0; d < 4; ++d)
        if (extent[d] > 1) order[m++] = d;
    for (int a = 1; a < m; ++a)                    // insertion sort by stride
        for (int b = a; b > 0 && stride[order[b]] < stride[order[b - 1]]; --b) { const int t = order[b]; order[b] = order[b - 1]; order[b - 1] = t; }
    unsigned __int128 need = 1;                    // the smallest stride the next dimension may have
    unsigned __int128 last = 0;                    // offset of the last element
    for (int a = 0; a < m; ++a) {
        const unsigned __int128 s = (unsigned __int128)(unsigned long long)stride[order[a]], e = (unsigned __int128)(unsigned long long)extent[order[a]];
        if (s < need) return kTensorOverlap;
        need = s * e;
        last += (e - 1) * s;
    }
    return last + 1 <= (unsigned __int128)cap_elems ? kTensorFits : kTensorNoSpace;
}

// 0, or finite with magnitude in [2^-100, 2^100]: then (float)byte * scale + bias neither overflows nor gives a subnormal or a NaN in binary32
inline bool tensor_value_in_band(float v)
{
    if (v == 0.0f) return true;
    const float a = std::fabs(v);
    return std::isfinite(v) && a >= 0x1p-100f && a <= 0x1p100f;
}

// scale[c] = (float)(1 / (255 * std[c])), bias[c] = (float)(-mean[c] / std[c]); binary64, every operation separate.  false: a std that is
// zero or not finite, a mean that is not finite (nothing is written then)
inline bool tensor_normalization(int C, const double* mean, const double* std_, float* scale, float* bias)
{
#pragma clang fp contract(off)
    for (int c = 0; c < C; ++c)
        if (!std::isfinite(std_[c]) || std_[c] == 0.0 || !std::isfinite(mean[c])) return false;
    for (int c = 0; c < C; ++c) {
        const double d = 255.0 * std_[c];
        scale[c] = (float)(1.0 / d);
        const double m = -mean[c];
        bias[c] = (float)(m / std_[c]);
    }
    return true;
}

}  // namespace jpezy_host
