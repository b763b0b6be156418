// jpezy_kernels_resized_tensor.hip -- a batch of windows, resized, straight into a tensor (include/jpezy_hip.h, BATCH OF WINDOWS, TENSOR
// OUTPUT): resample_kernel<3>'s tiling, descriptor table, tap tables and tap loops (resample_four, jpezy_resample_core.h),
// and a store stage of its own.
//   resample_tensor_kernel<DT, C> : a thread holds the three bytes of its four output pixels in registers.  Channel c of pixel j becomes one
//       element: the byte itself (U8), or v = (float)byte * scale[c] + bias[c] in binary32, the multiplication and the addition rounded
//       separately (__fmul_rn, __fadd_rn: never one fused operation), stored as it is (F32), converted to binary16 round-to-nearest-even
//       (v_cvt_f16_f32; NOT the truncating packed conversion) or to bfloat16 (v_cvt_pk_bf16_f32, the definition's integer formula).
//       Element (c, y, x) of the file goes to dst + (dst_off + c*sc + y*sh + x*sw) elements.  Three store forms, chosen per launch from
//       the strides, so the branch is wave-uniform:
//         sw == 1 (planar rows)         per channel the four elements as ONE store of 4, 8 or 16 bytes when all four exist and the address
//                                       is a multiple of the store's size, single elements otherwise
//         sc == 1, sw == 3 (NHWC)       the twelve consecutive elements as whole 4-byte words (12-byte stores for 1- and 2-byte elements,
//                                       16-byte stores for F32) when all four pixels exist and the address is a multiple of 4, single
//                                       elements otherwise
//         any other strides             single elements
// Only the elements named are written: no padding, and never the other half of a word that holds a neighbouring 2-byte element.  No
// scratch.  resample_tensor_kernel<DT, C, true> is resample_kernel<3, true>'s counterpart: the two-pass form through static LDS for the files
// whose descriptor says so (the filters wider than the triangle), the same store stage behind it; <DT, C, false> has no LDS.
#include "jpezy_resample_core.h"

namespace jpezy_dev {
namespace resized {

enum { kFormPlanar = 0, kFormNhwc = 1, kFormGeneral = 2 };

template <int DT> struct ElemBytes { static constexpr int value = DT == kTensorU8 ? 1 : DT == kTensorF32 ? 4 : 2; };

// the element's bit pattern, in the low ElemBytes<DT> bytes
template <int DT>
__device__ __forceinline__ unsigned to_element(unsigned byte, float scale, float bias)
{
    if (DT == kTensorU8) return byte;
    const float v = __fadd_rn(__fmul_rn((float)byte, scale), bias);
    const unsigned u = __float_as_uint(v);
    if (DT == kTensorF32) return u;
    if (DT == kTensorF16) return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)v);
    // v_cvt_pk_bf16_f32: round to nearest even, for the finite v that the call admits the upper half of u + 0x7FFF + ((u >> 16) & 1)
    return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)v);
}

template <int EB>
__device__ __forceinline__ void store_one(uint8_t* at, unsigned bits)
{
    if (EB == 1) *at = (uint8_t)bits;
    else if (EB == 2) *reinterpret_cast<uint16_t*>(at) = (uint16_t)bits;
    else *reinterpret_cast<uint32_t*>(at) = bits;
}

// word w of consecutive elements e[] of EB bytes each
template <int EB>
__device__ __forceinline__ unsigned word_of(const unsigned* e, int w)
{
    if (EB == 1) return e[4 * w] | e[4 * w + 1] << 8 | e[4 * w + 2] << 16 | e[4 * w + 3] << 24;
    if (EB == 2) return e[2 * w] | e[2 * w + 1] << 16;
    return e[w];
}

typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef unsigned v3u __attribute__((ext_vector_type(3)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef v3u v3u_a4 __attribute__((aligned(4)));
typedef v4u v4u_a4 __attribute__((aligned(4)));

template <int DT, int C, bool TILE>
__global__ __launch_bounds__(kThreads) void resample_tensor_kernel(ResampleParams p, TensorOut t, int form)
{
    constexpr int EB = ElemBytes<DT>::value;
    const ResampleDesc d = workgroup_file(p);
    int ox0, oy, npx;
    uint32_t w[3];                                // byte j of w[c]: channel c of pixel j
    if constexpr (TILE) {                         // resample_kernel<3, true>'s choice per file (jpezy_kernels_resized.hip)
        __shared__ uint32_t tile[kTileWords];
        if (!(d.tiled ? resample_four_tiled<3>(p, d, tile, ox0, oy, npx, w[0], w[1], w[2]) : resample_four<3>(p, d, ox0, oy, npx, w[0], w[1], w[2]))) return;
    } else {
        if (!resample_four<3>(p, d, ox0, oy, npx, w[0], w[1], w[2])) return;
    }

    unsigned e[C][4];                             // the elements' bit patterns (those of pixels that do not exist are never stored)
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) e[c][j] = to_element<DT>((w[c] >> (8 * j)) & 0xFFu, t.scale[c], t.bias[c]);

    uint8_t* const base = p.dst + (d.dst_off + (size_t)oy * t.sh + (size_t)ox0 * t.sw) * EB;      // element (0, oy, ox0) of the file
    if (form == kFormPlanar) {                    // t.sw == 1
#pragma unroll
        for (int c = 0; c < C; ++c) {
            uint8_t* const at = base + (size_t)c * t.sc * EB;
            if (npx == 4 && ((uintptr_t)at & (uintptr_t)(4 * EB - 1)) == 0) {
                if (EB == 1) *reinterpret_cast<uint32_t*>(at) = word_of<1>(e[c], 0);
                else if (EB == 2) *reinterpret_cast<v2u*>(at) = v2u{ word_of<2>(e[c], 0), word_of<2>(e[c], 1) };
                else *reinterpret_cast<v4u*>(at) = v4u{ e[c][0], e[c][1], e[c][2], e[c][3] };
            } else {
                for (int j = 0; j < npx; ++j) store_one<EB>(at + j * EB, e[c][j]);
            }
        }
    } else if (C == 3 && form == kFormNhwc) {     // t.sc == 1, t.sw == 3: twelve consecutive elements
        if constexpr (C == 3) {
            if (npx == 4 && ((uintptr_t)base & 3u) == 0) {
                unsigned q[12];
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int c = 0; c < 3; ++c) q[j * 3 + c] = e[c][j];
                if constexpr (EB == 4) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) reinterpret_cast<v4u_a4*>(base)[k] = v4u{ q[4 * k], q[4 * k + 1], q[4 * k + 2], q[4 * k + 3] };
                } else {
#pragma unroll
                    for (int k = 0; k < EB; ++k)          // (12 bytes apart: a v3u is 16 bytes in an array)
                        *reinterpret_cast<v3u_a4*>(base + 12 * k) = v3u{ word_of<EB>(q, 3 * k), word_of<EB>(q, 3 * k + 1), word_of<EB>(q, 3 * k + 2) };
                }
            } else {
                for (int j = 0; j < npx; ++j)
#pragma unroll
                    for (int c = 0; c < 3; ++c) store_one<EB>(base + (j * 3 + c) * EB, e[c][j]);
            }
        }
    } else {
        for (int j = 0; j < npx; ++j)
#pragma unroll
            for (int c = 0; c < C; ++c) store_one<EB>(base + ((size_t)j * t.sw + (size_t)c * t.sc) * EB, e[c][j]);
    }
}

template <int DT>
static void launch_dt(const ResampleParams& q, const TensorOut& t, int form, unsigned n_wg, hipStream_t s, bool tile)
{
    if (t.channels == 3 && tile) hipLaunchKernelGGL((resample_tensor_kernel<DT, 3, true>), dim3(n_wg), dim3(kThreads), 0, s, q, t, form);
    else if (t.channels == 3) hipLaunchKernelGGL((resample_tensor_kernel<DT, 3, false>), dim3(n_wg), dim3(kThreads), 0, s, q, t, form);
    else if (tile) hipLaunchKernelGGL((resample_tensor_kernel<DT, 1, true>), dim3(n_wg), dim3(kThreads), 0, s, q, t, form);
    else hipLaunchKernelGGL((resample_tensor_kernel<DT, 1, false>), dim3(n_wg), dim3(kThreads), 0, s, q, t, form);
}

}  // namespace resized

// launch_resample's splitting rule; the store form is decided here, once per call
hipError_t launch_resample_tensor(const ResampleParams& p, const TensorOut& t, unsigned long long total_wg, hipStream_t s, bool tile)
{
    if (p.pix_bytes != 3 || p.n_desc < 1 || total_wg < 1 || total_wg > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (p.out_w < 1 || p.out_h < 1 || p.out_w > 65535 || p.out_h > 65535 || (p.src_stride & 3u)) return hipErrorInvalidValue;
    if ((t.channels != 1 && t.channels != 3) || t.dtype < kTensorU8 || t.dtype > kTensorBF16) return hipErrorInvalidValue;
    const int form = t.sw == 1 ? resized::kFormPlanar : (t.channels == 3 && t.sc == 1 && t.sw == 3) ? resized::kFormNhwc : resized::kFormGeneral;
    constexpr unsigned long long per = (1ull << 24) - 1;
    for (unsigned long long w0 = 0; w0 < total_wg; w0 += per) {
        ResampleParams q = p;
        q.wg_base = (unsigned)w0;
        const unsigned n_wg = (unsigned)(total_wg - w0 < per ? total_wg - w0 : per);
        switch (t.dtype) {
        case kTensorU8: resized::launch_dt<kTensorU8>(q, t, form, n_wg, s, tile); break;
        case kTensorF32: resized::launch_dt<kTensorF32>(q, t, form, n_wg, s, tile); break;
        case kTensorF16: resized::launch_dt<kTensorF16>(q, t, form, n_wg, s, tile); break;
        default: resized::launch_dt<kTensorBF16>(q, t, form, n_wg, s, tile); break;
        }
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace jpezy_dev
