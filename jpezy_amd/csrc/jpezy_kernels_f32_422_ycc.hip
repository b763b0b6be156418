// jpezy_kernels_f32_422_ycc.hip -- the f32 encode kernel for 4:2:2 files from YCbCr 4:2:2 SAMPLES (include/jpezy_hip_ycc422.h): planar
// I422 / YV16 / NV16 / NV61, or packed macropixels YUY2 / UYVY / YVYU.  The caller's bytes are the file's samples, so the sample stage is
// ycc8 (jpezy_f32_quad.h: byte - 128, exact in FP32) -- no colour estimate, no guard test, no FP64 formula behind it.  The kernel body,
// the LDS geometry, the queue walk, the per-lane evaluator, the store and the launcher are jpezy_f32_octet.h's; this file holds the
// unit (Unit422Ycc), its load step -- the body's source hook -- and the __global__ wrapper.
//
// A lane (row r, MCU m of the octet) needs 16 Y bytes, 8 Cb and 8 Cr of its row.  It keeps them as R[0..3] = the Y words,
// G[0..1] = the Cb words, B[0..1] = the Cr words.  Three load forms:
//   aligned packed   32 contiguous bytes (8 macropixels) as two 16-byte loads -- the 8 lanes of a row cover 256 contiguous bytes --
//                    separated by v_perm_b32 into 4 Y + 2 Cb + 2 Cr words, the selectors chosen by format (wave-uniform)
//   aligned planar   one 16-byte Y load and two 8-byte chroma loads (c_step 1), or one 16-byte load of the interleaved CbCr segment
//                    whose even / odd bytes v_perm_b32 picks (c_step 2, Cb and Cr neighbours)
//   byte loop        the definition's clamps (W-1, CW-1; the row is clamped by the body), Y step and chroma step from the parameters:
//                    1 and 1 or 2 for planes, 2 and 4 for macropixels.  Every unaligned case and the test hooks' instances.
#include "jpezy_f32_octet.h"

namespace jpezy_dev {
namespace f32 {

struct Unit422Ycc {
    static constexpr int BPM = 4, LUMA = 2, NW = 4;
    static constexpr bool OWN_SOURCE = true;
    // Waves per SIMD the register allocation aims at.  The unit converts nothing, so it needs fewer registers than Unit422<false>: no
    // instance spills at 4 (128 VGPRs); DESIGN.md 4.24 has the compiler's table for 3 and 4.
    static constexpr int WAVES = 4;

    template <bool ALIGNED>
    static __device__ __forceinline__ void load(const EncParams& p, int frame, int mcu_x, int y, uint32_t* R, uint32_t* G, uint32_t* B)
    {
        // y_stride * H and c_stride * H < 2^32 (the entry points): the row offsets fit 32 bits
        const unsigned yoff = (unsigned)y * p.row_stride, coff = (unsigned)y * p.c_row_stride;
        const size_t fo = (size_t)frame * p.plane_stride, cfo = (size_t)frame * p.c_frame_stride;
        G[2] = G[3] = B[2] = B[3] = 0;                                    // not read
        if (ALIGNED && p.y_step == 2) {                                   // wave-uniform
            const uint4* s4 = reinterpret_cast<const uint4*>(p.pix + fo + (yoff + (unsigned)mcu_x * 32u));
            const uint4 v0 = s4[0], v1 = s4[1];
            const uint32_t w[8] = { v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w };      // one macropixel each
            const bool uyvy = p.yuv_format == 1;                          // JPEZY_YUV_UYVY: Cb Y0 Cr Y1
            const uint32_t ysel = uyvy ? 0x07050301u : 0x06040200u;
            // (Cb of the lower word, Cb of the upper, Cr of the lower, Cr of the upper); 2: JPEZY_YUV_YVYU (Y0 Cr Y1 Cb), else YUY2 (Y0 Cb Y1 Cr)
            const uint32_t csel = uyvy ? 0x06020400u : p.yuv_format == 2 ? 0x05010703u : 0x07030501u;
#pragma unroll
            for (int k = 0; k < 4; ++k) R[k] = __builtin_amdgcn_perm(w[2 * k + 1], w[2 * k], ysel);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const uint32_t c01 = __builtin_amdgcn_perm(w[4 * q + 1], w[4 * q], csel), c23 = __builtin_amdgcn_perm(w[4 * q + 3], w[4 * q + 2], csel);
                G[q] = __builtin_amdgcn_perm(c23, c01, 0x05040100u);
                B[q] = __builtin_amdgcn_perm(c23, c01, 0x07060302u);
            }
        } else if (ALIGNED) {
            const uint4 vy = *reinterpret_cast<const uint4*>(p.r + fo + (yoff + (unsigned)mcu_x * 16u));
            R[0] = vy.x; R[1] = vy.y; R[2] = vy.z; R[3] = vy.w;
            if (p.c_step == 1) {
                const uint2 vb = *reinterpret_cast<const uint2*>(p.g + cfo + (coff + (unsigned)mcu_x * 8u));
                const uint2 vr = *reinterpret_cast<const uint2*>(p.b + cfo + (coff + (unsigned)mcu_x * 8u));
                G[0] = vb.x; G[1] = vb.y; B[0] = vr.x; B[1] = vr.y;
            } else {
                const bool cb_first = p.g < p.b;
                const uint4 v = *reinterpret_cast<const uint4*>((cb_first ? p.g : p.b) + cfo + (coff + (unsigned)mcu_x * 16u));
                const uint32_t bsel = cb_first ? 0x06040200u : 0x07050301u, rsel = cb_first ? 0x07050301u : 0x06040200u;
                G[0] = __builtin_amdgcn_perm(v.y, v.x, bsel); G[1] = __builtin_amdgcn_perm(v.w, v.z, bsel);
                B[0] = __builtin_amdgcn_perm(v.y, v.x, rsel); B[1] = __builtin_amdgcn_perm(v.w, v.z, rsel);
            }
        } else {
            const uint8_t* py = p.r + fo + yoff;
            const uint8_t* pb = p.g + cfo + coff;
            const uint8_t* pr = p.b + cfo + coff;
            const unsigned ystep = (unsigned)p.y_step, cstep = (unsigned)p.c_step;
            const int CW = (p.W + 1) >> 1;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                uint32_t a = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) a |= (uint32_t)py[(unsigned)min(mcu_x * 16 + w * 4 + k, p.W - 1) * ystep] << (8 * k);
                R[w] = a;
            }
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                uint32_t ab = 0, ar = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned x = (unsigned)min(mcu_x * 8 + w * 4 + k, CW - 1) * cstep;
                    ab |= (uint32_t)pb[x] << (8 * k);
                    ar |= (uint32_t)pr[x] << (8 * k);
                }
                G[w] = ab; B[w] = ar;
            }
        }
    }

    // COMP 0 / 1: the Y words 0-1 / 2-3; COMP 2 / 3: the lane's two Cb / two Cr words
    template <int COMP>
    static __device__ __forceinline__ void samples(const uint32_t* R, const uint32_t* G, const uint32_t* B, f2 (*S)[4])
    {
        ycc8(COMP < 2 ? R + 2 * COMP : COMP == 2 ? G : B, S[COMP]);
    }
};

// PIX is the launcher's (always 0 here: the macropixel form is told by EncParams::y_step)
template <bool ALIGNED, int FORCE, bool DCG, int PIX>
__global__ __launch_bounds__(64 * OWPB, Unit422Ycc::WAVES) void fdct_quant_f32_422_ycc_kernel(EncParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[OWPB][Octet<Unit422Ycc>::WAVE_DWORDS];
    encode_octet<Unit422Ycc, ALIGNED, FORCE, DCG, 0>(p, &lds_all[0][0]);
}

struct Kernels422Ycc {
    typedef Unit422Ycc Unit;
    template <bool ALIGNED, int FORCE, bool DCG, int PIX>
    static constexpr void (*kernel)(EncParams) = fdct_quant_f32_422_ycc_kernel<ALIGNED, FORCE, DCG, 0>;
    // macropixels: the rules of the packed RGB launch; planes: those of launch_fdct_quant_f32_ycc (Y 16 bytes; chroma 8, or 16 for one
    // interleaved plane whose Cb and Cr are neighbours)
    static bool aligned(const EncParams& p)
    {
        if (p.W % 16) return false;
        if (p.y_step == 2) return p.row_stride % 16 == 0 && p.plane_stride % 16 == 0 && (uintptr_t)p.pix % 16 == 0;
        if (p.row_stride % 16 || p.plane_stride % 16 || (uintptr_t)p.r % 16) return false;
        const uintptr_t g = (uintptr_t)p.g, b = (uintptr_t)p.b;
        if (p.c_step == 1) return (g | b | p.c_row_stride | p.c_frame_stride) % 8 == 0;
        return (g > b ? g - b : b - g) == 1 && ((g < b ? g : b) | p.c_row_stride | p.c_frame_stride) % 16 == 0;
    }
};

}  // namespace f32

hipError_t launch_fdct_quant_f32_422_ycc(const EncParams& p, int force, hipStream_t stream)
{
    if (p.pix_bytes != 0 || (p.y_step == 1 ? p.c_step != 1 && p.c_step != 2 : p.y_step != 2 || p.c_step != 4)) return hipErrorInvalidValue;
    return launch_octets<f32::Kernels422Ycc>(p, force, stream);
}

}  // namespace jpezy_dev
