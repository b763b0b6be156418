// jpezy_kernels_f32_444.hip -- the f32 encode kernel for 4:4:4 chroma sampling (JPEZY_SAMPLING_444, include/jpezy_hip.h): 8 x 8 MCUs of
// three blocks Y, Cb, Cr, every pixel converted, nothing decimated.  The kernel body, the LDS geometry and the launcher are
// jpezy_f32_octet.h's; this file holds the description of the MCU (Unit444), the chroma sample stage and the __global__ wrapper.
//
// An octet is 64 x 8 pixels: 8 bytes of each plane per lane, 24 blocks and 3 KB of contiguous output per wave -- the block count and
// output footprint of a quad.  One component per pass (Y, then Cb, then Cr); the raw pixel words (6 registers) live until the Cr samples
// are formed.
#include "jpezy_f32_octet.h"

namespace jpezy_dev {
namespace f32 {

// The 8 chroma samples of one pixel row, A[k] = (C[k], C[7-k]) as fdct8p takes them; CR: Cr, else Cb.  chroma_px2's estimate and
// guard test on every pixel (the quad applies them to every second pixel of every second row), chroma_px_ref where the test fires.
template <bool CR>
__device__ __forceinline__ void chroma8(const uint32_t* wr, const uint32_t* wg, const uint32_t* wb, f2* A)
{
    // (Cb, Cr) = (-.1687 R - .3313 G + .5 B), (.5 R - .4187 G - .0813 B)   (ref encoder/jpezy_encoder.hpp:249-256)
    constexpr float k1 = CR ? 0.5f : -0.1687f, k2 = CR ? -0.4187f : -0.3313f, k3 = CR ? -0.0813f : 0.5f;
    f2 e[4];
    chroma_px2<0, 3>(wr[0], wg[0], wb[0], wr[1], wg[1], wb[1], k1, k2, k3, A[0], e[0]);
    chroma_px2<1, 2>(wr[0], wg[0], wb[0], wr[1], wg[1], wb[1], k1, k2, k3, A[1], e[1]);
    __builtin_amdgcn_sched_barrier(0);
    chroma_px2<2, 1>(wr[0], wg[0], wb[0], wr[1], wg[1], wb[1], k1, k2, k3, A[2], e[2]);
    chroma_px2<3, 0>(wr[0], wg[0], wb[0], wr[1], wg[1], wb[1], k1, k2, k3, A[3], e[3]);
    if (JPEZY_LAB_COLOUR_VOTE(wave_any(min8(e) < CHROMA_TH))) {
        bool f;
        f = e[0].x < CHROMA_TH; if (f) A[0].x = chroma_px_ref<0>(wr[0], wg[0], wb[0], CR);
        f = e[1].x < CHROMA_TH; if (f) A[1].x = chroma_px_ref<1>(wr[0], wg[0], wb[0], CR);
        f = e[2].x < CHROMA_TH; if (f) A[2].x = chroma_px_ref<2>(wr[0], wg[0], wb[0], CR);
        f = e[3].x < CHROMA_TH; if (f) A[3].x = chroma_px_ref<3>(wr[0], wg[0], wb[0], CR);
        f = e[3].y < CHROMA_TH; if (f) A[3].y = chroma_px_ref<0>(wr[1], wg[1], wb[1], CR);
        f = e[2].y < CHROMA_TH; if (f) A[2].y = chroma_px_ref<1>(wr[1], wg[1], wb[1], CR);
        f = e[1].y < CHROMA_TH; if (f) A[1].y = chroma_px_ref<2>(wr[1], wg[1], wb[1], CR);
        f = e[0].y < CHROMA_TH; if (f) A[0].y = chroma_px_ref<3>(wr[1], wg[1], wb[1], CR);
    }
}

struct Unit444 {
    static constexpr int BPM = 3, LUMA = 1, NW = 2;
    // Waves per SIMD the register allocation aims at: 4 (128 VGPRs).  At the quad kernel's 5 (96 VGPRs) this kernel spills ~250 bytes per
    // lane: three components' samples stay live for levels 2 and 3 where the quad holds two block rows and a half-filled chroma row.
    static constexpr int WAVES = 4;

    // 8 packed pixels: 24 bytes, 8-byte aligned, or 32 bytes, 16-byte aligned
    template <int PIX>
    static __device__ __forceinline__ void load_packed(const uint8_t* src, bool swap_rb, uint32_t* R, uint32_t* G, uint32_t* B)
    {
        load_packed8<PIX>(src, swap_rb, R, G, B);
    }

    template <int COMP>
    static __device__ __forceinline__ void samples(const uint32_t* R, const uint32_t* G, const uint32_t* B, f2 (*S)[4])
    {
        if (COMP == 0) luma8(R, G, B, S[0]);
        else chroma8<COMP == 2>(R, G, B, S[COMP]);
    }
};

template <bool ALIGNED, int FORCE, bool DCG, int PIX>
__global__ __launch_bounds__(64 * OWPB, Unit444::WAVES) void fdct_quant_f32_444_kernel(EncParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[OWPB][Octet<Unit444>::WAVE_DWORDS];
    encode_octet<Unit444, ALIGNED, FORCE, DCG, PIX>(p, &lds_all[0][0]);
}

struct Kernels444 {
    typedef Unit444 Unit;
    template <bool ALIGNED, int FORCE, bool DCG, int PIX>
    static constexpr void (*kernel)(EncParams) = fdct_quant_f32_444_kernel<ALIGNED, FORCE, DCG, PIX>;
};

}  // namespace f32

hipError_t launch_fdct_quant_f32_444(const EncParams& p, int force, hipStream_t stream)
{
    return launch_octets<f32::Kernels444>(p, force, stream);
}

}  // namespace jpezy_dev
