// jpezy_kernels_f32_422.hip -- the f32 encode kernel for 4:2:2 chroma sampling (JPEZY_SAMPLING_422, include/jpezy_hip.h): 16 x 8 MCUs of
// four blocks Y-left, Y-right, Cb, Cr; chroma decimated horizontally only -- point-sampled (the pixel at 2 x') or, with
// JPEZY_DOWNSAMPLE_AVERAGE, the libjpeg h2v1 average of the pair.  The kernel body, the LDS geometry and the launcher are
// jpezy_f32_octet.h's; this file holds the description of the MCU (Unit422), the pick (or pair average) of the chroma samples and the
// __global__ wrapper.
//
// An octet is 128 x 8 pixels: 16 bytes of each plane per lane, 32 blocks and 4 KB of contiguous output per wave.  Four passes: Y-left,
// Y-right, Cb, Cr -- the third forms the samples of both chroma components, the fourth none.
//
// The averaged stage needs no cross-lane traffic (a pair lies inside the lane's row segment; h2v2 needs the neighbouring row's lane): it
// converts all 16 pixels of the row to exact truncated Cb / Cr -- chroma_px2's estimate and guard test, chroma_px_ref where it fires -- and
// forms floor((a + b + bias) / 2), bias 0 for even x', 1 for odd x' (an MCU starts at an even x', so the parity is the sample's index in
// the lane); small integers and a power-of-two scale: every step exact in FP32.
#include "jpezy_f32_octet.h"

namespace jpezy_dev {
namespace f32 {

// Both chroma components of a row in one go, a few pixels at a time: Cb and Cr share the byte conversions of a pixel, and formed a
// component at a time the compiler keeps all of a lane's conversions alive from the Cb pass to the Cr pass (hundreds of bytes of scratch
// per lane in the averaged instances); together they die with the pixels they belong to.  (jpezy_f32_quad.h, chroma_pairsums4: the
// same finding for the averaged 4:2:0 stage.)
constexpr float CB1 = -0.1687f, CB2 = -0.3313f, CB3 = 0.5f, CR1 = 0.5f, CR2 = -0.4187f, CR3 = -0.0813f;   // ref encoder/jpezy_encoder.hpp:249-256

// Point sampling: the 8 chroma samples of one 16-pixel row are pixels 0, 2, .., 14 -- bytes 0 and 2 of the four words;
// A[k] = (C[k], C[7-k]) as fdct8p takes them.  Word pair (0, 3) holds samples 0, 1 and 7, 6, word pair (1, 2) samples 2, 3 and 5, 4.
__device__ __forceinline__ void chroma8_even(const uint32_t* wr, const uint32_t* wg, const uint32_t* wb, f2* Ab, f2* Ar)
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int lo = h, hi = 3 - h;
        f2 e[4];
        chroma_px2<0, 2>(wr[lo], wg[lo], wb[lo], wr[hi], wg[hi], wb[hi], CB1, CB2, CB3, Ab[2 * h], e[0]);
        chroma_px2<2, 0>(wr[lo], wg[lo], wb[lo], wr[hi], wg[hi], wb[hi], CB1, CB2, CB3, Ab[2 * h + 1], e[1]);
        chroma_px2<0, 2>(wr[lo], wg[lo], wb[lo], wr[hi], wg[hi], wb[hi], CR1, CR2, CR3, Ar[2 * h], e[2]);
        chroma_px2<2, 0>(wr[lo], wg[lo], wb[lo], wr[hi], wg[hi], wb[hi], CR1, CR2, CR3, Ar[2 * h + 1], e[3]);
        if (JPEZY_LAB_COLOUR_VOTE(wave_any(min8(e) < CHROMA_TH))) {
            bool f;
            f = e[0].x < CHROMA_TH; if (f) Ab[2 * h].x = chroma_px_ref<0>(wr[lo], wg[lo], wb[lo], false);
            f = e[0].y < CHROMA_TH; if (f) Ab[2 * h].y = chroma_px_ref<2>(wr[hi], wg[hi], wb[hi], false);
            f = e[1].x < CHROMA_TH; if (f) Ab[2 * h + 1].x = chroma_px_ref<2>(wr[lo], wg[lo], wb[lo], false);
            f = e[1].y < CHROMA_TH; if (f) Ab[2 * h + 1].y = chroma_px_ref<0>(wr[hi], wg[hi], wb[hi], false);
            f = e[2].x < CHROMA_TH; if (f) Ar[2 * h].x = chroma_px_ref<0>(wr[lo], wg[lo], wb[lo], true);
            f = e[2].y < CHROMA_TH; if (f) Ar[2 * h].y = chroma_px_ref<2>(wr[hi], wg[hi], wb[hi], true);
            f = e[3].x < CHROMA_TH; if (f) Ar[2 * h + 1].x = chroma_px_ref<2>(wr[lo], wg[lo], wb[lo], true);
            f = e[3].y < CHROMA_TH; if (f) Ar[2 * h + 1].y = chroma_px_ref<0>(wr[hi], wg[hi], wb[hi], true);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// JPEZY_DOWNSAMPLE_AVERAGE: sample k of the row from pixels 2k, 2k + 1 (word k / 2, bytes 0, 1 or 2, 3) -- both exact truncated samples,
// then floor((a + b + (k & 1)) / 2): libjpeg's h2v1 rule on signed samples with an arithmetic shift.  One word (four pixels, two samples
// of each component) at a time.
__device__ __forceinline__ void chroma8_pairs(const uint32_t* wr, const uint32_t* wg, const uint32_t* wb, f2* Ab, f2* Ar)
{
    float Cb[8], Cr[8];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        f2 c[4], e[4];
        chroma_px2<0, 1>(wr[w], wg[w], wb[w], wr[w], wg[w], wb[w], CB1, CB2, CB3, c[0], e[0]);
        chroma_px2<2, 3>(wr[w], wg[w], wb[w], wr[w], wg[w], wb[w], CB1, CB2, CB3, c[1], e[1]);
        chroma_px2<0, 1>(wr[w], wg[w], wb[w], wr[w], wg[w], wb[w], CR1, CR2, CR3, c[2], e[2]);
        chroma_px2<2, 3>(wr[w], wg[w], wb[w], wr[w], wg[w], wb[w], CR1, CR2, CR3, c[3], e[3]);
        if (JPEZY_LAB_COLOUR_VOTE(wave_any(min8(e) < CHROMA_TH))) {
            bool f;
            f = e[0].x < CHROMA_TH; if (f) c[0].x = chroma_px_ref<0>(wr[w], wg[w], wb[w], false);
            f = e[0].y < CHROMA_TH; if (f) c[0].y = chroma_px_ref<1>(wr[w], wg[w], wb[w], false);
            f = e[1].x < CHROMA_TH; if (f) c[1].x = chroma_px_ref<2>(wr[w], wg[w], wb[w], false);
            f = e[1].y < CHROMA_TH; if (f) c[1].y = chroma_px_ref<3>(wr[w], wg[w], wb[w], false);
            f = e[2].x < CHROMA_TH; if (f) c[2].x = chroma_px_ref<0>(wr[w], wg[w], wb[w], true);
            f = e[2].y < CHROMA_TH; if (f) c[2].y = chroma_px_ref<1>(wr[w], wg[w], wb[w], true);
            f = e[3].x < CHROMA_TH; if (f) c[3].x = chroma_px_ref<2>(wr[w], wg[w], wb[w], true);
            f = e[3].y < CHROMA_TH; if (f) c[3].y = chroma_px_ref<3>(wr[w], wg[w], wb[w], true);
        }
        // small integers and a power-of-two scale: every step exact in FP32; floor is the arithmetic shift
        Cb[2 * w] = __builtin_floorf((c[0].x + c[0].y) * 0.5f);
        Cb[2 * w + 1] = __builtin_floorf(((c[1].x + c[1].y) + 1.f) * 0.5f);
        Cr[2 * w] = __builtin_floorf((c[2].x + c[2].y) * 0.5f);
        Cr[2 * w + 1] = __builtin_floorf(((c[3].x + c[3].y) + 1.f) * 0.5f);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        Ab[k] = f2{ Cb[k], Cb[7 - k] };
        Ar[k] = f2{ Cr[k], Cr[7 - k] };
    }
}

template <bool AVG>
struct Unit422 {
    static constexpr int BPM = 4, LUMA = 2, NW = 4;
    // Waves per SIMD the register allocation aims at: 3 (168 VGPRs), by measurement.  At the 4:4:4 kernel's 4 (128 VGPRs) the point-sampled
    // instances spill 20-120 bytes per lane and the averaged ones 120-180 (32 sample registers stay live for levels 2 and 3, and the averaged
    // stage converts 16 pixels of two components); a 4096 x 4096 frame then takes 38.0 us instead of 36.8 (random pixels), 34.2 instead of
    // 31.4 (smooth) and, averaged, 121 us instead of 59.5.  (Figures of the kernel before it shared jpezy_f32_octet.h; DESIGN.md 4.22 has
    // the present register counts.)
    static constexpr int WAVES = 3;

    // 16 packed pixels: 48 or 64 bytes, 16-byte aligned -- the quad's load
    template <int PIX>
    static __device__ __forceinline__ void load_packed(const uint8_t* src, bool swap_rb, uint32_t* R, uint32_t* G, uint32_t* B)
    {
        load_packed16<PIX>(src, swap_rb, R, G, B);
    }

    // (the chroma passes in front of the luma passes, where only the pixel words are live beside the conversions, need MORE registers)
    template <int COMP>
    static __device__ __forceinline__ void samples(const uint32_t* R, const uint32_t* G, const uint32_t* B, f2 (*S)[4])
    {
        if (COMP < 2) luma8(R + 2 * COMP, G + 2 * COMP, B + 2 * COMP, S[COMP]);
        else if (COMP == 2) {                                             // both chroma components; the pixel words die here
            if (AVG) chroma8_pairs(R, G, B, S[2], S[3]);
            else chroma8_even(R, G, B, S[2], S[3]);
        }
    }
};

// AVG: the averaged chroma stage
template <bool ALIGNED, int FORCE, bool DCG, int PIX, bool AVG>
__global__ __launch_bounds__(64 * OWPB, Unit422<AVG>::WAVES) void fdct_quant_f32_422_kernel(EncParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[OWPB][Octet<Unit422<AVG>>::WAVE_DWORDS];
    encode_octet<Unit422<AVG>, ALIGNED, FORCE, DCG, PIX>(p, &lds_all[0][0]);
}

template <bool AVG>
struct Kernels422 {
    typedef Unit422<AVG> Unit;
    template <bool ALIGNED, int FORCE, bool DCG, int PIX>
    static constexpr void (*kernel)(EncParams) = fdct_quant_f32_422_kernel<ALIGNED, FORCE, DCG, PIX, AVG>;
};

}  // namespace f32

// average: the JPEZY_DOWNSAMPLE_AVERAGE instances
hipError_t launch_fdct_quant_f32_422(const EncParams& p, int force, bool average, hipStream_t stream)
{
    return average ? launch_octets<f32::Kernels422<true>>(p, force, stream) : launch_octets<f32::Kernels422<false>>(p, force, stream);
}

}  // namespace jpezy_dev
