// jpezy_kernels_f32.hip -- encode kernel, variant 1 (the default): one quad per wave, one launch of exactly as many waves as quads.
// Three precision levels, same bits as the reference: the arithmetic of a quad is jpezy_f32_quad.h.
#include "jpezy_f32_onequad.h"

namespace jpezy_dev {
namespace f32 {

// ---- planar YCbCr 4:2:0 samples (I420 / NV12 and their mirror images): jpezy_fdct_quant_ycc_dev -------------------------------------
// The caller's planes are the file's own sample domain, so step 1 fetches samples instead of pixels -- the lane's 16 Y bytes of its
// row and the 8 bytes of chroma row mcu_y * 8 + (row >> 1), Cb on even-row lanes and Cr on odd-row lanes -- and the sample stage of
// the quad is byte - 128 (jpezy_f32_quad.h, YCC): no colour estimates, no guard test, 1.5 bytes per pixel instead of 3.
// ALIGNED (the launcher: W % 16 == 0, every base and stride a multiple of the access): one 16-byte load of Y and one 8-byte load of a
// chroma plane, or -- c_step == 2, one interleaved plane -- one 16-byte load of the CbCr row segment whose even or odd bytes
// v_perm_b32 picks.  Anything else: the byte loop with the edge replication of the definition (include/jpezy_hip.h).
template <bool GRAY, bool ALIGNED, int FORCE, int EWPB, bool DCG>
__global__ __launch_bounds__(64 * EWPB, JPEZY_F32_WAVES) void fdct_quant_f32_ycc_kernel(EncParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[EWPB][WAVE_LDS_DWORDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int mcu_y = (int)fast_div(blockIdx.x, p.gpr_magic, p.gpr_shift);
    const int gx = (int)blockIdx.x - mcu_y * p.groups_per_row;
    const int quad_x = gx * EWPB + wave;
    if (quad_x >= p.quads_per_row) return;                                // wave-uniform; the waves never meet at a barrier
    const unsigned qidx = (unsigned)(mcu_y * p.quads_per_row + quad_x);
    const int frame = (int)blockIdx.y;
    uint32_t* lds = lds_all[wave];
    const int row = lane >> 2, m = lane & 3;
    const int mcu_x = min(quad_x * 4 + m, p.mcu_cols - 1);
    const int W = p.W, H = p.H, CW = (W + 1) >> 1, CH = (H + 1) >> 1;
    const int y = min(mcu_y * 16 + row, H - 1);                           // the definition's min(.., H - 1) / min(.., CH - 1)
    const int cy = min(mcu_y * 8 + (row >> 1), CH - 1);
    // row_stride * H and c_row_stride * CH < 2^32 (the entry point refuses more)
    const uint8_t* py = p.r + (size_t)frame * p.plane_stride + (unsigned)y * p.row_stride;
    const uint8_t* mine = (row & 1) ? p.b : p.g;                          // Cb for even pixel rows, Cr for odd ones
    const uint8_t* pc = mine + (size_t)frame * p.c_frame_stride + (unsigned)cy * p.c_row_stride;
    uint32_t Yw[4], Cw[4] = { 0, 0, 0, 0 };
    if (ALIGNED) {
        const uint4 v = *reinterpret_cast<const uint4*>(py + (unsigned)mcu_x * 16u);
        Yw[0] = v.x; Yw[1] = v.y; Yw[2] = v.z; Yw[3] = v.w;
        if (!GRAY) {
            if (p.c_step == 1) {                                          // wave-uniform
                const uint2 c = *reinterpret_cast<const uint2*>(pc + (unsigned)mcu_x * 8u);
                Cw[0] = c.x; Cw[1] = c.y;
            } else {
                // Cb and Cr are neighbours (the launcher): the lane's sample bytes are the even or the odd bytes of 16
                const bool second = ((uintptr_t)mine & 1u) != 0;
                const uint4 c = *reinterpret_cast<const uint4*>(pc - (second ? 1 : 0) + (unsigned)mcu_x * 16u);
                const uint32_t sel = second ? 0x07050301u : 0x06040200u;
                Cw[0] = __builtin_amdgcn_perm(c.y, c.x, sel);
                Cw[1] = __builtin_amdgcn_perm(c.w, c.z, sel);
            }
        }
    } else {
#pragma unroll
        for (int w4 = 0; w4 < 4; ++w4) {
            uint32_t a = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) a |= (uint32_t)py[min(mcu_x * 16 + w4 * 4 + k, W - 1)] << (8 * k);
            Yw[w4] = a;
        }
        if (!GRAY) {
            const unsigned step = (unsigned)p.c_step;
#pragma unroll
            for (int w4 = 0; w4 < 2; ++w4) {
                uint32_t a = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) a |= (uint32_t)pc[(unsigned)min(mcu_x * 8 + w4 * 4 + k, CW - 1) * step] << (8 * k);
                Cw[w4] = a;
            }
        }
    }
#ifdef JPEZY_TRACE
    QuadTrace tr;                                                         // (the wave trace follows the planar RGB kernel only)
#if JPEZY_TRACE >= 3
    unsigned long long* ph = tr.ph;
#endif
#endif
    encode_quad<GRAY, FORCE, false, DCG, true>(p, Yw, Cw, Cw, lds, lane, mcu_y, quad_x, frame, qidx, nullptr, nullptr, nullptr QUAD_TRACE_ARG);
}

}  // namespace f32

template <bool GRAY, bool ALIGNED, int EW>
static void enc_f32_ycc_launch(const EncParams& p, int force, dim3 grid, hipStream_t s)
{
    const bool dcg = p.dc_rq[0] != 0.f && p.dc_rq[1] != 0.f;            // as enc_f32_launch2
#define JPEZY_YCC_LAUNCH(F)                                                                                                  \
    do {                                                                                                                     \
        if (dcg) hipLaunchKernelGGL((f32::fdct_quant_f32_ycc_kernel<GRAY, ALIGNED, F, EW, true>), grid, dim3(64 * EW), 0, s, p); \
        else hipLaunchKernelGGL((f32::fdct_quant_f32_ycc_kernel<GRAY, ALIGNED, F, EW, false>), grid, dim3(64 * EW), 0, s, p);    \
    } while (0)
    if constexpr (EW == 2) {
        if (force == 1) { JPEZY_YCC_LAUNCH(1); return; }
        if (force == 2) { JPEZY_YCC_LAUNCH(2); return; }
        if (force == 3) { JPEZY_YCC_LAUNCH(3); return; }
    }
    JPEZY_YCC_LAUNCH(0);
#undef JPEZY_YCC_LAUNCH
}

hipError_t launch_fdct_quant_f32_ycc(const EncParams& p0, bool gray, int force, hipStream_t stream)
{
    EncParams p = p0;
    if (p.n_frames > 65535 || (!gray && p.c_step != 1 && p.c_step != 2)) return hipErrorInvalidValue;
    bool al = p.W % 16 == 0 && p.row_stride % 16 == 0 && p.plane_stride % 16 == 0 && (uintptr_t)p.r % 16 == 0;
    if (al && !gray) {
        const uintptr_t g = (uintptr_t)p.g, b = (uintptr_t)p.b;
        if (p.c_step == 1) al = (g | b | p.c_row_stride | p.c_frame_stride) % 8 == 0;
        else al = (g > b ? g - b : b - g) == 1 && ((g < b ? g : b) | p.c_row_stride | p.c_frame_stride) % 16 == 0;
    }
    // the workgroup shapes of the packed launch (direct loads in both); the test hooks' instances exist for two waves only
    const int ew = (al && p.quads_per_row % 4 == 0 && force == 0) ? 4 : 2;
    p.groups_per_row = (p.quads_per_row + ew - 1) / ew;
    const long groups = (long)p.mcu_rows * p.groups_per_row;
    if (groups <= 0 || p.n_frames <= 0) return hipSuccess;
    fast_div_setup((unsigned)p.groups_per_row, &p.gpr_magic, &p.gpr_shift);
    const dim3 grid((unsigned)groups, (unsigned)p.n_frames);
    if (ew == 4) {
        if (gray) enc_f32_ycc_launch<true, true, 4>(p, force, grid, stream); else enc_f32_ycc_launch<false, true, 4>(p, force, grid, stream);
    } else if (gray) {
        if (al) enc_f32_ycc_launch<true, true, 2>(p, force, grid, stream); else enc_f32_ycc_launch<true, false, 2>(p, force, grid, stream);
    } else {
        if (al) enc_f32_ycc_launch<false, true, 2>(p, force, grid, stream); else enc_f32_ycc_launch<false, false, 2>(p, force, grid, stream);
    }
    return hipGetLastError();
}

template <bool GRAY, bool ALIGNED, int EW, bool DCG, bool COOP>
static void enc_f32_launch3(const EncParams& p, int force, dim3 grid, hipStream_t s)
{
    if (force == 1)
        hipLaunchKernelGGL((f32::fdct_quant_f32_kernel<GRAY, ALIGNED, 1, EW, DCG, false, COOP>), grid, dim3(64 * EW), 0, s, p);
    else if (force == 2)
        hipLaunchKernelGGL((f32::fdct_quant_f32_kernel<GRAY, ALIGNED, 2, EW, DCG, false, COOP>), grid, dim3(64 * EW), 0, s, p);
    else if (force == 3)
        hipLaunchKernelGGL((f32::fdct_quant_f32_kernel<GRAY, ALIGNED, 3, EW, DCG, false, COOP>), grid, dim3(64 * EW), 0, s, p);
    else
        hipLaunchKernelGGL((f32::fdct_quant_f32_kernel<GRAY, ALIGNED, 0, EW, DCG, false, COOP>), grid, dim3(64 * EW), 0, s, p);
}

template <bool GRAY, bool ALIGNED, int EW, bool COOP>
static void enc_f32_launch2(const EncParams& p, int force, dim3 grid, hipStream_t s)
{
    // the DC through the generic quantiser where jpezy_ctx_create verified it for this build's constants (both tables), else on its
    // own path from the exact table -- a second instance of the kernel, so that the common one carries no trace of the DC path
    if (p.dc_rq[0] != 0.f && p.dc_rq[1] != 0.f) enc_f32_launch3<GRAY, ALIGNED, EW, true, COOP>(p, force, grid, s);
    else enc_f32_launch3<GRAY, ALIGNED, EW, false, COOP>(p, force, grid, s);
}

static bool enc_f32_aligned16(const EncParams& p)
{
    return (p.W % 16 == 0) && (p.plane_stride % 16 == 0) && (((uintptr_t)p.r | (uintptr_t)p.g | (uintptr_t)p.b) % 16 == 0);
}

// The workgroup form of a launch (enum jpezy_encode_groups in include/jpezy_hip.h): both cooperative forms need 16-byte pieces (al),
// the four-wave one also rows of quads that divide by four (its waves all compute); the direct form serves everything.
bool fdct_quant_f32_groups_legal(const EncParams& p, int groups)
{
    const bool al = enc_f32_aligned16(p);
    switch (groups) {
    case ENC_GROUPS_AUTO: case ENC_GROUPS_2_DIRECT: return true;
    case ENC_GROUPS_4_COOP: return al && p.quads_per_row % 4 == 0;
    case ENC_GROUPS_2_COOP: return al;
    default: return false;
    }
}

#ifndef JPEZY_ENC_GROUPS_DEFAULT
#define JPEZY_ENC_GROUPS_DEFAULT ENC_GROUPS_AUTO     // A/B builds (tools/ab/ab_build.py) pin a form here
#endif

static int enc_f32_pick_groups(const EncParams& p, bool al)
{
    // the record behind every line is profiles/r26_two_wave_coop.txt (interleaved A/B against the form of the line before it)
    if (!al) return ENC_GROUPS_2_DIRECT;                              // no 16-byte pieces: the only legal form
    // rows that divide into groups of four quads (4096 and 7680 wide) took four cooperative waves; two cooperative waves release
    // their LDS sooner and won every round on encode4096 (-0.5 / -0.6 us of 26.3 / 26.75) and gray8k (-0.8 us of 38.1)
    if (p.quads_per_row % 4 == 0) return ENC_GROUPS_2_COOP;
    // every other row (1920 wide: 30 quads) keeps direct loads: batch1080p was 1.4 us of 87 SLOWER in every round with cooperative ones
    return ENC_GROUPS_2_DIRECT;
}

hipError_t launch_fdct_quant_f32(const EncParams& p0, bool gray, int force, hipStream_t stream, int groups)
{
    EncParams p = p0;
    const bool al = enc_f32_aligned16(p);
    if (groups == ENC_GROUPS_AUTO && fdct_quant_f32_groups_legal(p, JPEZY_ENC_GROUPS_DEFAULT)) groups = JPEZY_ENC_GROUPS_DEFAULT;
    if (!fdct_quant_f32_groups_legal(p, groups)) return hipErrorInvalidValue;      // (jpezy_internal_fdct_quant_core refuses it first)
    if (groups == ENC_GROUPS_AUTO) groups = enc_f32_pick_groups(p, al);
    const int ew = groups == ENC_GROUPS_4_COOP ? 4 : 2;
    p.groups_per_row = (p.quads_per_row + ew - 1) / ew;
    const long ngroups = (long)p.mcu_rows * p.groups_per_row;
    if (ngroups <= 0 || p.n_frames <= 0) return hipSuccess;
    if (p.n_frames > 65535) return hipErrorInvalidValue;               // grid.y limit; callers chunk larger batches
    fast_div_setup((unsigned)p.groups_per_row, &p.gpr_magic, &p.gpr_shift);
    const dim3 grid((unsigned)ngroups, (unsigned)p.n_frames);
    if (groups == ENC_GROUPS_4_COOP) {
        if (gray) enc_f32_launch2<true, true, 4, true>(p, force, grid, stream); else enc_f32_launch2<false, true, 4, true>(p, force, grid, stream);
    } else if (groups == ENC_GROUPS_2_COOP) {
        if (gray) enc_f32_launch2<true, true, 2, true>(p, force, grid, stream); else enc_f32_launch2<false, true, 2, true>(p, force, grid, stream);
    } else if (gray) {
        if (al) enc_f32_launch2<true, true, 2, false>(p, force, grid, stream); else enc_f32_launch2<true, false, 2, false>(p, force, grid, stream);
    } else {
        if (al) enc_f32_launch2<false, true, 2, false>(p, force, grid, stream); else enc_f32_launch2<false, false, 2, false>(p, force, grid, stream);
    }
    return hipGetLastError();
}


template <bool GRAY, bool ALIGNED, int EW, int PIX>
static void enc_f32_packed_launch(const EncParams& p, int force, dim3 grid, hipStream_t s)
{
    const bool dcg = p.dc_rq[0] != 0.f && p.dc_rq[1] != 0.f;            // as enc_f32_launch2
#define JPEZY_PACKED_LAUNCH(F)                                                                                                   \
    do {                                                                                                                         \
        if (dcg) hipLaunchKernelGGL((f32::fdct_quant_f32_packed_kernel<GRAY, ALIGNED, F, EW, true, PIX>), grid, dim3(64 * EW), 0, s, p); \
        else hipLaunchKernelGGL((f32::fdct_quant_f32_packed_kernel<GRAY, ALIGNED, F, EW, false, PIX>), grid, dim3(64 * EW), 0, s, p);    \
    } while (0)
    if constexpr (EW == 2) {
        if (force == 1) { JPEZY_PACKED_LAUNCH(1); return; }
        if (force == 2) { JPEZY_PACKED_LAUNCH(2); return; }
        if (force == 3) { JPEZY_PACKED_LAUNCH(3); return; }
    }
    JPEZY_PACKED_LAUNCH(0);
#undef JPEZY_PACKED_LAUNCH
}

template <int PIX>
static void enc_f32_packed_launch_pix(const EncParams& p, bool gray, bool al, int ew, int force, dim3 grid, hipStream_t s)
{
    if (ew == 4) {
        if (gray) enc_f32_packed_launch<true, true, 4, PIX>(p, force, grid, s); else enc_f32_packed_launch<false, true, 4, PIX>(p, force, grid, s);
    } else if (gray) {
        if (al) enc_f32_packed_launch<true, true, 2, PIX>(p, force, grid, s); else enc_f32_packed_launch<true, false, 2, PIX>(p, force, grid, s);
    } else {
        if (al) enc_f32_packed_launch<false, true, 2, PIX>(p, force, grid, s); else enc_f32_packed_launch<false, false, 2, PIX>(p, force, grid, s);
    }
}

bool packed_is_aligned16(const void* pix, int W, size_t row_stride, size_t frame_stride)
{
    return W % 16 == 0 && row_stride % 16 == 0 && frame_stride % 16 == 0 && (uintptr_t)pix % 16 == 0;
}

hipError_t launch_fdct_quant_f32_packed(const EncParams& p0, bool gray, int force, hipStream_t stream)
{
    EncParams p = p0;
    const bool al = packed_is_aligned16(p.pix, p.W, p.row_stride, p.plane_stride);
    // the workgroup shapes of the planar launch (both with direct loads here); the test hooks' instances exist for two waves only
    const int ew = (al && p.quads_per_row % 4 == 0 && force == 0) ? 4 : 2;
    p.groups_per_row = (p.quads_per_row + ew - 1) / ew;
    const long groups = (long)p.mcu_rows * p.groups_per_row;
    if (groups <= 0 || p.n_frames <= 0) return hipSuccess;
    if (p.n_frames > 65535 || (p.pix_bytes != 3 && p.pix_bytes != 4)) return hipErrorInvalidValue;
    fast_div_setup((unsigned)p.groups_per_row, &p.gpr_magic, &p.gpr_shift);
    const dim3 grid((unsigned)groups, (unsigned)p.n_frames);
    if (p.pix_bytes == 3) enc_f32_packed_launch_pix<3>(p, gray, al, ew, force, grid, stream);
    else enc_f32_packed_launch_pix<4>(p, gray, al, ew, force, grid, stream);
    return hipGetLastError();
}

}  // namespace jpezy_dev
