// jpezy_kernels_f32.hip -- encode kernel, variant 1 (the default): one quad per wave, one launch of exactly as many waves as quads.
// Three precision levels, same bits as the reference: the arithmetic of a quad is jpezy_f32_quad.h.
#include "jpezy_f32_quad.h"

namespace jpezy_dev {
namespace f32 {

template <bool GRAY, bool ALIGNED, int FORCE, int EWPB, bool DCG>
__global__ __launch_bounds__(64 * EWPB, JPEZY_F32_WAVES) void fdct_quant_f32_kernel(EncParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[EWPB][WAVE_LDS_DWORDS];
    constexpr bool COOP = ALIGNED && EWPB == 4;     // (the cooperative load is written for 4 waves: 4 x 4 rows of 256 bytes)
    static_assert(!COOP || 3 * 4096 <= EWPB * WAVE_LDS_DWORDS * 4, "the pixel staging area lies over the waves' slices");

    // WPB waves per workgroup; the wave index is made an SGPR so that everything derived from it (quad position, plane
    // and coefficient base addresses, the LDS slice) is computed once on the scalar unit
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // One quad per wave, one launch of exactly as many waves as quads.  Measured alternatives: a grid-stride loop over a
    // grid sized to the resident workgroups -- same 4096^2 time (the kernel's tail comes from XCD-to-XCD variation, which
    // a static partition cannot balance either) and 8 more VGPRs; resident waves drawing quads from one device-scope
    // atomic counter -- 240 us instead of 30: 21 k draws on one address serialise at ~10 ns each; 4 resident waves per
    // SIMD, 4 quads each, the next quad's pixels prefetched during the current one (109 VGPRs) -- 34.7 us: waves started
    // together stay in the same phase of the quad (all in the LDS transposes, then all in the butterflies), whereas waves
    // of one-quad launches arrive staggered and overlap each other's latency-bound phases.
    // grid x = groups of EWPB quads: groups_per_row = ceil(quads_per_row / EWPB) per MCU row (a group never straddles rows)
    const int mcu_y = (int)fast_div(blockIdx.x, p.gpr_magic, p.gpr_shift);
    const int gx = (int)blockIdx.x - mcu_y * p.groups_per_row;
    const int quad_x = gx * EWPB + wave;
    const bool has_quad = quad_x < p.quads_per_row;                    // wave-uniform
    if (!COOP && !has_quad) return;
    const unsigned qidx = (unsigned)(mcu_y * p.quads_per_row + quad_x);   // quad index inside the frame
    const int frame = (int)blockIdx.y;
#ifdef JPEZY_TRACE
    const unsigned long long tr_t0 = __builtin_amdgcn_s_memrealtime();
    QuadTrace tr;
#if JPEZY_TRACE >= 3
    unsigned long long* ph = tr.ph;
    for (int k = 0; k < 8; ++k) ph[k] = 0;
    PHASE_STAMP(0);
#endif
#endif
    uint32_t* lds = lds_all[wave];
    const int row = lane >> 2, m = lane & 3;
    const int mcu_x = min(quad_x * 4 + m, p.mcu_cols - 1);
    const int W = p.W, H = p.H;
    const uint8_t* pr = p.r + (size_t)frame * p.plane_stride;
    const uint8_t* pg = p.g + (size_t)frame * p.plane_stride;
    const uint8_t* pb = p.b + (size_t)frame * p.plane_stride;

    // ---- 1. this lane's 16-pixel row segment of the three planes ----
    uint32_t R[4], G[4], B[4];
    if (COOP) {
        // The workgroup's 256 x 16 pixels of each plane go to LDS as [plane][row][16 pieces of 16 bytes]: wave w fetches rows
        // 4w .. 4w+3, 16 lanes per row, with ONE LDS-DMA instruction per plane (the destination of an LDS-DMA is the wave's
        // base + 16 x lane, so the image is lane-linear: 4 rows of 256 bytes).  Piece c of row r lies at position
        // c ^ 4(r & 3) -- the swizzle is applied to the SOURCE address -- so that the 16-byte reads below, whose 16-lane
        // groups span the rows {0,3,5,6} / {1,2,4,7} of one quad, hit 16 different bank groups.  The area lies over the
        // waves' slices: a second barrier before anybody writes a slice.
        char* stg = reinterpret_cast<char*>(&lds_all[0][0]);
        {
            const int lr = lane >> 4, cp = lane & 15;
            const int y = min(mcu_y * 16 + wave * 4 + lr, H - 1);                     // edge replication, ref :101
            const int piece = min(gx * 16 + (cp ^ (4 * lr)), p.mcu_cols - 1);         // W % 16 == 0 here: a piece is an MCU column
            const unsigned off = (unsigned)y * (unsigned)W + (unsigned)piece * 16u;   // W, H <= 65535 (launcher): fits 32 bits
            typedef __attribute__((address_space(1))) const void* gptr;
            typedef __attribute__((address_space(3))) void* lptr;
            __builtin_amdgcn_global_load_lds((gptr)(pr + off), (lptr)(stg + wave * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr)(pg + off), (lptr)(stg + 4096 + wave * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr)(pb + off), (lptr)(stg + 8192 + wave * 1024), 16, 0, 0);
        }
        __syncthreads();                                   // waits for this wave's DMA (vmcnt) and for the other three
        {
            const char* src = stg + row * 256 + (((wave * 4 + m) ^ (4 * (row & 3))) * 16);
            const uint4 vr = *reinterpret_cast<const uint4*>(src);
            const uint4 vg = *reinterpret_cast<const uint4*>(src + 4096);
            const uint4 vb = *reinterpret_cast<const uint4*>(src + 8192);
            R[0] = vr.x; R[1] = vr.y; R[2] = vr.z; R[3] = vr.w;
            G[0] = vg.x; G[1] = vg.y; G[2] = vg.z; G[3] = vg.w;
            B[0] = vb.x; B[1] = vb.y; B[2] = vb.z; B[3] = vb.w;
        }
        __syncthreads();                                   // staging area consumed: the slices are private from here on
        if (!has_quad) return;
    } else {
        const int y = min(mcu_y * 16 + row, H - 1);                   // edge replication, ref :101
        const unsigned rowoff = (unsigned)y * (unsigned)W;            // W, H <= 65535 (launcher): fits 32 bits
        if (ALIGNED) {
            const unsigned off = rowoff + (unsigned)mcu_x * 16u;
            const uint4 vr = *reinterpret_cast<const uint4*>(pr + off);
            const uint4 vg = *reinterpret_cast<const uint4*>(pg + off);
            const uint4 vb = *reinterpret_cast<const uint4*>(pb + off);
            R[0] = vr.x; R[1] = vr.y; R[2] = vr.z; R[3] = vr.w;
            G[0] = vg.x; G[1] = vg.y; G[2] = vg.z; G[3] = vg.w;
            B[0] = vb.x; B[1] = vb.y; B[2] = vb.z; B[3] = vb.w;
        } else {
#pragma unroll
            for (int w4 = 0; w4 < 4; ++w4) {
                uint32_t ar = 0, ag = 0, ab = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int x = min(mcu_x * 16 + w4 * 4 + k, W - 1);   // ref :104
                    ar |= (uint32_t)pr[rowoff + x] << (8 * k);
                    ag |= (uint32_t)pg[rowoff + x] << (8 * k);
                    ab |= (uint32_t)pb[rowoff + x] << (8 * k);
                }
                R[w4] = ar; G[w4] = ag; B[w4] = ab;
            }
        }
    }
#ifdef JPEZY_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long tr_t1 = __builtin_amdgcn_s_memrealtime();
#endif
    PHASE_STAMP(1);
    encode_quad<GRAY, FORCE, false, DCG>(p, R, G, B, lds, lane, mcu_y, quad_x, frame, qidx, nullptr, nullptr, nullptr QUAD_TRACE_ARG);
#ifdef JPEZY_TRACE
    if (frame == 0 && qidx < 65536u) {
#if JPEZY_TRACE > 1
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        const unsigned long long tr_t3 = __builtin_amdgcn_s_memrealtime();
        const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
        if (lane == 0) {
            p.trace[qidx * 4 + 0] = tr_t0;
            p.trace[qidx * 4 + 1] = ((tr_t1 - tr_t0) << 32) | (tr.t2 - tr_t0);
            p.trace[qidx * 4 + 2] = tr_t3 - tr_t0;
            p.trace[qidx * 4 + 3] = ((unsigned long long)xcc << 32) | hw;
#if JPEZY_TRACE >= 3
            unsigned long long t_end;
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_end) : : "memory");
#pragma unroll
            for (int k = 0; k < 8; ++k) p.trace[4 * 65536 + qidx * 9 + k] = ph[k];
            p.trace[4 * 65536 + qidx * 9 + 8] = t_end;
#endif
        }
    }
#endif
}

// ---- packed (interleaved) pixels: jpezy_fdct_quant_packed_dev ------------------------------------------------------------------
// The same quad, the same arithmetic (encode_quad takes R[4], G[4], B[4] as before); only step 1 differs.  PIX = bytes per pixel.
// ALIGNED (W % 16 == 0; base, row stride and frame stride multiples of 16): a lane's 16-pixel row segment is 48 or 64 contiguous
// bytes -- three or four 16-byte loads, the four lanes of a pixel row read 192 or 256 contiguous bytes, so there is no
// 64-bytes-of-16-rows pattern to cure and no cooperative load for either workgroup shape -- and the channels are separated in
// registers with v_perm_b32: 24 bits per pixel need 2 per output word (24 per lane), 32 bits per pixel 7 per four pixels (28 per
// lane, two levels: the (c0, c2) pairs and the c1 pairs of two pixels, then one per output word).  Blue first (BGR, BGRA) only
// exchanges the selectors of the first and the third channel, chosen on the scalar unit: it costs no vector instruction.
// Anything else: the byte loop over the three channel pointers with the planar kernel's edge replication.
template <int PIX>
__device__ __forceinline__ void load_packed16(const uint8_t* src, bool swap_rb, uint32_t* R, uint32_t* G, uint32_t* B)
{
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    if (PIX == 3) {
        // bytes of three words = four pixels: c0 at 0, 3, 6, 9; c1 at 1, 4, 7, 10; c2 at 2, 5, 8, 11
        const uint32_t a1 = swap_rb ? 0x00000502u : 0x00060300u, a2 = swap_rb ? 0x07040100u : 0x05020100u;   // red
        const uint32_t c1 = swap_rb ? 0x00060300u : 0x00000502u, c2 = swap_rb ? 0x05020100u : 0x07040100u;   // blue
        const uint4 v0 = s4[0], v1 = s4[1], v2 = s4[2];
        const uint32_t w[12] = { v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w };
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t w0 = w[3 * q], w1 = w[3 * q + 1], w2 = w[3 * q + 2];
            R[q] = __builtin_amdgcn_perm(w2, __builtin_amdgcn_perm(w1, w0, a1), a2);
            G[q] = __builtin_amdgcn_perm(w2, __builtin_amdgcn_perm(w1, w0, 0x00070401u), 0x06020100u);
            B[q] = __builtin_amdgcn_perm(w2, __builtin_amdgcn_perm(w1, w0, c1), c2);
        }
    } else {
        // one word per pixel (c0, c1, c2, unused): u = (c0, c0', c2, c2') and v = (c1, c1', ., .) of a pixel pair, then the words
        const uint32_t a = swap_rb ? 0x07060302u : 0x05040100u, c = swap_rb ? 0x05040100u : 0x07060302u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {                          // one 16-byte piece at a time: its four words die here
            const uint4 v = s4[q];
            const uint32_t u01 = __builtin_amdgcn_perm(v.y, v.x, 0x06020400u), u23 = __builtin_amdgcn_perm(v.w, v.z, 0x06020400u);
            const uint32_t v01 = __builtin_amdgcn_perm(v.y, v.x, 0x00000501u), v23 = __builtin_amdgcn_perm(v.w, v.z, 0x00000501u);
            R[q] = __builtin_amdgcn_perm(u23, u01, a);
            G[q] = __builtin_amdgcn_perm(v23, v01, 0x05040100u);
            B[q] = __builtin_amdgcn_perm(u23, u01, c);
        }
    }
}

template <bool GRAY, bool ALIGNED, int FORCE, int EWPB, bool DCG, int PIX>
__global__ __launch_bounds__(64 * EWPB, JPEZY_F32_WAVES) void fdct_quant_f32_packed_kernel(EncParams p)
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
    const int W = p.W, H = p.H;
    const int y = min(mcu_y * 16 + row, H - 1);                           // edge replication, ref :101
    const unsigned rowoff = (unsigned)y * p.row_stride;                   // row_stride * H < 2^32 (the entry point refuses more)
    uint32_t R[4], G[4], B[4];
    if (ALIGNED) {
        load_packed16<PIX>(p.pix + (size_t)frame * p.plane_stride + (rowoff + (unsigned)mcu_x * (16u * PIX)), p.swap_rb != 0, R, G, B);
    } else {
        const uint8_t* pr = p.r + (size_t)frame * p.plane_stride + rowoff;
        const uint8_t* pg = p.g + (size_t)frame * p.plane_stride + rowoff;
        const uint8_t* pb = p.b + (size_t)frame * p.plane_stride + rowoff;
#pragma unroll
        for (int w4 = 0; w4 < 4; ++w4) {
            uint32_t ar = 0, ag = 0, ab = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned x = (unsigned)min(mcu_x * 16 + w4 * 4 + k, W - 1) * (unsigned)PIX;   // ref :104
                ar |= (uint32_t)pr[x] << (8 * k);
                ag |= (uint32_t)pg[x] << (8 * k);
                ab |= (uint32_t)pb[x] << (8 * k);
            }
            R[w4] = ar; G[w4] = ag; B[w4] = ab;
        }
    }
#ifdef JPEZY_TRACE
    QuadTrace tr;                                                         // (the wave trace follows the planar kernel only)
#if JPEZY_TRACE >= 3
    unsigned long long* ph = tr.ph;
#endif
#endif
    encode_quad<GRAY, FORCE, false, DCG>(p, R, G, B, lds, lane, mcu_y, quad_x, frame, qidx, nullptr, nullptr, nullptr QUAD_TRACE_ARG);
}

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

template <bool GRAY, bool ALIGNED, int EW, bool DCG>
static void enc_f32_launch3(const EncParams& p, int force, dim3 grid, hipStream_t s)
{
    if (force == 1)
        hipLaunchKernelGGL((f32::fdct_quant_f32_kernel<GRAY, ALIGNED, 1, EW, DCG>), grid, dim3(64 * EW), 0, s, p);
    else if (force == 2)
        hipLaunchKernelGGL((f32::fdct_quant_f32_kernel<GRAY, ALIGNED, 2, EW, DCG>), grid, dim3(64 * EW), 0, s, p);
    else if (force == 3)
        hipLaunchKernelGGL((f32::fdct_quant_f32_kernel<GRAY, ALIGNED, 3, EW, DCG>), grid, dim3(64 * EW), 0, s, p);
    else
        hipLaunchKernelGGL((f32::fdct_quant_f32_kernel<GRAY, ALIGNED, 0, EW, DCG>), grid, dim3(64 * EW), 0, s, p);
}

template <bool GRAY, bool ALIGNED, int EW>
static void enc_f32_launch2(const EncParams& p, int force, dim3 grid, hipStream_t s)
{
    // the DC through the generic quantiser where jpezy_ctx_create verified it for this build's constants (both tables), else on its
    // own path from the exact table -- a second instance of the kernel, so that the common one carries no trace of the DC path
    if (p.dc_rq[0] != 0.f && p.dc_rq[1] != 0.f) enc_f32_launch3<GRAY, ALIGNED, EW, true>(p, force, grid, s);
    else enc_f32_launch3<GRAY, ALIGNED, EW, false>(p, force, grid, s);
}

hipError_t launch_fdct_quant_f32(const EncParams& p0, bool gray, int force, hipStream_t stream)
{
    EncParams p = p0;
    const bool al = (p.W % 16 == 0) && (p.plane_stride % 16 == 0) &&
                    (((uintptr_t)p.r | (uintptr_t)p.g | (uintptr_t)p.b) % 16 == 0);
    // four quads per workgroup with the cooperative load where the rows divide evenly, two with direct loads elsewhere
    const int ew = (al && p.quads_per_row % 4 == 0) ? 4 : 2;
    p.groups_per_row = (p.quads_per_row + ew - 1) / ew;
    const long groups = (long)p.mcu_rows * p.groups_per_row;
    if (groups <= 0 || p.n_frames <= 0) return hipSuccess;
    if (p.n_frames > 65535) return hipErrorInvalidValue;               // grid.y limit; callers chunk larger batches
    fast_div_setup((unsigned)p.groups_per_row, &p.gpr_magic, &p.gpr_shift);
    const dim3 grid((unsigned)groups, (unsigned)p.n_frames);
    if (ew == 4) {
        if (gray) enc_f32_launch2<true, true, 4>(p, force, grid, stream); else enc_f32_launch2<false, true, 4>(p, force, grid, stream);
    } else if (gray) {
        if (al) enc_f32_launch2<true, true, 2>(p, force, grid, stream); else enc_f32_launch2<true, false, 2>(p, force, grid, stream);
    } else {
        if (al) enc_f32_launch2<false, true, 2>(p, force, grid, stream); else enc_f32_launch2<false, false, 2>(p, force, grid, stream);
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
