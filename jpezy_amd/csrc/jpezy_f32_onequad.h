// jpezy_f32_onequad.h -- the one-quad-per-wave kernels of the f32 encode path for RGB input, planar and packed: step 1 (the pixel load)
// in front of jpezy_f32_quad.h's arithmetic.  A header because two files instantiate them: jpezy_kernels_f32.hip the default instances
// (point-sampled chroma), jpezy_kernels_f32_avg.hip the instances with the averaged chroma stage (AVG, JPEZY_DOWNSAMPLE_AVERAGE).
#pragma once
#include "jpezy_f32_quad.h"

namespace jpezy_dev {
namespace f32 {

// COOP: the workgroup's waves fetch its pixels together (below).  Four-wave workgroups always do, two-wave workgroups where the
// launcher asks for it (jpezy_kernels_f32.hip: three forms -- {4 waves, cooperative}, {2 waves, cooperative}, {2 waves, direct}).
template <bool GRAY, bool ALIGNED, int FORCE, int EWPB, bool DCG, bool AVG = false, bool COOP = ALIGNED && EWPB == 4>
__global__ __launch_bounds__(64 * EWPB, AVG && !ALIGNED ? AVG_BYTELOOP_WAVES : JPEZY_F32_WAVES) void fdct_quant_f32_kernel(EncParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[EWPB][WAVE_LDS_DWORDS];
    static_assert(!COOP || (ALIGNED && (EWPB == 4 || EWPB == 2)), "the cooperative load is written for 4 x 4 rows of 256 bytes and 2 x 8 rows of 128");
    // geometry of the staged image: a row of the workgroup is 64 * EWPB bytes = COOP_LPR pieces of 16, a wave fetches COOP_RPW rows
    constexpr int COOP_LPR = 4 * EWPB, COOP_RPW = 64 / COOP_LPR, COOP_ROW = 64 * EWPB, COOP_PLANE = 16 * COOP_ROW;
    static_assert(!COOP || 3 * COOP_PLANE <= EWPB * WAVE_LDS_DWORDS * 4, "the pixel staging area lies over the waves' slices");

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
        // Two waves: 128 x 16 pixels, wave w fetches rows 8w .. 8w+7, 8 lanes per row (8 rows of 128 bytes = whole 128-byte lines
        // per row), and piece c of row r lies at position c ^ (r & 4): a 16-lane read group holds the wave's four pieces of two
        // even and two odd rows, each pair one with and one without bit 2 ({0,6} {3,5} / {2,4} {1,7}), and a row's parity picks
        // the half of the 64 banks -- 16 different bank groups again (tools/profile/lds_bank_model.py: 12 cycles for the 3 reads).
        char* stg = reinterpret_cast<char*>(&lds_all[0][0]);
        {
            const int lr = lane / COOP_LPR, cp = lane % COOP_LPR;
            const int swz = EWPB == 4 ? 4 * lr : (lr & 4);
            const int y = min(mcu_y * 16 + wave * COOP_RPW + lr, H - 1);              // edge replication, ref :101
            const int piece = min(gx * COOP_LPR + (cp ^ swz), p.mcu_cols - 1);        // W % 16 == 0 here: a piece is an MCU column
            const unsigned off = (unsigned)y * (unsigned)W + (unsigned)piece * 16u;   // W, H <= 65535 (launcher): fits 32 bits
            typedef __attribute__((address_space(1))) const void* gptr;
            typedef __attribute__((address_space(3))) void* lptr;
            __builtin_amdgcn_global_load_lds((gptr)(pr + off), (lptr)(stg + wave * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr)(pg + off), (lptr)(stg + COOP_PLANE + wave * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr)(pb + off), (lptr)(stg + 2 * COOP_PLANE + wave * 1024), 16, 0, 0);
        }
        __syncthreads();                                   // waits for this wave's DMA (vmcnt) and for the other waves
        {
            const int swz = EWPB == 4 ? 4 * (row & 3) : (row & 4);
            const char* src = stg + row * COOP_ROW + (((wave * 4 + m) ^ swz) * 16);
            const uint4 vr = *reinterpret_cast<const uint4*>(src);
            const uint4 vg = *reinterpret_cast<const uint4*>(src + COOP_PLANE);
            const uint4 vb = *reinterpret_cast<const uint4*>(src + 2 * COOP_PLANE);
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
    encode_quad<GRAY, FORCE, false, DCG, false, AVG>(p, R, G, B, lds, lane, mcu_y, quad_x, frame, qidx, nullptr, nullptr, nullptr QUAD_TRACE_ARG);
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

template <bool GRAY, bool ALIGNED, int FORCE, int EWPB, bool DCG, int PIX, bool AVG = false>
__global__ __launch_bounds__(64 * EWPB, AVG && !ALIGNED ? AVG_BYTELOOP_WAVES : JPEZY_F32_WAVES) void fdct_quant_f32_packed_kernel(EncParams p)
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
    encode_quad<GRAY, FORCE, false, DCG, false, AVG>(p, R, G, B, lds, lane, mcu_y, quad_x, frame, qidx, nullptr, nullptr, nullptr QUAD_TRACE_ARG);
}

}  // namespace f32
}  // namespace jpezy_dev
