// jpezy_kernels_f32_444.hip -- the f32 encode kernel for 4:4:4 chroma sampling (JPEZY_SAMPLING_444, include/jpezy_hip.h): 8 x 8 MCUs of
// three blocks Y, Cb, Cr, every pixel converted, nothing decimated.  The arithmetic is the quad kernel's (jpezy_f32_quad.h): the packed
// 8-point transform, the colour estimates with their guard tests, the quantiser with its level-1 guard band, levels 2 and 3 and the
// DC paths are CALLED from there, not restated -- the F32Column records and delta1 are per (table, block column) and do not know the
// sampling (a chroma sample has the same range either way).  What is this file's own: the work unit, the LDS geometry, the load step.
//
// Work unit: an OCTET of 8 horizontally adjacent MCUs per wave, lane = 8 * row + MCU (row 0..7): 8 bytes of each plane per lane, 24
// blocks and 3 KB of contiguous output per wave -- the block count and output footprint of a quad.  Per component (Y, then Cb, then Cr):
// the lane's 8 samples -> row pass -> transpose tile -> column pass -> quantiser -> staged block; then the queued coefficients, then
// three whole-line stores per lane.  The raw pixel words (6 registers) live until the Cr samples are formed; the integer samples of all
// three components stay in registers (24) for levels 2 and 3, as YL / YR / CS do in the quad.
//
// LDS per wave (6400 bytes, the quad's): transpose tile 8 MCUs x 68 dwords (rows 8 dwords apart; 68 == 4 mod 32: the column reads of a
// 32-lane group -- 8 MCUs x 4 adjacent columns -- hit banks 4 m + c, all different; a row's two 16-byte writes over 8 lanes cover
// 32 banks once) = 2176 bytes, one component at a time; behind it the staging area of 24 blocks x STG_BLK; behind that the queue.
#include "jpezy_f32_quad.h"

namespace jpezy_dev {
namespace f32 {

constexpr int O_PITCH = 8;
constexpr int O_MCU = 68;
constexpr int O_TILE_BYTES = 8 * O_MCU * 4;                 // 2176
constexpr int O_STG_BYTES = 24 * STG_BLK;                   // 3456
constexpr int O_WAVE_DWORDS = (O_TILE_BYTES + O_STG_BYTES) / 4 + JPEZY_QUEUE_DWORDS;
constexpr int OWPB = 4;                                     // waves (octets) per workgroup; they share nothing
// Waves per SIMD the register allocation aims at: 4 (128 VGPRs).  At the quad kernel's 5 (96 VGPRs) this kernel spills ~250 bytes per
// lane: three components' samples stay live for levels 2 and 3 where the quad holds two block rows and a half-filled chroma row.
constexpr int O_WAVES = 4;
static_assert(O_TILE_BYTES >= 24 * 64, "the per-lane evaluator keeps the octet's samples as bytes in the tile");
static_assert(O_TILE_BYTES % 16 == 0 && STG_BLK % 16 == 0, "16-byte reads of the staged blocks");

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

// 8 packed pixels (24 or 32 bytes, 8-byte / 16-byte aligned) -> two words per channel; load_packed16's selectors
template <int PIX>
__device__ __forceinline__ void load_packed8(const uint8_t* src, bool swap_rb, uint32_t* R, uint32_t* G, uint32_t* B)
{
    if (PIX == 3) {
        const uint32_t a1 = swap_rb ? 0x00000502u : 0x00060300u, a2 = swap_rb ? 0x07040100u : 0x05020100u;   // red
        const uint32_t c1 = swap_rb ? 0x00060300u : 0x00000502u, c2 = swap_rb ? 0x05020100u : 0x07040100u;   // blue
        const uint2* s2 = reinterpret_cast<const uint2*>(src);
        const uint2 v0 = s2[0], v1 = s2[1], v2 = s2[2];
        const uint32_t w[6] = { v0.x, v0.y, v1.x, v1.y, v2.x, v2.y };
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const uint32_t w0 = w[3 * q], w1 = w[3 * q + 1], w2 = w[3 * q + 2];
            R[q] = __builtin_amdgcn_perm(w2, __builtin_amdgcn_perm(w1, w0, a1), a2);
            G[q] = __builtin_amdgcn_perm(w2, __builtin_amdgcn_perm(w1, w0, 0x00070401u), 0x06020100u);
            B[q] = __builtin_amdgcn_perm(w2, __builtin_amdgcn_perm(w1, w0, c1), c2);
        }
    } else {
        const uint32_t a = swap_rb ? 0x07060302u : 0x05040100u, c = swap_rb ? 0x05040100u : 0x07060302u;
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const uint4 v = s4[q];
            const uint32_t u01 = __builtin_amdgcn_perm(v.y, v.x, 0x06020400u), u23 = __builtin_amdgcn_perm(v.w, v.z, 0x06020400u);
            const uint32_t v01 = __builtin_amdgcn_perm(v.y, v.x, 0x00000501u), v23 = __builtin_amdgcn_perm(v.w, v.z, 0x00000501u);
            R[q] = __builtin_amdgcn_perm(u23, u01, a);
            G[q] = __builtin_amdgcn_perm(v23, v01, 0x05040100u);
            B[q] = __builtin_amdgcn_perm(u23, u01, c);
        }
    }
}

// four samples of a row in natural order as signed bytes (the per-lane evaluator's input)
__device__ __forceinline__ uint32_t pack4(const f2* A, int x0)
{
    return ((uint32_t)(int)pick(A, x0) & 0xFFu) | (((uint32_t)(int)pick(A, x0 + 1) & 0xFFu) << 8) |
           (((uint32_t)(int)pick(A, x0 + 2) & 0xFFu) << 16) | (((uint32_t)(int)pick(A, x0 + 3) & 0xFFu) << 24);
}

// EncParams as the 4:4:4 entry points fill it: mcu_cols / mcu_rows count 8 x 8 MCUs, quads_per_row = OCTETS per MCU row,
// coeffs_per_frame = 192 * mcu_cols * mcu_rows.
// ALIGNED: W % 8 == 0, bases and strides multiples of 8 (packed: of 16): 8-byte loads of the planes (PIX == 0) or 24 / 32 contiguous
// bytes of packed pixels separated in registers (PIX == 3 / 4).  !ALIGNED (PIX == 0 only): the byte loop with edge clamping over the
// three channel pointers, pixels p.pix_bytes apart (planes: 1) -- planar and packed input alike; the test hooks' instances (FORCE != 0)
// exist in this form only.
template <bool ALIGNED, int FORCE, bool DCG, int PIX>
__global__ __launch_bounds__(64 * OWPB, O_WAVES) void fdct_quant_f32_444_kernel(EncParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[OWPB][O_WAVE_DWORDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int mcu_y = (int)fast_div(blockIdx.x, p.gpr_magic, p.gpr_shift);
    const int gx = (int)blockIdx.x - mcu_y * p.groups_per_row;
    const int oct_x = gx * OWPB + wave;
    if (oct_x >= p.quads_per_row) return;                                 // wave-uniform; the waves never meet at a barrier
    const unsigned qidx = (unsigned)(mcu_y * p.quads_per_row + oct_x);
    const int frame = (int)blockIdx.y;
    uint32_t* lds = lds_all[wave];
    float* ldsf = reinterpret_cast<float*>(lds);
    char* stage = reinterpret_cast<char*>(lds) + O_TILE_BYTES;
    unsigned* queue = lds + (O_TILE_BYTES + O_STG_BYTES) / 4;             // [0] = count, then 16-bit entries
    const int row = lane >> 3, m = lane & 7;
    const bool live = oct_x * 8 + m < p.mcu_cols;
    const int mcu_x = min(oct_x * 8 + m, p.mcu_cols - 1);                 // a dead MCU slot repeats the row's last MCU and stores nothing
    const int W = p.W, H = p.H;
    const DeviceTables* tab = p.tab;
    if (lane == 0) queue[0] = 0;

    // ---- 1. this lane's 8-pixel row segment ----
    uint32_t R[2], G[2], B[2];
    {
        const int y = min(mcu_y * 8 + row, H - 1);                        // clamped extension to whole MCUs, ref :101
        const bool packed = p.pix_bytes != 0;                             // wave-uniform
        // W, H <= 65535 and row_stride * H < 2^32 (the entry points): fits 32 bits
        const unsigned rowoff = (unsigned)y * (PIX != 0 || packed ? p.row_stride : (unsigned)W);
        const size_t fo = (size_t)frame * p.plane_stride;
        if (ALIGNED && PIX != 0) {
            load_packed8<PIX>(p.pix + fo + (rowoff + (unsigned)mcu_x * (8u * PIX)), p.swap_rb != 0, R, G, B);
        } else if (ALIGNED) {
            const unsigned off = rowoff + (unsigned)mcu_x * 8u;
            const uint2 vr = *reinterpret_cast<const uint2*>(p.r + fo + off);
            const uint2 vg = *reinterpret_cast<const uint2*>(p.g + fo + off);
            const uint2 vb = *reinterpret_cast<const uint2*>(p.b + fo + off);
            R[0] = vr.x; R[1] = vr.y; G[0] = vg.x; G[1] = vg.y; B[0] = vb.x; B[1] = vb.y;
        } else {
            const uint8_t* pr = p.r + fo + rowoff;
            const uint8_t* pg = p.g + fo + rowoff;
            const uint8_t* pb = p.b + fo + rowoff;
            const unsigned step = packed ? (unsigned)p.pix_bytes : 1u;
#pragma unroll
            for (int w2 = 0; w2 < 2; ++w2) {
                uint32_t ar = 0, ag = 0, ab = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned x = (unsigned)min(mcu_x * 8 + w2 * 4 + k, W - 1) * step;   // ref :104
                    ar |= (uint32_t)pr[x] << (8 * k);
                    ag |= (uint32_t)pg[x] << (8 * k);
                    ab |= (uint32_t)pb[x] << (8 * k);
                }
                R[w2] = ar; G[w2] = ag; B[w2] = ab;
            }
        }
    }

    PkCos kc = pk_cos();
    asm volatile("" : "+s"(kc.k13), "+s"(kc.k37), "+s"(kc.k51), "+s"(kc.k75), "+s"(kc.k26));   // as encode_quad_compute
    // the lane at position cq of a block row handles the natural column j = pair_row(cq) (the row pass stores in pair order)
    const int cq = row, j = (int)((0x75316240u >> (4 * cq)) & 7u);
    const unsigned ju = (unsigned)j;
    const F32Column* lcol = &tab->f32col[0][ju];
    const uint32_t zz_lo = lcol->zz_lo, zz_hi = lcol->zz_hi;
    const bool DCF = p.dc_rq[0] != 0.f && p.dc_rq[1] != 0.f;
    char* sbase = stage + (m * 3) * STG_BLK;                              // this lane's first block; Cb and Cr are immediates away
    float* trow = ldsf + m * O_MCU + row * O_PITCH;
    const float* tcol = ldsf + m * O_MCU + cq;

    // ---- 2-5. per component: samples, row pass, transpose, column pass, quantise + zig-zag into the staging area ----
    f2 S[3][4];
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
        const int t = comp ? 1 : 0;
        f2 ks[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) ks[k] = f2{ lcol[8 * t].ks[2 * k], lcol[8 * t].ks[2 * k + 1] };
        const f2 dd = f2{ lcol[8 * t].delta1[0], lcol[8 * t].delta1[1] };
        const float th = lcol[8 * t].th;
        if (comp == 0) luma8(R, G, B, S[0]);
        else if (comp == 1) chroma8<false>(R, G, B, S[1]);
        else chroma8<true>(R, G, B, S[2]);
        __builtin_amdgcn_sched_barrier(0);   // keep the phases apart, as PHASE_FENCE does in the quad: overlapped they need more registers
        {
            f2 X[4];
            fdct8p(S[comp], X, kc);
            f2* dst = reinterpret_cast<f2*>(trow);
            dst[0] = X[0]; dst[1] = X[1]; dst[2] = X[2]; dst[3] = X[3];
        }
        wave_sync();
        __builtin_amdgcn_sched_barrier(0);
        f2 col[4], F[4];
        lds_column<O_PITCH>(tcol, col);
        wave_sync();                                                      // tile consumed: the next component's rows may land
        __builtin_amdgcn_sched_barrier(0);
        fdct8p(col, F, kc);
        const int dc = DCG ? 0 : DCF ? dc_formula(F[0].x, p.dc_rq[t], p.dc_bias[t]) : dc_lookup(F[0].x, t ? p.dcq_chroma : p.dcq_luma);
        quant_block_column<DCG>(F, ks, dd, th, j, dc, p.dc_rq[t], p.dc_bias[t], live, sbase, zz_lo, zz_hi, comp * STG_BLK, m * 3 + comp,
                                queue, FORCE != 0
#ifdef JPEZY_DUMP_T
                                , nullptr
#endif
        );
        __builtin_amdgcn_sched_barrier(0);   // keep the components apart: overlapped they need more registers
    }
    wave_sync();

    // ---- 5b. levels 2 and 3 for the queued coefficients (FORCE 1/2: every coefficient of the octet) ----
    const unsigned nq = queue[0];
    if (FORCE == 3 || (FORCE == 0 && nq > (unsigned)QUEUE_CAP)) {
        // the queue-overflow case of encode_quad_compute: every lane evaluates the 24 coefficients of its three block columns in the
        // reference's order (ref :146-166) from the samples, which go to the dead tile as bytes: block (m, comp) at (3 m + comp) * 64
        signed char* smp = reinterpret_cast<signed char*>(lds);
#pragma unroll
        for (int comp = 0; comp < 3; ++comp) {
            uint32_t* d = reinterpret_cast<uint32_t*>(smp + (m * 3 + comp) * 64 + row * 8);
            d[0] = pack4(S[comp], 0); d[1] = pack4(S[comp], 4);
        }
        wave_sync();
        const double cu = j ? 1.0 : JPEZY_S;
#pragma unroll 1
        for (int comp = 0; comp < 3; ++comp) {
            const int blk = m * 3 + comp, tbl = comp ? 1 : 0;
            const signed char* src = smp + blk * 64;
            double A[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll 1
            for (int y = 0; y < 8; ++y) {
#pragma unroll 1
                for (int x = 0; x < 8; ++x) {
                    const double px = (double)(int)src[y * 8 + x] * c_cos[j * 8 + x];
#pragma unroll
                    for (int i = 0; i < 8; ++i) A[i] += px * c_cos[i * 8 + y];
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const double cv = i ? 1.0 : JPEZY_S;
                const int dct = (int)(A[i] * cu * cv / 4);
                const int qv = dct / tab->qt[tbl][i * 8 + j];
                *reinterpret_cast<int16_t*>(stage + blk * STG_BLK + 2 * (int)c_zzinv[i * 8 + j]) = (int16_t)qv;
            }
        }
        if (lane == 0) atomicAdd(p.fallback_count + (qidx & (COUNTER_SHARDS - 1)), (unsigned long long)(24 * 64));
        wave_sync();
    } else {
        const bool all = FORCE != 0;
        const unsigned total = all ? (unsigned)(24 * 64) : nq;
        if (total) {
            const int valid_mcus = min(8, p.mcu_cols - oct_x * 8);
            unsigned done = 0;
#pragma unroll 1
            for (unsigned e = 0; e < total; ++e) {
                const unsigned code = all ? e : reinterpret_cast<const unsigned short*>(queue + 1)[e];
                const int blk = __builtin_amdgcn_readfirstlane((int)(code >> 6)), nat = __builtin_amdgcn_readfirstlane((int)(code & 63));
                const int em = blk / 3, comp = blk - em * 3;
                if (em >= valid_mcus) continue;
                const int ei = nat >> 3, ej = nat & 7, tbl = comp ? 1 : 0;
                // the 8 lanes that hold the block's rows: lanes em, em + 8, .., em + 56, row y on lane 8 y + em
                float w[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) w[k] = comp == 0 ? pick(S[0], k) : comp == 1 ? pick(S[1], k) : pick(S[2], k);
                const int Q = tab->qt[tbl][nat];
                const double qinv = tab->qinv[tbl][nat];
                const int zpos = c_zzinv[nat];
                const int qv = resolve_coef<FORCE, false>(w, m == em, row, em, 8, ei, ej, Q, qinv, nullptr);
                if (lane == 0) *reinterpret_cast<int16_t*>(stage + blk * STG_BLK + 2 * zpos) = (int16_t)qv;
                ++done;
            }
            if (lane == 0 && done) atomicAdd(p.fallback_count + (qidx & (COUNTER_SHARDS - 1)), (unsigned long long)done);
            wave_sync();
        }
    }

    // ---- 6. coalesced store: the octet's blocks are contiguous in the coefficient buffer (24 x 128 bytes), three 16-byte chunks per lane
    {
        const int valid_chunks = min(8, p.mcu_cols - oct_x * 8) * 3 * 8;
        int16_t* gbase = p.coeffs + (size_t)frame * p.coeffs_per_frame + ((size_t)mcu_y * p.mcu_cols + (size_t)oct_x * 8) * 192;
        uint4* g4 = reinterpret_cast<uint4*>(gbase);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int c = k * 64 + lane;
            if (c < valid_chunks) {
                const uint4 v = *reinterpret_cast<const uint4*>(stage + (c >> 3) * STG_BLK + (c & 7) * 16);
                nt_store16(g4 + c, v);
            }
        }
    }
}

}  // namespace f32

template <bool DCG>
static void enc_f32_444_launch(const EncParams& p, bool al, int force, dim3 grid, hipStream_t s)
{
    const dim3 block(64 * f32::OWPB);
    if (force == 1) hipLaunchKernelGGL((f32::fdct_quant_f32_444_kernel<false, 1, DCG, 0>), grid, block, 0, s, p);
    else if (force == 2) hipLaunchKernelGGL((f32::fdct_quant_f32_444_kernel<false, 2, DCG, 0>), grid, block, 0, s, p);
    else if (force == 3) hipLaunchKernelGGL((f32::fdct_quant_f32_444_kernel<false, 3, DCG, 0>), grid, block, 0, s, p);
    else if (!al) hipLaunchKernelGGL((f32::fdct_quant_f32_444_kernel<false, 0, DCG, 0>), grid, block, 0, s, p);
    else if (p.pix_bytes == 3) hipLaunchKernelGGL((f32::fdct_quant_f32_444_kernel<true, 0, DCG, 3>), grid, block, 0, s, p);
    else if (p.pix_bytes == 4) hipLaunchKernelGGL((f32::fdct_quant_f32_444_kernel<true, 0, DCG, 4>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((f32::fdct_quant_f32_444_kernel<true, 0, DCG, 0>), grid, block, 0, s, p);
}

// planar (p.pix_bytes == 0) and packed (3 / 4) input; force as launch_fdct_quant_f32
hipError_t launch_fdct_quant_f32_444(const EncParams& p0, int force, hipStream_t stream)
{
    EncParams p = p0;
    if (p.pix_bytes != 0 && p.pix_bytes != 3 && p.pix_bytes != 4) return hipErrorInvalidValue;
    if (p.n_frames > 65535) return hipErrorInvalidValue;                  // grid.y limit; callers chunk larger batches
    bool al;
    if (p.pix_bytes) al = p.W % 8 == 0 && p.row_stride % 16 == 0 && p.plane_stride % 16 == 0 && (uintptr_t)p.pix % 16 == 0;
    else al = p.W % 8 == 0 && p.plane_stride % 8 == 0 && (((uintptr_t)p.r | (uintptr_t)p.g | (uintptr_t)p.b) % 8 == 0);
    p.groups_per_row = (p.quads_per_row + f32::OWPB - 1) / f32::OWPB;
    const long groups = (long)p.mcu_rows * p.groups_per_row;
    if (groups <= 0 || p.n_frames <= 0) return hipSuccess;
    fast_div_setup((unsigned)p.groups_per_row, &p.gpr_magic, &p.gpr_shift);
    const dim3 grid((unsigned)groups, (unsigned)p.n_frames);
    if (p.dc_rq[0] != 0.f && p.dc_rq[1] != 0.f) enc_f32_444_launch<true>(p, al, force, grid, stream);
    else enc_f32_444_launch<false>(p, al, force, grid, stream);
    return hipGetLastError();
}

}  // namespace jpezy_dev
