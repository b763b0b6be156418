// jpezy_kernels_f32_422.hip -- the f32 encode kernel for 4:2:2 chroma sampling (JPEZY_SAMPLING_422, include/jpezy_hip.h): 16 x 8 MCUs of
// four blocks Y-left, Y-right, Cb, Cr; chroma decimated horizontally only -- point-sampled (the pixel at 2 x') or, with
// JPEZY_DOWNSAMPLE_AVERAGE, the libjpeg h2v1 average of the pair.  As in jpezy_kernels_f32_444.hip the arithmetic is the quad kernel's
// (jpezy_f32_quad.h): fdct8p, luma8, chroma_px2 / chroma_px_ref, lds_column, quant_block_column, resolve_coef, the DC paths and the three
// precision levels with their guard bands are CALLED from there, not restated.  What is this file's own: the work unit, the LDS geometry,
// the load step and the pick (or pair average) of the chroma samples.
//
// Work unit: 8 horizontally adjacent MCUs (128 x 8 pixels) per wave, lane = 8 * row + MCU (row 0..7): 16 bytes of each plane per lane,
// 32 blocks and 4 KB of contiguous output per wave.  Four component passes (Y-left, Y-right, Cb, Cr), each of eight blocks of one kind
// through the octet's transpose tile: the lane's 8 samples -> row pass -> tile -> column pass -> quantiser -> staged block; then the
// queued coefficients, then four whole-line stores per lane.  The integer samples of all four passes stay in registers (32) for levels 2
// and 3.
//
// LDS per wave (7552 bytes): the octet's transpose tile, 8 MCUs x 68 dwords (rows 8 dwords apart; the bank argument of
// jpezy_kernels_f32_444.hip carries over unchanged, a pass is eight blocks of one kind there too) = 2176 bytes; behind it the staging area
// of 32 blocks x STG_BLK; behind that the queue.  A workgroup of four waves takes 30208 bytes: five workgroups, 20 waves, fit the CU's
// 160 KB -- more than the 12 the register allocation admits.
//
// The averaged stage needs no cross-lane traffic (a pair lies inside the lane's row segment; h2v2 needs the neighbouring row's lane): it
// converts all 16 pixels of the row to exact truncated Cb / Cr -- chroma_px2's estimate and guard test, chroma_px_ref where it fires -- and
// forms floor((a + b + bias) / 2), bias 0 for even x', 1 for odd x' (an MCU starts at an even x', so the parity is the sample's index in
// the lane); small integers and a power-of-two scale: every step exact in FP32.
#include "jpezy_f32_onequad.h"   // load_packed16

namespace jpezy_dev {
namespace f32 {

constexpr int H_PITCH = 8;
constexpr int H_MCU = 68;
constexpr int H_TILE_BYTES = 8 * H_MCU * 4;                 // 2176
constexpr int H_BLOCKS = 32;                                // 8 MCUs x 4
constexpr int H_STG_BYTES = H_BLOCKS * STG_BLK;             // 4608
constexpr int H_WAVE_DWORDS = (H_TILE_BYTES + H_STG_BYTES) / 4 + JPEZY_QUEUE_DWORDS;
constexpr int HWPB = 4;                                     // waves per workgroup; they share nothing
// Waves per SIMD the register allocation aims at: 3 (168 VGPRs), by measurement.  At the 4:4:4 kernel's 4 (128 VGPRs) the point-sampled
// instances spill 20-120 bytes per lane and the averaged ones 120-180 (32 sample registers stay live for levels 2 and 3, and the averaged
// stage converts 16 pixels of two components); a 4096 x 4096 frame then takes 38.0 us instead of 36.8 (random pixels), 34.2 instead of
// 31.4 (smooth) and, averaged, 121 us instead of 59.5.  At 3 the point-sampled instances use 142-152 VGPRs and no scratch.
constexpr int H_WAVES = 3;
static_assert(H_TILE_BYTES >= H_BLOCKS * 64, "the per-lane evaluator keeps the unit's samples as bytes in the tile");
static_assert(H_TILE_BYTES % 16 == 0 && STG_BLK % 16 == 0, "16-byte reads of the staged blocks");
static_assert(((H_BLOCKS - 1) << 6 | 63) < 65536, "a queue entry (block, natural position) fits 16 bits");

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

// four samples of a row in natural order as signed bytes (the per-lane evaluator's input)
__device__ __forceinline__ uint32_t pack4_422(const f2* A, int x0)
{
    return ((uint32_t)(int)pick(A, x0) & 0xFFu) | (((uint32_t)(int)pick(A, x0 + 1) & 0xFFu) << 8) |
           (((uint32_t)(int)pick(A, x0 + 2) & 0xFFu) << 16) | (((uint32_t)(int)pick(A, x0 + 3) & 0xFFu) << 24);
}

// EncParams as the 4:2:2 entry points fill it: mcu_cols counts 16-pixel, mcu_rows 8-pixel MCUs, quads_per_row = work units (8 MCUs) per
// MCU row, coeffs_per_frame = 256 * mcu_cols * mcu_rows.
// ALIGNED: W % 16 == 0, bases and strides multiples of 16: one 16-byte load of each plane (PIX == 0) or 48 / 64 contiguous bytes of
// packed pixels separated in registers (PIX == 3 / 4, load_packed16).  !ALIGNED (PIX == 0 only): the byte loop with edge clamping over
// the three channel pointers, pixels p.pix_bytes apart (planes: 1) -- planar and packed input alike; the test hooks' instances
// (FORCE != 0) exist in this form only.  AVG: the averaged chroma stage.
template <bool ALIGNED, int FORCE, bool DCG, int PIX, bool AVG>
__global__ __launch_bounds__(64 * HWPB, H_WAVES) void fdct_quant_f32_422_kernel(EncParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[HWPB][H_WAVE_DWORDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int mcu_y = (int)fast_div(blockIdx.x, p.gpr_magic, p.gpr_shift);
    const int gx = (int)blockIdx.x - mcu_y * p.groups_per_row;
    const int unit_x = gx * HWPB + wave;
    if (unit_x >= p.quads_per_row) return;                                // wave-uniform; the waves never meet at a barrier
    const unsigned qidx = (unsigned)(mcu_y * p.quads_per_row + unit_x);
    const int frame = (int)blockIdx.y;
    uint32_t* lds = lds_all[wave];
    float* ldsf = reinterpret_cast<float*>(lds);
    char* stage = reinterpret_cast<char*>(lds) + H_TILE_BYTES;
    unsigned* queue = lds + (H_TILE_BYTES + H_STG_BYTES) / 4;             // [0] = count, then 16-bit entries
    const int row = lane >> 3, m = lane & 7;
    const bool live = unit_x * 8 + m < p.mcu_cols;
    const int mcu_x = min(unit_x * 8 + m, p.mcu_cols - 1);                // a dead MCU slot repeats the row's last MCU and stores nothing
    const int W = p.W, H = p.H;
    const DeviceTables* tab = p.tab;
    if (lane == 0) queue[0] = 0;

    // ---- 1. this lane's 16-pixel row segment ----
    uint32_t R[4], G[4], B[4];
    {
        const int y = min(mcu_y * 8 + row, H - 1);                        // clamped extension to whole MCUs
        const bool packed = p.pix_bytes != 0;                             // wave-uniform
        // W, H <= 65535 and row_stride * H < 2^32 (the entry points): fits 32 bits
        const unsigned rowoff = (unsigned)y * (PIX != 0 || packed ? p.row_stride : (unsigned)W);
        const size_t fo = (size_t)frame * p.plane_stride;
        if (ALIGNED && PIX != 0) {
            load_packed16<PIX>(p.pix + fo + (rowoff + (unsigned)mcu_x * (16u * PIX)), p.swap_rb != 0, R, G, B);
        } else if (ALIGNED) {
            const unsigned off = rowoff + (unsigned)mcu_x * 16u;
            const uint4 vr = *reinterpret_cast<const uint4*>(p.r + fo + off);
            const uint4 vg = *reinterpret_cast<const uint4*>(p.g + fo + off);
            const uint4 vb = *reinterpret_cast<const uint4*>(p.b + fo + off);
            R[0] = vr.x; R[1] = vr.y; R[2] = vr.z; R[3] = vr.w;
            G[0] = vg.x; G[1] = vg.y; G[2] = vg.z; G[3] = vg.w;
            B[0] = vb.x; B[1] = vb.y; B[2] = vb.z; B[3] = vb.w;
        } else {
            const uint8_t* pr = p.r + fo + rowoff;
            const uint8_t* pg = p.g + fo + rowoff;
            const uint8_t* pb = p.b + fo + rowoff;
            const unsigned step = packed ? (unsigned)p.pix_bytes : 1u;
#pragma unroll
            for (int w4 = 0; w4 < 4; ++w4) {
                uint32_t ar = 0, ag = 0, ab = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned x = (unsigned)min(mcu_x * 16 + w4 * 4 + k, W - 1) * step;
                    ar |= (uint32_t)pr[x] << (8 * k);
                    ag |= (uint32_t)pg[x] << (8 * k);
                    ab |= (uint32_t)pb[x] << (8 * k);
                }
                R[w4] = ar; G[w4] = ag; B[w4] = ab;
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
    char* sbase = stage + (m * 4) * STG_BLK;                              // this lane's first block; the other three are immediates away
    float* trow = ldsf + m * H_MCU + row * H_PITCH;
    const float* tcol = ldsf + m * H_MCU + cq;

    // ---- 2-5. per pass: samples, row pass, transpose, column pass, quantise + zig-zag into the staging area ----
    // (the chroma passes in front of the luma passes, where only the pixel words are live beside the conversions, need MORE registers)
    f2 S[4][4];
#pragma unroll
    for (int comp = 0; comp < 4; ++comp) {
        const int t = comp >= 2 ? 1 : 0;
        f2 ks[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) ks[k] = f2{ lcol[8 * t].ks[2 * k], lcol[8 * t].ks[2 * k + 1] };
        const f2 dd = f2{ lcol[8 * t].delta1[0], lcol[8 * t].delta1[1] };
        const float th = lcol[8 * t].th;
        if (comp == 0) luma8(R, G, B, S[0]);
        else if (comp == 1) luma8(R + 2, G + 2, B + 2, S[1]);
        else if (comp == 2) {                                             // both chroma components; the pixel words die here
            if (AVG) chroma8_pairs(R, G, B, S[2], S[3]);
            else chroma8_even(R, G, B, S[2], S[3]);
        }
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
        lds_column<H_PITCH>(tcol, col);
        wave_sync();                                                      // tile consumed: the next pass' rows may land
        __builtin_amdgcn_sched_barrier(0);
        fdct8p(col, F, kc);
        const int dc = DCG ? 0 : DCF ? dc_formula(F[0].x, p.dc_rq[t], p.dc_bias[t]) : dc_lookup(F[0].x, t ? p.dcq_chroma : p.dcq_luma);
        quant_block_column<DCG>(F, ks, dd, th, j, dc, p.dc_rq[t], p.dc_bias[t], live, sbase, zz_lo, zz_hi, comp * STG_BLK, m * 4 + comp,
                                queue, FORCE != 0
#ifdef JPEZY_DUMP_T
                                , nullptr
#endif
        );
        __builtin_amdgcn_sched_barrier(0);   // keep the passes apart: overlapped they need more registers
    }
    wave_sync();

    // ---- 5b. levels 2 and 3 for the queued coefficients (FORCE 1/2: every coefficient of the unit) ----
    const unsigned nq = queue[0];
    if (FORCE == 3 || (FORCE == 0 && nq > (unsigned)QUEUE_CAP)) {
        // the queue-overflow case of encode_quad_compute: every lane evaluates the 32 coefficients of its four block columns in the
        // reference's order from the samples, which go to the dead tile as bytes: block (m, comp) at (4 m + comp) * 64
        signed char* smp = reinterpret_cast<signed char*>(lds);
#pragma unroll
        for (int comp = 0; comp < 4; ++comp) {
            uint32_t* d = reinterpret_cast<uint32_t*>(smp + (m * 4 + comp) * 64 + row * 8);
            d[0] = pack4_422(S[comp], 0); d[1] = pack4_422(S[comp], 4);
        }
        wave_sync();
        const double cu = j ? 1.0 : JPEZY_S;
#pragma unroll 1
        for (int comp = 0; comp < 4; ++comp) {
            const int blk = m * 4 + comp, tbl = comp >= 2 ? 1 : 0;
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
        if (lane == 0) atomicAdd(p.fallback_count + (qidx & (COUNTER_SHARDS - 1)), (unsigned long long)(H_BLOCKS * 64));
        wave_sync();
    } else {
        const bool all = FORCE != 0;
        const unsigned total = all ? (unsigned)(H_BLOCKS * 64) : nq;
        if (total) {
            const int valid_mcus = min(8, p.mcu_cols - unit_x * 8);
            unsigned done = 0;
#pragma unroll 1
            for (unsigned e = 0; e < total; ++e) {
                const unsigned code = all ? e : reinterpret_cast<const unsigned short*>(queue + 1)[e];
                const int blk = __builtin_amdgcn_readfirstlane((int)(code >> 6)), nat = __builtin_amdgcn_readfirstlane((int)(code & 63));
                const int em = blk >> 2, comp = blk & 3;
                if (em >= valid_mcus) continue;
                const int ei = nat >> 3, ej = nat & 7, tbl = comp >= 2 ? 1 : 0;
                // the 8 lanes that hold the block's rows: lanes em, em + 8, .., em + 56, row y on lane 8 y + em
                float w[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) w[k] = comp == 0 ? pick(S[0], k) : comp == 1 ? pick(S[1], k) : comp == 2 ? pick(S[2], k) : pick(S[3], k);
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

    // ---- 6. coalesced store: the unit's blocks are contiguous in the coefficient buffer (32 x 128 bytes), four 16-byte chunks per lane
    {
        const int valid_chunks = min(8, p.mcu_cols - unit_x * 8) * 4 * 8;
        int16_t* gbase = p.coeffs + (size_t)frame * p.coeffs_per_frame + ((size_t)mcu_y * p.mcu_cols + (size_t)unit_x * 8) * 256;
        uint4* g4 = reinterpret_cast<uint4*>(gbase);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = k * 64 + lane;
            if (c < valid_chunks) {
                const uint4 v = *reinterpret_cast<const uint4*>(stage + (c >> 3) * STG_BLK + (c & 7) * 16);
                nt_store16(g4 + c, v);
            }
        }
    }
}

}  // namespace f32

template <bool DCG, bool AVG>
static void enc_f32_422_launch(const EncParams& p, bool al, int force, dim3 grid, hipStream_t s)
{
    const dim3 block(64 * f32::HWPB);
    if (force == 1) hipLaunchKernelGGL((f32::fdct_quant_f32_422_kernel<false, 1, DCG, 0, AVG>), grid, block, 0, s, p);
    else if (force == 2) hipLaunchKernelGGL((f32::fdct_quant_f32_422_kernel<false, 2, DCG, 0, AVG>), grid, block, 0, s, p);
    else if (force == 3) hipLaunchKernelGGL((f32::fdct_quant_f32_422_kernel<false, 3, DCG, 0, AVG>), grid, block, 0, s, p);
    else if (!al) hipLaunchKernelGGL((f32::fdct_quant_f32_422_kernel<false, 0, DCG, 0, AVG>), grid, block, 0, s, p);
    else if (p.pix_bytes == 3) hipLaunchKernelGGL((f32::fdct_quant_f32_422_kernel<true, 0, DCG, 3, AVG>), grid, block, 0, s, p);
    else if (p.pix_bytes == 4) hipLaunchKernelGGL((f32::fdct_quant_f32_422_kernel<true, 0, DCG, 4, AVG>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((f32::fdct_quant_f32_422_kernel<true, 0, DCG, 0, AVG>), grid, block, 0, s, p);
}

// planar (p.pix_bytes == 0) and packed (3 / 4) input; force as launch_fdct_quant_f32; average: the JPEZY_DOWNSAMPLE_AVERAGE instances
hipError_t launch_fdct_quant_f32_422(const EncParams& p0, int force, bool average, hipStream_t stream)
{
    EncParams p = p0;
    if (p.pix_bytes != 0 && p.pix_bytes != 3 && p.pix_bytes != 4) return hipErrorInvalidValue;
    if (p.n_frames > 65535) return hipErrorInvalidValue;                  // grid.y limit; callers chunk larger batches
    bool al;
    if (p.pix_bytes) al = p.W % 16 == 0 && p.row_stride % 16 == 0 && p.plane_stride % 16 == 0 && (uintptr_t)p.pix % 16 == 0;
    else al = p.W % 16 == 0 && p.plane_stride % 16 == 0 && (((uintptr_t)p.r | (uintptr_t)p.g | (uintptr_t)p.b) % 16 == 0);
    p.groups_per_row = (p.quads_per_row + f32::HWPB - 1) / f32::HWPB;
    const long groups = (long)p.mcu_rows * p.groups_per_row;
    if (groups <= 0 || p.n_frames <= 0) return hipSuccess;
    fast_div_setup((unsigned)p.groups_per_row, &p.gpr_magic, &p.gpr_shift);
    const dim3 grid((unsigned)groups, (unsigned)p.n_frames);
    const bool dcg = p.dc_rq[0] != 0.f && p.dc_rq[1] != 0.f;
    if (average) {
        if (dcg) enc_f32_422_launch<true, true>(p, al, force, grid, stream);
        else enc_f32_422_launch<false, true>(p, al, force, grid, stream);
    } else {
        if (dcg) enc_f32_422_launch<true, false>(p, al, force, grid, stream);
        else enc_f32_422_launch<false, false>(p, al, force, grid, stream);
    }
    return hipGetLastError();
}

}  // namespace jpezy_dev
