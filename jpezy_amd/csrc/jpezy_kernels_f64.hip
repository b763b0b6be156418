// jpezy_kernels_f64.hip -- encode variant 0: the all-FP64 encode kernel for gfx950 (MI355X / CDNA4).
//
//   fdct_quant_kernel : RGB->YCbCr + 4:2:0 decimation + 8x8 FDCT + Annex-K quantise + zig-zag
//                       (ref encoder/jpezy_encoder.hpp:90-172, 244-256; jpezy.hpp:36-45,131-152)
//
// Kept as a second encoder written independently of the f32 path (jpezy_f32_quad.h, the default): the parity tests compare the
// two.  So its colour formulas (ref_y / ref_cb / ref_cr), its transform (fdct8) and its cosine and zig-zag tables are duplicated
// here ON PURPOSE and must not be shared with that path; only the wave-level plumbing (jpezy_wave.h) is common.
//
// Work decomposition: one 64-lane wavefront owns a "quad" = 4 horizontally adjacent 16x16 MCUs (64x16 pixels, 24 blocks); a
// workgroup is WPB = 2 independent waves, two adjacent quads (no s_barrier -- each wave has a private LDS slice and synchronises
// with itself only).  Lane = (row, m): row = lane>>2
// is a pixel row of the MCU, m = lane&3 the MCU of the quad, so one lane streams a 16-pixel row segment
// of each plane as a single 16-byte access (4 lanes = 64 contiguous bytes) and the 3 KB of coefficients
// of a quad move as 3 coalesced 1 KB wave accesses.  The two separable 1-D passes run in registers (one
// 8-point transform per lane-row/column, 2 independent transforms per lane for ILP) with a padded,
// bank-conflict-free LDS transpose between them.  No MFMA: FP64 8x8 is VALU work.
//
// Exactness (DESIGN.md "exactness"): the reference truncates FP64 results, so the output depends on the
// exact rounding sequence only where the true value sits on a quantiser boundary.  The fast
// separable transform (FMA allowed, error < 1e-9) is accepted when the fixed-point value is >= 2 units
// of 2^-24 away from every boundary; otherwise the coefficient is re-evaluated by
// exact_fdct_coef_wave() in the reference's exact operation order (plain IEEE mul/add, no contraction).  DC terms are
// sums of integers and are always evaluated exactly.  Colour conversion is evaluated in the reference's
// exact FP64 order everywhere.  This file must be compiled with -ffp-contract=off; every fused
// multiply-add below is an explicit __builtin_fma in a fast-path estimate.
#include "jpezy_wave.h"
#include "../../include/jpezy_constants.h"

namespace jpezy_dev {

// (static: jpezy_kernels_decode.hip has tables of the same names)
static __constant__ double c_cos[64] = JPEZY_COS_INIT;            // [u*8+x] = cos((2x+1)u*pi/16)
static __constant__ unsigned char c_zzinv[64] = JPEZY_ZZ_INV_INIT;  // natural index -> zig-zag position

#define JPEZY_S JPEZY_INV_SQRT2

// cos(k*pi/16) -- the same correctly rounded doubles as the cos table rows (fast path only)
#define C1 0x1.f6297cff75cb0p-1
#define C2 0x1.d906bcf328d46p-1
#define C3 0x1.a9b66290ea1a3p-1
#define C4 0x1.6a09e667f3bcdp-1
#define C5 0x1.1c73b39ae68c8p-1
#define C6 0x1.87de2a6aea963p-2
#define C7 0x1.8f8b83c69a60bp-3

#define FMA(a, b, c) __builtin_fma((a), (b), (c))

// LDS geometry (dwords), chosen so that the column reads (ds_read_b64, 32-lane groups, 64 banks) are
// conflict free: per-MCU stride == 16 (mod 64) dwords.  Row pitch 36 dwords keeps 16-byte alignment and
// limits the ds_write_b128 conflicts to 2-way.
constexpr int Y_PITCH = 36;                 // 16 doubles + 2 pad
constexpr int Y_MCU = 16 * Y_PITCH + 16;    // 592
constexpr int C_PITCH = 20;                 // 8 doubles + 2 pad
constexpr int C_COMP = 8 * C_PITCH;         // 160
constexpr int C_MCU = 2 * C_COMP + 16;      // 336
constexpr int TILE_DWORDS = 4 * Y_MCU;      // 2368 dwords = 9472 B: transpose tiles / staging
// Behind the tiles: the wave's queue of guard-band hits (count + entries), never overlapped by a tile.
constexpr int QUEUE_CAP = 126;
constexpr int WAVE_LDS_DWORDS = TILE_DWORDS + 64;   // 9728 B per wave, 19456 B per workgroup of two

// X[u] = sum_x x[x] * cos((2x+1)u*pi/16), u = 0..7 ; X[0] is the plain (exact, for integers) sum.
__device__ __forceinline__ void fdct8(const double* x, double* X)
{
    const double s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
    const double d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
    const double e0 = s0 + s3, e1 = s1 + s2, e2 = s0 - s3, e3 = s1 - s2;
    X[0] = e0 + e1;
    X[4] = (e0 - e1) * C4;
    X[2] = FMA(e3, C6, e2 * C2);
    X[6] = FMA(-e3, C2, e2 * C6);
    X[1] = FMA(d3, C7, FMA(d2, C5, FMA(d1, C3, d0 * C1)));
    X[3] = FMA(-d3, C5, FMA(-d2, C1, FMA(-d1, C7, d0 * C3)));
    X[5] = FMA(d3, C3, FMA(d2, C7, FMA(-d1, C1, d0 * C5)));
    X[7] = FMA(-d3, C1, FMA(d2, C3, FMA(-d1, C5, d0 * C7)));
}

// ---- colour conversion in the reference's exact order (ref jpezy_encoder.hpp:244-256) ----
__device__ __forceinline__ double ref_y(double r, double g, double b)
{
    return __builtin_trunc((0.2990 * r) + (0.5870 * g) + (0.1140 * b) - 128.0);
}
__device__ __forceinline__ double ref_cb(double r, double g, double b)
{
    return __builtin_trunc(-(0.1687 * r) - (0.3313 * g) + (0.5000 * b));
}
__device__ __forceinline__ double ref_cr(double r, double g, double b)
{
    return __builtin_trunc((0.5000 * r) - (0.4187 * g) - (0.0813 * b));
}

// In-order sum of one double per lane, lane 0 first: sum = (((0 + t0) + t1) + ...) + t63, every add
// rounded -- the reference's accumulation order.  Wave-uniform result.
__device__ __forceinline__ double ordered_wave_sum(double t)
{
    const int lo = (int)(unsigned)(__builtin_bit_cast(unsigned long long, t) & 0xFFFFFFFFull);
    const int hi = (int)(unsigned)(__builtin_bit_cast(unsigned long long, t) >> 32);
    double sum = 0;
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const unsigned long long bits = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, k) << 32) |
                                        (unsigned)__builtin_amdgcn_readlane(lo, k);
        sum += __builtin_bit_cast(double, bits);
    }
    return sum;
}

struct BlockRef {   // the frame's planes: what the exact path needs to find a block again
    const uint8_t* r;
    const uint8_t* g;
    const uint8_t* b;
    int W, H;
    unsigned row_stride, pix_bytes;     // packed pixels only (PACKED instances): bytes between rows / between pixels of one channel
    unsigned c_row_stride, c_step;      // YCC instances: r, g, b = the Y, Cb, Cr samples (0, 0) of the frame; Y rows row_stride apart,
};                                      // chroma rows c_row_stride and chroma samples c_step apart

// ---- exact-order FDCT + quantise of ONE coefficient by the whole wave (ref jpezy_encoder.hpp:146-172) ----
// All arguments are wave-uniform.  Lane k owns term k = y*8+x of the reference's double loop: it re-reads its
// pixel, converts it, forms (pic*cos[j][x])*cos[i][y]; the 64 terms are then added in the reference's order.
// comp 0: luma block with top-left pixel (px0,py0), step 1.  comp 1/2: Cb/Cr of the MCU at (px0,py0), step 2
// (top-left sample of each 2x2, ref :134-142).  Coordinates clamp to the image (ref :101,104).
// YCC: the planes hold the samples themselves (jpezy_fdct_quant_ycc_dev): pic = byte - 128 of luma sample (px0 + x, py0 + y) or of
// chroma sample (px0 / 2 + x, py0 / 2 + y), clamped to the plane (W x H, ceil(W/2) x ceil(H/2)).
template <bool PACKED = false, bool YCC = false>
__device__ __forceinline__ int exact_fdct_coef_wave(const BlockRef& img, int px0, int py0, int comp, int i, int j,
                                                    int Q, int lane)
{
    const int step = comp ? 2 : 1;
    const int y = lane >> 3, x = lane & 7;
    double pic;
    if constexpr (YCC) {
        if (comp == 0) {
            const int yy = min(py0 + y, img.H - 1), xx = min(px0 + x, img.W - 1);
            pic = (double)((int)img.r[(size_t)yy * img.row_stride + xx] - 128);
        } else {
            const int yy = min((py0 >> 1) + y, ((img.H + 1) >> 1) - 1), xx = min((px0 >> 1) + x, ((img.W + 1) >> 1) - 1);
            pic = (double)((int)(comp == 1 ? img.g : img.b)[(size_t)yy * img.c_row_stride + (size_t)xx * img.c_step] - 128);
        }
    } else {
        const int yy = min(py0 + y * step, img.H - 1);
        const int xx = min(px0 + x * step, img.W - 1);
        const size_t idx = PACKED ? (size_t)yy * img.row_stride + (size_t)xx * img.pix_bytes : (size_t)yy * img.W + xx;
        const double rf = (double)img.r[idx], gf = (double)img.g[idx], bf = (double)img.b[idx];
        pic = comp == 0 ? ref_y(rf, gf, bf) : comp == 1 ? ref_cb(rf, gf, bf) : ref_cr(rf, gf, bf);
    }
    const double sum = ordered_wave_sum(pic * c_cos[j * 8 + x] * c_cos[i * 8 + y]);
    const double cu = j ? 1.0 : JPEZY_S, cv = i ? 1.0 : JPEZY_S;
    const int dct = (int)(sum * cu * cv / 4);
    return dct / Q;
}

// Quantise the 8 coefficients F[i] (vertical frequency i, this lane's horizontal frequency j).
// ks[i] = cu*cv/(4Q) * 2^bits.  n[i] = trunc(v/Q * 2^bits); q[i] = trunc-toward-zero(n / 2^bits).
// bits = DeviceTables::qfrac_bits, chosen by the host from the tables so that |n| <= 2^30 (jpezy_device.h): 24 with the Annex-K tables,
// 20 when a table holds a 1.  Returns true when some coefficient lies within 1 unit of a multiple of 2^bits (candidate for the exact
// path).  Why one unit is enough at every width: n is off from trunc(t * 2^bits) of the reference's own t = v/Q by at most one unit as
// long as the two values of t differ by less than 2^-bits.  They differ by the rounding of the FP64 butterflies against the reference's
// 64-term FP64 sum and of ks -- below 200 roundings of 2^-53 on |v| <= 1024, i.e. 3e-11 in v and no more in t (Q >= 1) -- against a
// unit of 2^-24 = 6e-8 at the widest width (a factor of 2000) and of 2^-20 = 9.5e-7 at the narrowest (a factor of 30000).
__device__ __forceinline__ bool quant8(const double* F, const double* ks, bool dc_lane, double rq_dc, int bits, int* n, int* q)
{
    const int MASK = (1 << bits) - 1;
    unsigned m[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        n[i] = (int)(F[i] * ks[i]);                          // v_cvt_i32_f64 truncates toward zero
        q[i] = (n[i] + ((n[i] >> 31) & MASK)) >> bits;       // trunc-toward-zero division by 2^bits
        m[i] = (unsigned)(n[i] + 1) & MASK;                  // 0,1,2 <=> within one unit of a boundary
    }
    // DC: F[0] of the j == 0 lane is the exact integer sum of the block, so the reference value
    // int(sum*S*S/4) is reproduced bit for bit; (|iv|+0.5)/Q is never within 0.5/Q of an integer.
    {
        const double iv = __builtin_trunc(F[0] * JPEZY_S * JPEZY_S / 4);
        int nq = (int)((__builtin_fabs(iv) + 0.5) * rq_dc);
        nq = iv < 0 ? -nq : nq;
        if (dc_lane) {
            q[0] = nq;
            m[0] = MASK;
        }
    }
    const unsigned a = min(min(m[0], m[1]), m[2]), b = min(min(m[3], m[4]), m[5]), c = min(m[6], m[7]);
    return min(min(a, b), c) <= 2u;
}

// byte offsets of the staging area: blocks padded to 144 B so that the 8 blocks written by one
// ds_write_b16 wave-instruction fall on different banks
constexpr int STG_BLK = 144;

// Quantise one block column, write it (zig-zag) to the staging area and queue the guard-band hits.
// blk = index of the block inside the quad (m*BPM + b).  Queue entry = blk << 6 | natural index.
__device__ __forceinline__ void quant_block_column(const double* F, const double* ks, int j, double rq_dc, int bits,
                                                   bool live, const int* zoff, char* stage_blk, int blk,
                                                   unsigned* queue)
{
    const int MASK = (1 << bits) - 1;
    int n[8], q[8];
    const bool cand = quant8(F, ks, j == 0, rq_dc, bits, n, q);
    if (cand && live) {   // rare.  Fully unrolled: a runtime index into n[] would send the array to scratch
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            // within one unit of a multiple of 2^bits -- except around 0, which is not a truncation boundary;
            // the DC term of the j == 0 lane is already exact
            const bool f = ((unsigned)(n[i] + 1) & MASK) <= 2u && (unsigned)(n[i] + 1) > 2u && !(i == 0 && j == 0);
            if (f) {
                const unsigned slot = atomicAdd(&queue[0], 1u);
                if (slot < (unsigned)QUEUE_CAP)
                    reinterpret_cast<unsigned short*>(queue + 1)[slot] = (unsigned short)((blk << 6) | (i * 8 + j));
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) *reinterpret_cast<int16_t*>(stage_blk + zoff[i]) = (int16_t)q[i];
}

__device__ __forceinline__ double byte_of(const uint32_t* w, int k)
{
    return (double)((w[k >> 2] >> ((k & 3) * 8)) & 0xFFu);
}

// ======================================================================================================
// ENCODE
// ======================================================================================================
// PACKED (jpezy_fdct_quant_packed_dev): r, g, b are the channel bytes of pixel (0, 0) of an interleaved buffer, p.pix_bytes between
// pixels and p.row_stride between rows; such input takes the byte loop (ALIGNED is never set with it)
// YCC (jpezy_fdct_quant_ycc_dev): r = the Y plane, g / b = the Cb / Cr samples; the byte loop fetches the lane's 16 Y samples and the 8
// samples of its chroma row (Cb on even-row lanes, Cr on odd-row lanes), and the two conversions become byte - 128
template <bool GRAY, bool ALIGNED, bool FORCE_EXACT, bool PACKED = false, bool YCC = false>
__global__ __launch_bounds__(64 * WPB, 4) void fdct_quant_kernel(EncParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[WPB][WAVE_LDS_DWORDS];
    constexpr int BPM = GRAY ? 4 : 6;
    constexpr int STG_BASE = 4 * C_MCU * 4;                   // bytes: staging sits behind the chroma tile
    static_assert(STG_BASE + 4 * 6 * STG_BLK <= TILE_DWORDS * 4, "staging does not fit the tile area");

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;   // WPB waves per workgroup
    const long quad = (long)blockIdx.x * WPB + wave;
    const long quads_per_frame = (long)p.mcu_rows * p.quads_per_row;
    if (quad >= quads_per_frame * p.n_frames) return;   // wave-uniform
    const int frame = (int)(quad / quads_per_frame);
    const int qrem = (int)(quad - (long)frame * quads_per_frame);
    const int mcu_y = qrem / p.quads_per_row;
    const int quad_x = qrem - mcu_y * p.quads_per_row;

    uint32_t* lds = lds_all[wave];
    unsigned* queue = lds + TILE_DWORDS;                        // [0] = count, then 16-bit entries
    if (lane == 0) queue[0] = 0;
    const int row = lane >> 2, m = lane & 3;
    const int mcu_x_raw = quad_x * 4 + m;
    const bool live = mcu_x_raw < p.mcu_cols;
    const int mcu_x = live ? mcu_x_raw : p.mcu_cols - 1;
    const int W = p.W, H = p.H;
    const uint8_t* pr = p.r + (size_t)frame * p.plane_stride;
    const uint8_t* pg = p.g + (size_t)frame * (YCC ? p.c_frame_stride : p.plane_stride);
    const uint8_t* pb = p.b + (size_t)frame * (YCC ? p.c_frame_stride : p.plane_stride);
    const BlockRef img = { pr, pg, pb, W, H, PACKED || YCC ? p.row_stride : 0u, PACKED ? (unsigned)p.pix_bytes : 0u,
                           YCC ? p.c_row_stride : 0u, YCC ? (unsigned)p.c_step : 0u };

    // ---- 1. stream this lane's 16-pixel row segment of the three planes ----
    uint32_t R[4], G[4], B[4];
    if constexpr (YCC) {
        const int y = min(mcu_y * 16 + row, H - 1), cy = min(mcu_y * 8 + (row >> 1), ((H + 1) >> 1) - 1), CW = (W + 1) >> 1;
        const uint8_t* py = pr + (size_t)y * p.row_stride;
        const uint8_t* pc = ((row & 1) ? pb : pg) + (size_t)cy * p.c_row_stride;
#pragma unroll
        for (int w4 = 0; w4 < 4; ++w4) {
            uint32_t ay = 0, ac = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ay |= (uint32_t)py[min(mcu_x * 16 + w4 * 4 + k, W - 1)] << (8 * k);
                if (!GRAY && w4 < 2) ac |= (uint32_t)pc[(size_t)min(mcu_x * 8 + w4 * 4 + k, CW - 1) * (size_t)p.c_step] << (8 * k);
            }
            R[w4] = ay; G[w4] = ac; B[w4] = 0;
        }
    } else {
        const int y = min(mcu_y * 16 + row, H - 1);             // edge replication, ref :101
        const size_t rowoff = PACKED ? (size_t)y * p.row_stride : (size_t)y * W;
        if (ALIGNED) {
            const size_t off = rowoff + (size_t)mcu_x * 16;
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
                    const int x = min(mcu_x * 16 + w4 * 4 + k, W - 1) * (PACKED ? p.pix_bytes : 1);   // ref :104
                    ar |= (uint32_t)pr[rowoff + x] << (8 * k);
                    ag |= (uint32_t)pg[rowoff + x] << (8 * k);
                    ab |= (uint32_t)pb[rowoff + x] << (8 * k);
                }
                R[w4] = ar; G[w4] = ag; B[w4] = ab;
            }
        }
    }

    // ---- 2. luma of the 16 pixels, row pass of the left / right block, into the transpose tile ----
    {
        double yv[16], X[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) yv[k] = YCC ? byte_of(R, k) - 128.0 : ref_y(byte_of(R, k), byte_of(G, k), byte_of(B, k));
        fdct8(yv, X);
        fdct8(yv + 8, X + 8);
        double2* dst = reinterpret_cast<double2*>(lds + m * Y_MCU + row * Y_PITCH);
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k] = make_double2(X[2 * k], X[2 * k + 1]);
    }
    wave_sync();

    // ---- 3. luma column pass: lane (cq, m) owns column cq of the 16x16 tile = column j of two blocks ----
    const int cq = row;                 // 0..15
    const int j = cq & 7;
    const DeviceTables* tab = p.tab;
    const int qbits = tab->qfrac_bits;  // wave-uniform: one scalar load
    char* stage = reinterpret_cast<char*>(lds) + STG_BASE;
    int zoff[8];                        // byte offset of natural coefficient (i, j) inside a staged block
#pragma unroll
    for (int i = 0; i < 8; ++i) zoff[i] = 2 * (int)c_zzinv[i * 8 + j];
    {
        double Ftop[8], Fbot[8];
        {
            double col[16];
            const uint32_t* src = lds + m * Y_MCU + cq * 2;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) col[rr] = *reinterpret_cast<const double*>(src + rr * Y_PITCH);
            fdct8(col, Ftop);
            fdct8(col + 8, Fbot);
        }
        wave_sync();   // every lane has read the luma tile: the slice is reused from here on

        // ---- 4. quantise + zig-zag the two luma block columns into the staging area ----
        double ks[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ks[i] = tab->qscale[0][j][i];
        const double rq = tab->rq_dc[0];
        const int bx = cq >> 3;   // 0: left blocks (Y0,Y2), 1: right blocks (Y1,Y3)
        quant_block_column(Ftop, ks, j, rq, qbits, live, zoff, stage + (m * BPM + bx) * STG_BLK, m * BPM + bx, queue);
        quant_block_column(Fbot, ks, j, rq, qbits, live, zoff, stage + (m * BPM + 2 + bx) * STG_BLK, m * BPM + 2 + bx, queue);
    }

    // ---- 5. chroma: top-left pixel of every 2x2 (ref :134-142) = even pixel rows, even columns.  The odd-row
    //         lane fetches its even neighbour's pixels (DPP row_shr:4) and computes Cr while the even-row lane
    //         computes Cb, so all 64 lanes carry one chroma row each. ----
    if (!GRAY) {
        const bool odd = (row & 1) != 0;
        uint32_t R2[4], G2[4], B2[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // row_shr:4 within each 16-lane DPP row, written only to lanes 4-7 and 12-15 (bank_mask 0b1010)
            R2[k] = (uint32_t)__builtin_amdgcn_update_dpp((int)R[k], (int)R[k], 0x114, 0xF, 0xA, false);
            G2[k] = (uint32_t)__builtin_amdgcn_update_dpp((int)G[k], (int)G[k], 0x114, 0xF, 0xA, false);
            B2[k] = (uint32_t)__builtin_amdgcn_update_dpp((int)B[k], (int)B[k], 0x114, 0xF, 0xA, false);
        }
        // Cb = (-(0.1687 r) - 0.3313 g) + 0.5 b ; Cr = (0.5 r - 0.4187 g) - 0.0813 b  (ref :249-256), both as
        // trunc((k1*r - k2*g) + k3*b): (-a)*r == -(a*r) and x - y == x + (-y) hold bit for bit in IEEE-754.
        const double k1 = odd ? 0.5000 : -0.1687, k2 = odd ? 0.4187 : 0.3313, k3 = odd ? -0.0813 : 0.5000;
        double cv[8], cX[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            cv[k] = YCC ? byte_of(G, k) - 128.0 : __builtin_trunc((k1 * byte_of(R2, 2 * k) - k2 * byte_of(G2, 2 * k)) + k3 * byte_of(B2, 2 * k));
        fdct8(cv, cX);
        double2* dst = reinterpret_cast<double2*>(lds + m * C_MCU + (odd ? C_COMP : 0) + (row >> 1) * C_PITCH);
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = make_double2(cX[2 * k], cX[2 * k + 1]);
        wave_sync();

        double Fc[8];
        {
            double col[8];
            const uint32_t* src = lds + m * C_MCU + (cq >> 3) * C_COMP + j * 2;
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) col[rr] = *reinterpret_cast<const double*>(src + rr * C_PITCH);
            fdct8(col, Fc);
        }
        double ks[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ks[i] = tab->qscale[1][j][i];
        const int comp = 1 + (cq >> 3);
        quant_block_column(Fc, ks, j, tab->rq_dc[1], qbits, live, zoff, stage + (m * BPM + 3 + comp) * STG_BLK,
                           m * BPM + 3 + comp, queue);
    }
    wave_sync();

    // ---- 5b. guard-band hits: re-evaluate in the reference's exact operation order, one coefficient at a
    //          time, all 64 lanes cooperating (rare: ~0.7 % of blocks on random pixels).  FORCE_EXACT (test
    //          hook) and a queue overflow send EVERY coefficient of the quad through this path. ----
    {
        const unsigned nq = queue[0];
        const bool all = FORCE_EXACT || nq > (unsigned)QUEUE_CAP;
        const unsigned total = all ? (unsigned)(4 * BPM * 64) : nq;
        if (total) {
            const int valid_mcus = min(4, p.mcu_cols - quad_x * 4);
            unsigned done = 0;
#pragma unroll 1
            for (unsigned e = 0; e < total; ++e) {
                const unsigned code = all ? e : reinterpret_cast<const unsigned short*>(queue + 1)[e];
                const int blk = __builtin_amdgcn_readfirstlane((int)(code >> 6)), nat = __builtin_amdgcn_readfirstlane((int)(code & 63));
                const int em = blk / BPM, eb = blk - em * BPM;
                if (em >= valid_mcus) continue;
                const int ei = nat >> 3, ej = nat & 7;
                const int emx = quad_x * 4 + em;
                int px0 = emx * 16, py0 = mcu_y * 16, comp = 0;
                if (eb < 4) { px0 += (eb & 1) * 8; py0 += (eb >> 1) * 8; } else { comp = eb - 3; }
                const int Q = tab->qt[comp ? 1 : 0][nat];
                const int qv = exact_fdct_coef_wave<PACKED, YCC>(img, px0, py0, comp, ei, ej, Q, lane);
                if (lane == 0) *reinterpret_cast<int16_t*>(stage + blk * STG_BLK + 2 * (int)c_zzinv[nat]) = (int16_t)qv;
                ++done;
            }
            if (lane == 0 && done) atomicAdd(p.fallback_count + ((blockIdx.x * (unsigned)WPB + wave) & (COUNTER_SHARDS - 1)), (unsigned long long)done);
            wave_sync();
        }
    }

    // ---- 6. coalesced store of the quad's coefficients (BPM*128 bytes per MCU, contiguous) ----
    {
        const int valid_mcus = min(4, p.mcu_cols - quad_x * 4);
        const int valid_chunks = valid_mcus * BPM * 8;         // 16-byte chunks
        int16_t* gbase = p.coeffs + (size_t)frame * p.coeffs_per_frame +
                         ((size_t)mcu_y * p.mcu_cols + (size_t)quad_x * 4) * (BPM * 64);
        uint4* g4 = reinterpret_cast<uint4*>(gbase);
#pragma unroll
        for (int k = 0; k < BPM * 128 * 4 / 1024; ++k) {
            const int c = k * 64 + lane;
            if (c < valid_chunks) nt_store16(g4 + c, *reinterpret_cast<const uint4*>(stage + (c >> 3) * STG_BLK + (c & 7) * 16));
        }
    }
}

// ======================================================================================================
// launchers
// ======================================================================================================
template <bool GRAY, bool ALIGNED>
static void enc_launch2(const EncParams& p, bool force, dim3 grid, hipStream_t s)
{
    if (force)
        hipLaunchKernelGGL((fdct_quant_kernel<GRAY, ALIGNED, true>), grid, dim3(64 * WPB), 0, s, p);
    else
        hipLaunchKernelGGL((fdct_quant_kernel<GRAY, ALIGNED, false>), grid, dim3(64 * WPB), 0, s, p);
}

hipError_t launch_fdct_quant(const EncParams& p, bool gray, bool force_exact, hipStream_t stream)
{
    const long quads = (long)p.n_frames * p.mcu_rows * p.quads_per_row;
    if (quads <= 0) return hipSuccess;
    const dim3 grid((unsigned)((quads + WPB - 1) / WPB));
    const bool al = is_aligned16(p, p.r, p.g, p.b);
    if (gray) { if (al) enc_launch2<true, true>(p, force_exact, grid, stream); else enc_launch2<true, false>(p, force_exact, grid, stream); }
    else      { if (al) enc_launch2<false, true>(p, force_exact, grid, stream); else enc_launch2<false, false>(p, force_exact, grid, stream); }
    return hipGetLastError();
}

hipError_t launch_fdct_quant_packed(const EncParams& p, bool gray, bool force_exact, hipStream_t stream)
{
    const long quads = (long)p.n_frames * p.mcu_rows * p.quads_per_row;
    if (quads <= 0) return hipSuccess;
    const dim3 grid((unsigned)((quads + WPB - 1) / WPB));
    if (gray) {
        if (force_exact) hipLaunchKernelGGL((fdct_quant_kernel<true, false, true, true>), grid, dim3(64 * WPB), 0, stream, p);
        else hipLaunchKernelGGL((fdct_quant_kernel<true, false, false, true>), grid, dim3(64 * WPB), 0, stream, p);
    } else {
        if (force_exact) hipLaunchKernelGGL((fdct_quant_kernel<false, false, true, true>), grid, dim3(64 * WPB), 0, stream, p);
        else hipLaunchKernelGGL((fdct_quant_kernel<false, false, false, true>), grid, dim3(64 * WPB), 0, stream, p);
    }
    return hipGetLastError();
}

hipError_t launch_fdct_quant_ycc(const EncParams& p, bool gray, bool force_exact, hipStream_t stream)
{
    const long quads = (long)p.n_frames * p.mcu_rows * p.quads_per_row;
    if (quads <= 0) return hipSuccess;
    const dim3 grid((unsigned)((quads + WPB - 1) / WPB));
    if (gray) {
        if (force_exact) hipLaunchKernelGGL((fdct_quant_kernel<true, false, true, false, true>), grid, dim3(64 * WPB), 0, stream, p);
        else hipLaunchKernelGGL((fdct_quant_kernel<true, false, false, false, true>), grid, dim3(64 * WPB), 0, stream, p);
    } else {
        if (force_exact) hipLaunchKernelGGL((fdct_quant_kernel<false, false, true, false, true>), grid, dim3(64 * WPB), 0, stream, p);
        else hipLaunchKernelGGL((fdct_quant_kernel<false, false, false, false, true>), grid, dim3(64 * WPB), 0, stream, p);
    }
    return hipGetLastError();
}

}  // namespace jpezy_dev
