// jpezy_kernels_generic.hip -- decode for ANY baseline layout the reference's decoder accepts (1 or 3 components,
// sampling factors 1..4).  Blocks are independent 8x8 inverse transforms whatever the layout:
//   generic_idct_kernel : one wavefront per EIGHT consecutive blocks, lane = (block, column).  Fast path as in the fused
//                         kernel of jpezy_kernels_decode.hip: FP64 separable butterflies (column pass, transpose through LDS, row
//                         pass), sample = int(v) with a guard band of 2^-18 around every integer, DC-only blocks exact by
//                         construction.  A block with a sample inside the band (5e-4 of the blocks), with a coefficient
//                         above the magnitude guard, or under the force_exact test hook is recomputed by all 64 lanes in
//                         the reference's own order: lane (y, x) accumulates the 64 terms
//                         ((cu*cv) * (coef*Q)) * cos[u][x] * cos[v][y], v outer, u inner, and stores int(sum/4 + sl),
//                         sl = 128 (2048 if precision != 8)                 (ref decoder/jpezy_decoder.hpp:645-670)
//   generic_rgb_kernel  : one lane per pixel; block placement of each component exactly as decode_mcu does it (ref
//                         :504-528), then make_rgb / revise_value in the reference's FP64 order (ref :531-578, 672-676);
//                         its instance generic_yuv422_kernel writes packed YCbCr 4:2:2 macropixels instead, without make_rgb
// The fused kernel covers jpezy_encode's own 2x2,1x1,1x1 layout in one pass; this pair exists so that every file the
// reference decodes also decodes here, at about a third of the fused kernel's speed.
#include "jpezy_pixel_out.h"
#include "../../include/jpezy_constants.h"

namespace jpezy_dev {
namespace generic {

__constant__ double c_cos[64] = JPEZY_COS_INIT;
__constant__ unsigned char c_zzinv[64] = JPEZY_ZZ_INV_INIT;
#define JPEZY_S JPEZY_INV_SQRT2
#define GFMA(a, b, c) __builtin_fma((a), (b), (c))

// x[y] = sum_v X[v] * cos((2y+1)v*pi/16)   (X[0] already carries its 1/sqrt2); an estimate: FMAs allowed
__device__ __forceinline__ void idct8_est(const double* X, double* x)
{
    const double C1 = 0.98078528040323044913, C2 = 0.92387953251128675613, C3 = 0.83146961230254523708, C4 = 0.70710678118654752440,
                 C5 = 0.55557023301960222474, C6 = 0.38268343236508977173, C7 = 0.19509032201612826785;
    const double t0 = GFMA(X[4], C4, X[0]), t1 = GFMA(-X[4], C4, X[0]);
    const double t2 = GFMA(X[6], C6, X[2] * C2), t3 = GFMA(-X[6], C2, X[2] * C6);
    const double E0 = t0 + t2, E3 = t0 - t2, E1 = t1 + t3, E2 = t1 - t3;
    const double O0 = GFMA(X[7], C7, GFMA(X[5], C5, GFMA(X[3], C3, X[1] * C1)));
    const double O1 = GFMA(-X[7], C5, GFMA(-X[5], C1, GFMA(-X[3], C7, X[1] * C3)));
    const double O2 = GFMA(X[7], C3, GFMA(X[5], C7, GFMA(-X[3], C1, X[1] * C5)));
    const double O3 = GFMA(-X[7], C1, GFMA(X[5], C3, GFMA(-X[3], C5, X[1] * C7)));
    x[0] = E0 + O0; x[7] = E0 - O0;
    x[1] = E1 + O1; x[6] = E1 - O1;
    x[2] = E2 + O2; x[5] = E2 - O2;
    x[3] = E3 + O3; x[4] = E3 - O3;
}

constexpr int G_BLOCKS = 8;                 // blocks per wavefront
constexpr int G_STG = 72;                   // int16 elements between staged blocks (144 bytes: the eight blocks' zig-zag reads spread over the banks)
constexpr int G_PITCH = 18;                 // dwords per transposed row: 8 doubles + 1 pad
constexpr int G_TILE = 8 * G_PITCH + 2;     // dwords per block of the transpose tile
constexpr float G_EPS = 0x1p-18f;

__global__ __launch_bounds__(64) void generic_idct_kernel(GenericDecParams p, long nblk)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[G_BLOCKS * G_TILE];     // 1168 dwords; the coefficient staging (576 B.. 1152 B) shares it
    __shared__ int dct[64];
    const int lane = threadIdx.x, b = lane >> 3, u = lane & 7;
    const long g0 = (long)blockIdx.x * G_BLOCKS, g = g0 + b;
    const bool live = g < nblk;

    // ---- coefficients of the eight blocks: 1 KB contiguous -> LDS ----
    {
        const uint4* src = reinterpret_cast<const uint4*>(p.coeffs + g0 * 64);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (g0 + (lane >> 3) < nblk) v = src[lane];                              // lane: block lane>>3, 16-byte piece lane&7
        *reinterpret_cast<uint4*>(reinterpret_cast<char*>(lds) + (lane >> 3) * (G_STG * 2) + (lane & 7) * 16) = v;
    }
    wave_sync();
    const int k = live ? (int)(g % p.blocks_per_mcu) : 0;
    int comp = 0;
    if (k >= p.blk_start[1]) comp = 1;
    if (k >= p.blk_start[2]) comp = 2;

    // ---- column pass for column u of block b ----
    double col[8];
    int amax = 0, acor = 0;
    {
        const int16_t* blk = reinterpret_cast<const int16_t*>(lds) + b * G_STG;
        double in[8];
        int c[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            c[v] = blk[c_zzinv[v * 8 + u]];
            in[v] = (double)c[v] * p.dqscale[(comp * 8 + u) * 8 + v];
            amax = max(amax, max(c[v], -c[v]));
        }
        // the DC term in the reference's own order, so that a block with no other coefficient comes out exact
        if (u == 0) in[0] = (JPEZY_S * JPEZY_S) * (double)(c[0] * p.qt[comp * 64]) * 0.25;
        acor = (u ? c[0] : 0) | c[1] | c[2] | c[3] | c[4] | c[5] | c[6] | c[7];
        idct8_est(in, col);
    }
    const unsigned long long ac_any = __ballot(acor != 0);
    const bool dc_only = ((ac_any >> (8 * b)) & 0xFFull) == 0;
    const unsigned long long big = __ballot(amax > p.coef_limit);
    wave_sync();                                                                 // staging consumed: the tile overwrites it

    // ---- transpose, row pass ----
#pragma unroll
    for (int y = 0; y < 8; ++y) *reinterpret_cast<double*>(lds + b * G_TILE + y * G_PITCH + u * 2) = col[y];
    wave_sync();
    int smp[8];
    bool flagged = false;
    {
        const int y = u;                                                         // this lane now owns row y of block b
        double in[8], out[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) in[q] = *reinterpret_cast<const double*>(lds + b * G_TILE + y * G_PITCH + q * 2);
        in[0] += (double)p.level;
        idct8_est(in, out);
        float em = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            smp[q] = (int)out[q];
            em = __builtin_fmaxf(em, __builtin_fabsf((float)__builtin_amdgcn_fract(out[q]) - 0.5f));
        }
        flagged = !dc_only && em > 0.5f - G_EPS;
    }
    // blocks that go to the reference-order path: any sample in the band, any coefficient above the magnitude guard
    unsigned long long fl = __ballot(flagged) | big;
    unsigned need = 0;
#pragma unroll
    for (int q = 0; q < G_BLOCKS; ++q) need |= ((fl >> (8 * q)) & 0xFFull) ? (1u << q) : 0u;
    if (p.force_exact) need = 0xFFu;
    if (live && !((need >> b) & 1u)) {
        int4* dst = reinterpret_cast<int4*>(p.samples + g * 64 + u * 8);
        dst[0] = make_int4(smp[0], smp[1], smp[2], smp[3]);
        dst[1] = make_int4(smp[4], smp[5], smp[6], smp[7]);
    }
    // ---- reference order, one block at a time, lane = sample (y, x) ----
    unsigned done = 0;
    while (need) {
        const int q = __builtin_ctz(need);
        need &= need - 1;
        const long gq = g0 + q;
        if (gq >= nblk) continue;
        const int kq = (int)(gq % p.blocks_per_mcu);
        int cq = 0;
        if (kq >= p.blk_start[1]) cq = 1;
        if (kq >= p.blk_start[2]) cq = 2;
        wave_sync();
        // natural index `lane`: coefficient at zig-zag position zzinv[lane], times its quantiser (ref :645-650)
        dct[lane] = (int)p.coeffs[gq * 64 + c_zzinv[lane]] * p.qt[cq * 64 + lane];
        wave_sync();
        const int y = lane >> 3, x = lane & 7;
        double sum = 0;
        for (int v = 0; v < 8; ++v) {
            const double cv = (!v) ? JPEZY_S : 1.0;
            for (int uu = 0; uu < 8; ++uu) {
                const double cu = (!uu) ? JPEZY_S : 1.0;
                sum += cu * cv * dct[v * 8 + uu] * c_cos[uu * 8 + x] * c_cos[v * 8 + y];
            }
        }
        p.samples[gq * 64 + lane] = ref_int(sum / 4 + p.level);
        done += 64;
    }
    if (done && lane == 0) atomicAdd(p.fallback_count + (blockIdx.x & (COUNTER_SHARDS - 1)), (unsigned long long)done);
}

// One thread: four consecutive pixels of a row (one 4-byte store per plane when the row allows it); a workgroup: 256 pixels
// of four rows.  Everything that depends on the row only (MCU row, the component's block row, whether decode_mcu ever
// writes that row of the component's plane) is computed once per thread.
// The second stages share that thread: the per-layout sample fetch -- smp[c][j], the integer sample of component c that the
// nearest-neighbour decode feeds make_rgb for pixel (x0 + j, y) -- and behind it the sink's store, chosen at compile time.  (The fetch as
// a __forceinline__ function of its own, called from two kernels, moved the instructions of the three RGB instances -- it is optimised
// once on its own before it is inlined --; as one template the instances 0 / 3 / 4 are the machine code they were.)
// SINK: 0 = planes; 3 / 4 = packed (interleaved) pixels of that many bytes -- the thread's four pixels are 12 or 16 contiguous bytes,
// one 12- or 16-byte store when they start on a 4-byte boundary and all four exist, single bytes otherwise.
// SINK_YUV422: packed YCbCr 4:2:2 macropixels (include/jpezy_hip_ycc422.h) -- the thread's four pixels are two macropixels, 8 contiguous
// bytes.  The Y byte of a pixel is revise_value of its luma sample, the Cb / Cr bytes of a macropixel those of the samples fetched for its
// EVEN pixel (pixels 0 and 2 of the thread); no make_rgb.  p.r, p.g, p.b: the Y0, Cb, Cr bytes of macropixel (0, 0) -- the format is
// their order --, rows p.row_stride, frames p.plane_stride apart.  One 8-byte store when the address is a multiple of 8 and all four
// pixels exist, single bytes otherwise; with an odd W the last macropixel's second Y byte repeats its first.
constexpr int SINK_YUV422 = 2;
template <int SINK = 0>
__global__ __launch_bounds__(256) void generic_rgb_kernel(GenericDecParams p)
{
    const unsigned x0 = (blockIdx.x * 64u + (threadIdx.x & 63u)) * 4u;
    const unsigned y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (y >= (unsigned)p.H || x0 >= (unsigned)p.W) return;
    {   // batch form: blockIdx.z is the frame
        const size_t f = blockIdx.z;
        p.samples += f * ((size_t)p.mcu_cols * p.mcu_rows * p.blocks_per_mcu * 64);
        p.r += f * p.plane_stride; p.g += f * p.plane_stride; p.b += f * p.plane_stride;
    }
    const unsigned mw = (unsigned)p.hmax * 8u, mh = (unsigned)p.vmax * 8u;
    const unsigned uy = fast_div(y, p.mh_magic, p.mh_shift), iy = y - uy * mh;
    // decode_mcu (ref :504-528) writes block (kx, ky) of a component at plane offset (kx*8, ky*8) -- not scaled by the
    // replication factor -- as a rectangle of 8*dupx x 8*dupy samples, ky outer, kx inner; the last write to a position
    // stays.  For H == hmax or H == 1 that is ordinary nearest-neighbour upsampling.  For the other legal factors
    // (H = 2 or 3 under hmax = 3 or 4) later blocks overwrite part of earlier ones and the right/bottom end of the
    // plane is never written: it keeps the initial value of comp[] (0 / 0x80, ref :104-105) in every MCU.
    unsigned rowblk[3], rowsmp[3];
    bool rowok[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned cvv = (unsigned)p.cv[c], dupy = (unsigned)p.vmax / cvv;
        const unsigned ky = min(cvv - 1u, iy >> 3), yu = iy - ky * 8u;                   // last block row written over iy
        rowok[c] = c < p.ncomp && yu < 8u * dupy;
        rowblk[c] = (unsigned)p.blk_start[c] + ky * (unsigned)p.ch[c];
        rowsmp[c] = fast_div(yu, p.dy_magic[c], p.dy_shift[c]) * 8u;
    }
    const unsigned npx = min(4u, (unsigned)p.W - x0);
    int smp[3][4];
    {
        // the four pixels sit in one MCU (x0 is a multiple of 4, MCUs are multiples of 8 wide)
        const unsigned ux = fast_div(x0, p.mw_magic, p.mw_shift), ix0 = x0 - ux * mw;
        const size_t mcu_blk = ((size_t)uy * p.mcu_cols + ux) * (size_t)p.blocks_per_mcu;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int init = c ? 0x80 : 0;                                              // missing components read 0x80 (ref :104-105)
            smp[c][0] = smp[c][1] = smp[c][2] = smp[c][3] = init;
            if (!rowok[c]) continue;
            const unsigned chh = (unsigned)p.ch[c], dupx = (unsigned)p.hmax / chh;
            if (chh == (unsigned)p.hmax) {              // one sample per pixel: four neighbours of one block row, one 16-byte load
                const int4 v = *reinterpret_cast<const int4*>(p.samples + (mcu_blk + rowblk[c] + (ix0 >> 3)) * 64 + rowsmp[c] + (ix0 & 7u));
                smp[c][0] = v.x; smp[c][1] = v.y; smp[c][2] = v.z; smp[c][3] = v.w;
            } else if (chh == 1u && dupx == 2u) {       // every sample twice
                const int2 v = *reinterpret_cast<const int2*>(p.samples + (mcu_blk + rowblk[c]) * 64 + rowsmp[c] + (ix0 >> 1));
                smp[c][0] = smp[c][1] = v.x; smp[c][2] = smp[c][3] = v.y;
            } else if (chh == 1u && dupx == 4u) {       // one sample for all four
                smp[c][0] = smp[c][1] = smp[c][2] = smp[c][3] = p.samples[(mcu_blk + rowblk[c]) * 64 + rowsmp[c] + (ix0 >> 2)];
            } else {                                    // the other legal factors: the last block written over each pixel
                for (unsigned j = 0; j < 4; ++j) {
                    const unsigned ix = ix0 + j;
                    const unsigned kx = min(chh - 1u, ix >> 3), xu = ix - kx * 8u;
                    if (xu < 8u * dupx) smp[c][j] = p.samples[(mcu_blk + rowblk[c] + kx) * 64 + rowsmp[c] + fast_div(xu, p.dx_magic[c], p.dx_shift[c])];
                }
            }
        }
    }
    if constexpr (SINK == SINK_YUV422) {
        uint8_t* base = p.r < p.g ? p.r : p.g;                   // the macropixel's first byte: Y0 or Cb
        const unsigned sy = 8u * (unsigned)(p.r - base), sb = 8u * (unsigned)(p.g - base), sr = 8u * (unsigned)(p.b - base);
        uint32_t w[2];
#pragma unroll
        for (unsigned q = 0; q < 2; ++q) {
            const uint32_t y0 = (uint32_t)clamp8(smp[0][2 * q]), y1 = 2 * q + 1 < npx ? (uint32_t)clamp8(smp[0][2 * q + 1]) : y0;
            w[q] = y0 << sy | y1 << (sy + 16u) | (uint32_t)clamp8(smp[1][2 * q]) << sb | (uint32_t)clamp8(smp[2][2 * q]) << sr;
        }
        uint8_t* px = base + (size_t)y * p.row_stride + (size_t)x0 * 2u;
        if (npx == 4 && ((uintptr_t)px & 7u) == 0) {
            *reinterpret_cast<uint2*>(px) = make_uint2(w[0], w[1]);
        } else {
            const unsigned nb = npx > 2 ? 8u : 4u;
#pragma unroll
            for (unsigned j = 0; j < 8; ++j)
                if (j < nb) px[j] = (uint8_t)(w[j >> 2] >> (8u * (j & 3u)));
        }
    } else {
        constexpr int PIX = SINK;
        uint32_t rw = 0, gw = 0, bw = 0;
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) {
            uint32_t r, g, b;
            make_rgb(p.gray, smp[0][j], smp[1][j], smp[2][j], r, g, b);
            rw |= r << (8 * j); gw |= g << (8 * j); bw |= b << (8 * j);
        }
        if constexpr (PIX != 0) {
            const bool blue_first = p.b < p.r;                       // r, g, b: the channel bytes of pixel (0, 0)
            uint8_t* px = (blue_first ? p.b : p.r) + (size_t)y * p.row_stride + (size_t)x0 * PIX;
            store_packed4<PIX>(px, npx, blue_first ? bw : rw, gw, blue_first ? rw : bw);
        } else {
            const size_t off = (size_t)y * p.W + x0;
            store_planes4(p.r, p.g, p.b, off, npx, rw, gw, bw, (p.W & 3) == 0);   // rows start 4-byte aligned (the planes are device allocations)
        }
    }
}

// the packed 4:2:2 second stage: that template's instance with the macropixel sink
constexpr auto generic_yuv422_kernel = generic_rgb_kernel<SINK_YUV422>;

// Native component planes (GenericDecParams::ycc, jpezy_decode_jpeg_ycc on a layout that is not this project's own): component c comes
// out at its own sampling, ceil(W * H_c / hmax) x ceil(H * V_c / vmax) samples, block (kx, ky) of MCU (ux, uy) at ((ux * H_c + kx) * 8,
// (uy * V_c + ky) * 8); every byte is revise_value of the integer sample (INT_MIN from ref_int: 0).  No replication, no make_rgb.
// One thread: four samples of a component row (they lie in one block row of one block); blockIdx.z: the component.
__global__ __launch_bounds__(256) void generic_ycc_kernel(GenericDecParams p)
{
    const int c = (int)blockIdx.z;
    uint8_t* const plane = c == 0 ? p.r : c == 1 ? p.g : p.b;
    if (c >= p.ncomp || plane == nullptr) return;
    const unsigned chh = (unsigned)p.ch[c], cvv = (unsigned)p.cv[c];
    const unsigned wc = ((unsigned)p.W * chh + (unsigned)p.hmax - 1u) / (unsigned)p.hmax;
    const unsigned hc = ((unsigned)p.H * cvv + (unsigned)p.vmax - 1u) / (unsigned)p.vmax;
    const unsigned x0 = (blockIdx.x * 64u + (threadIdx.x & 63u)) * 4u;
    const unsigned y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (y >= hc || x0 >= wc) return;
    const unsigned bxq = x0 >> 3, byq = y >> 3;
    const unsigned ux = bxq / chh, kx = bxq - ux * chh, uy = byq / cvv, ky = byq - uy * cvv;
    const size_t blk = ((size_t)uy * p.mcu_cols + ux) * (size_t)p.blocks_per_mcu + (unsigned)p.blk_start[c] + ky * chh + kx;
    const int4 v = *reinterpret_cast<const int4*>(p.samples + blk * 64 + (y & 7u) * 8u + (x0 & 7u));
    const int smp[4] = { v.x, v.y, v.z, v.w };
    const unsigned npx = min(4u, wc - x0);
    const unsigned step = c ? (unsigned)p.c_step : 1u;
    uint8_t* dst = plane + (size_t)y * (c ? p.c_row_stride : p.row_stride) + (size_t)x0 * step;
    for (unsigned j = 0; j < npx; ++j) dst[j * step] = (uint8_t)min(max(smp[j], 0), 255);
}

}  // namespace generic

// the second stage of launch_dequant_idct_generic for a packed 4:2:2 sink: q is what generic_rgb_kernel would be launched with
hipError_t launch_generic_yuv422(const GenericDecParams& q, dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL(generic::generic_yuv422_kernel, grid, dim3(256), 0, s, q);
    return hipGetLastError();
}

int generic_frames_per_launch(const GenericDecParams& p)
{
    const long fblk = (long)p.mcu_cols * p.mcu_rows * p.blocks_per_mcu;
    if (fblk <= 0 || fblk > 0x7FFFFFFFL) return 0;
    const long per = 0x7FFFFFFFL / fblk;                   // the block index of a launch is 32-bit
    return per < 65535 ? (int)per : 65535;                 // the frame index is grid.z
}

hipError_t launch_dequant_idct_generic(const GenericDecParams& p_in, hipStream_t s, GenericStage2 stage2)
{
    GenericDecParams p = p_in;
    const int nfr = p.n_frames < 1 ? 1 : p.n_frames;
    const long fblk = (long)p.mcu_cols * p.mcu_rows * p.blocks_per_mcu;       // the block loop does not care where a frame ends
    if (fblk <= 0) return hipSuccess;
    const int per = generic_frames_per_launch(p);
    if (per < 1) return hipErrorInvalidValue;
    fast_div_setup((unsigned)p.hmax * 8u, &p.mw_magic, &p.mw_shift);
    fast_div_setup((unsigned)p.vmax * 8u, &p.mh_magic, &p.mh_shift);
    for (int c = 0; c < 3; ++c) {
        fast_div_setup((unsigned)(p.hmax / p.ch[c]), &p.dx_magic[c], &p.dx_shift[c]);
        fast_div_setup((unsigned)(p.vmax / p.cv[c]), &p.dy_magic[c], &p.dy_shift[c]);
    }
    const unsigned gx = ((unsigned)p.W + 255u) / 256u, gy = ((unsigned)p.H + 3u) / 4u;
    // larger batches go out as several pairs of launches; the samples scratch (per frames of one launch) is reused in stream order
    for (int f0 = 0; f0 < nfr; f0 += per) {
        GenericDecParams q = p;
        q.n_frames = nfr - f0 < per ? nfr - f0 : per;
        q.coeffs += (size_t)f0 * (size_t)fblk * 64;
        q.r += (size_t)f0 * p.plane_stride; q.g += (size_t)f0 * p.plane_stride; q.b += (size_t)f0 * p.plane_stride;
        const long nblk = fblk * q.n_frames;
        hipLaunchKernelGGL(generic::generic_idct_kernel, dim3((unsigned)((nblk + generic::G_BLOCKS - 1) / generic::G_BLOCKS)), dim3(64), 0, s, q, nblk);
        if (q.ycc) {                                            // native component planes (one frame): no plane is larger than W x H
            hipLaunchKernelGGL(generic::generic_ycc_kernel, dim3(gx, gy, (unsigned)q.ncomp), dim3(256), 0, s, q);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
            continue;
        }
        if (stage2) {                                           // another second stage over the same samples (smooth chroma upsampling)
            if (hipError_t e = stage2(q, dim3(gx, gy, (unsigned)q.n_frames), s); e != hipSuccess) return e;
            continue;
        }
        if (q.pix_bytes == 3) hipLaunchKernelGGL(generic::generic_rgb_kernel<3>, dim3(gx, gy, (unsigned)q.n_frames), dim3(256), 0, s, q);
        else if (q.pix_bytes == 4) hipLaunchKernelGGL(generic::generic_rgb_kernel<4>, dim3(gx, gy, (unsigned)q.n_frames), dim3(256), 0, s, q);
        else hipLaunchKernelGGL(generic::generic_rgb_kernel<0>, dim3(gx, gy, (unsigned)q.n_frames), dim3(256), 0, s, q);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace jpezy_dev
