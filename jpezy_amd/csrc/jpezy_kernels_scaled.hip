// jpezy_kernels_scaled.hip -- reduced-size decode (1/2, 1/4, 1/8) for ANY baseline layout the generic pair decodes: an N x N
// inverse DCT (N = 8 / scale_denom = 4, 2, 1) over the N x N low-frequency corner of every block gives the reduced picture
// directly, with no full-size intermediate.  The reference has no such mode; the result is DEFINED as what its
// decode loop (ref decoder/jpezy_decoder.hpp:504-578, 645-676) would give if its block were N x N instead of 8 x 8:
//   scaled_idct_kernel<N> : lane = one output sample of one block, 64 / (N*N) blocks per wavefront.  The zig-zag head of each
//                           block that holds the corner (64 B for N = 4, 16 B for N = 2) is staged once through LDS and
//                           dequantised there, one coefficient per lane -- for N = 1 the one lane of a block reads its DC --
//                           and every lane accumulates its N*N terms
//                           cu*cv * (coef*Q) * cos[u*8/N][x] * cos[v*8/N][y], v outer, u inner, left to right in FP64 -- the
//                           definition's own order, nothing else -- and stores ref_int(sum / 4 + level).  There is no fast
//                           path, no guard band and no second level, so force_exact / decode_tolerance have nothing to act on
//                           and the fallback counter is not advanced.
//   scaled_rgb_kernel<PIX>: one thread per four consecutive output pixels of a row; block placement, replication, make_rgb /
//                           revise_value and the stores of generic_rgb_kernel with N in place of 8.  An MCU is hmax*N pixels
//                           wide -- as narrow as one pixel -- so every pixel finds its own MCU.
#include "jpezy_pixel_out.h"
#include "../../include/jpezy_constants.h"

namespace jpezy_dev {
namespace scaled {

__constant__ double c_cos[64] = JPEZY_COS_INIT;
__constant__ unsigned char c_zzinv[64] = JPEZY_ZZ_INV_INIT;

template <int N> struct Geo {
    static constexpr int NN = N * N;
    static constexpr int BPW = 64 / NN;               // blocks per wavefront
    static constexpr int HEAD = N == 4 ? 32 : 8;      // int16 elements of a block's zig-zag head that hold the corner (N >= 2):
                                                      // positions 0..24 for N = 4, {0, 1, 2, 4} for N = 2
    static constexpr int PIECES = HEAD / 8;           // 16-byte pieces of a head
};

template <int N>
__global__ __launch_bounds__(64) void scaled_idct_kernel(ScaledDecParams p, long nblk)
{
    using G = Geo<N>;
    const int lane = threadIdx.x;
    const long g0 = (long)blockIdx.x * G::BPW;
    const int b = lane / G::NN, s = lane % G::NN;     // block of the wavefront, sample (y, x) of the block
    const long g = g0 + b;
    const bool live = g < nblk;
    const int k = live ? (int)(g % p.blocks_per_mcu) : 0;
    int comp = 0;
    if (k >= p.blk_start[1]) comp = 1;
    if (k >= p.blk_start[2]) comp = 2;
    const int* qt = p.qt + comp * 64;

    double sum = 0;
    if constexpr (N == 1) {
        // one lane per block: its DC (ref :645-650), then the one term of the sum
        const int dct = live ? (int)p.coeffs[g * 64] * qt[0] : 0;
        sum += JPEZY_INV_SQRT2 * JPEZY_INV_SQRT2 * dct * c_cos[0] * c_cos[0];
    } else {
        __shared__ __attribute__((aligned(16))) int16_t head[G::BPW * G::HEAD];        // 256 bytes
        if (lane < G::BPW * G::PIECES) {                                              // 16 lanes, one 16-byte piece each
            const int hb = lane / G::PIECES, piece = lane % G::PIECES;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (g0 + hb < nblk) v = *reinterpret_cast<const uint4*>(p.coeffs + (g0 + hb) * 64 + piece * 8);
            *reinterpret_cast<uint4*>(head + hb * G::HEAD + piece * 8) = v;
        }
        wave_sync();
        // lane (b, s) dequantises coefficient (v, u) = (s / N, s % N) of its block (ref :645-650, 32-bit int), so that every table
        // entry and every coefficient is fetched once per block and not once per sample
        __shared__ __attribute__((aligned(16))) int dct[64];
        {
            const int nat = (s / N) * 8 + s % N;
            dct[lane] = (int)head[b * G::HEAD + c_zzinv[nat]] * qt[nat];
        }
        wave_sync();
        const int* d = dct + b * G::NN;
        const int y = s / N, x = s % N;
        double cx[N], cy[N];
#pragma unroll
        for (int u = 0; u < N; ++u) { cx[u] = c_cos[(u * 8 / N) * 8 + x]; cy[u] = c_cos[(u * 8 / N) * 8 + y]; }
#pragma unroll
        for (int v = 0; v < N; ++v) {
            const double cv = (!v) ? JPEZY_INV_SQRT2 : 1.0;
#pragma unroll
            for (int u = 0; u < N; ++u) {
                const double cu = (!u) ? JPEZY_INV_SQRT2 : 1.0;
                sum += cu * cv * d[v * N + u] * cx[u] * cy[v];
            }
        }
    }
    if (live) p.samples[g0 * G::NN + lane] = ref_int(sum / 4 + p.level);              // = samples[g * NN + s]
}

// PIX: 0 = planes; 3 / 4 = packed (interleaved) pixels of that many bytes, as in generic_rgb_kernel.
template <int PIX>
__global__ __launch_bounds__(256) void scaled_rgb_kernel(ScaledDecParams p)
{
    const unsigned x0 = (blockIdx.x * 64u + (threadIdx.x & 63u)) * 4u;
    const unsigned y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (y >= (unsigned)p.Hs || x0 >= (unsigned)p.Ws) return;
    {   // blockIdx.z is the frame
        const size_t f = blockIdx.z;
        p.samples += f * ((size_t)p.mcu_cols * p.mcu_rows * p.blocks_per_mcu << (2 * p.log2n));
        p.r += f * p.plane_stride; p.g += f * p.plane_stride; p.b += f * p.plane_stride;
    }
    const unsigned l2 = (unsigned)p.log2n;
    const unsigned mw = (unsigned)p.hmax << l2, mh = (unsigned)p.vmax << l2;
    const unsigned uy = fast_div(y, p.mh_magic, p.mh_shift), iy = y - uy * mh;
    // decode_mcu (ref :504-528) with N for 8: block (kx, ky) of a component is written at (kx*N, ky*N) as a rectangle of
    // N*dupx x N*dupy samples, ky outer, kx inner, the last write to a position stays; what is never written keeps 0 / 0x80
    unsigned rowblk[3], rowsmp[3];
    bool rowok[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned cvv = (unsigned)p.cv[c], dupy = (unsigned)p.vmax / cvv;
        const unsigned ky = min(cvv - 1u, iy >> l2), yu = iy - (ky << l2);              // last block row written over iy
        rowok[c] = c < p.ncomp && yu < (dupy << l2);
        rowblk[c] = (unsigned)p.blk_start[c] + ky * (unsigned)p.ch[c];
        rowsmp[c] = fast_div(yu, p.dy_magic[c], p.dy_shift[c]) << l2;
    }
    const unsigned npx = min(4u, (unsigned)p.Ws - x0);
    uint32_t rw = 0, gw = 0, bw = 0;
    for (unsigned j = 0; j < npx; ++j) {
        const unsigned x = x0 + j;
        const unsigned ux = fast_div(x, p.mw_magic, p.mw_shift), ix = x - ux * mw;
        const size_t mcu_blk = ((size_t)uy * p.mcu_cols + ux) * (size_t)p.blocks_per_mcu;
        int smp[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            smp[c] = c ? 0x80 : 0;                                                     // ref :104-105
            if (!rowok[c]) continue;
            const unsigned chh = (unsigned)p.ch[c], dupx = (unsigned)p.hmax / chh;
            const unsigned kx = min(chh - 1u, ix >> l2), xu = ix - (kx << l2);
            if (xu < (dupx << l2))
                smp[c] = p.samples[((mcu_blk + rowblk[c] + kx) << (2 * l2)) + rowsmp[c] + fast_div(xu, p.dx_magic[c], p.dx_shift[c])];
        }
        uint32_t r, g, b;
        make_rgb(p.gray, smp[0], smp[1], smp[2], r, g, b);                             // ref :531-578, 672-676
        rw |= r << (8 * j); gw |= g << (8 * j); bw |= b << (8 * j);
    }
    if constexpr (PIX != 0) {
        const bool blue_first = p.b < p.r;                       // r, g, b: the channel bytes of pixel (0, 0)
        uint8_t* px = (blue_first ? p.b : p.r) + (size_t)y * p.row_stride + (size_t)x0 * PIX;
        store_packed4<PIX>(px, npx, blue_first ? bw : rw, gw, blue_first ? rw : bw);
    } else {
        // planes: rows are Ws apart and frames plane_stride, neither need be a multiple of 4 -- the word store goes by the addresses
        const size_t off = (size_t)y * p.Ws + x0;
        store_planes4(p.r, p.g, p.b, off, npx, rw, gw, bw, planes_word_aligned(p.r, p.g, p.b, off));
    }
}

template <int N>
void launch_idct(const ScaledDecParams& q, long nblk, hipStream_t s)
{
    const long per = Geo<N>::BPW;
    hipLaunchKernelGGL(scaled_idct_kernel<N>, dim3((unsigned)((nblk + per - 1) / per)), dim3(64), 0, s, q, nblk);
}

}  // namespace scaled

int scaled_frames_per_launch(const ScaledDecParams& p)
{
    const long fblk = (long)p.mcu_cols * p.mcu_rows * p.blocks_per_mcu;
    if (fblk <= 0 || fblk > 0x7FFFFFFFL) return 0;
    const long per = 0x7FFFFFFFL / fblk;                   // the block index of a launch is 32-bit
    return per < 65535 ? (int)per : 65535;                 // the frame index is grid.z
}

hipError_t launch_dequant_idct_scaled(const ScaledDecParams& p_in, hipStream_t s)
{
    ScaledDecParams p = p_in;
    if (p.log2n < 0 || p.log2n > 2) return hipErrorInvalidValue;
    const int nfr = p.n_frames < 1 ? 1 : p.n_frames;
    const long fblk = (long)p.mcu_cols * p.mcu_rows * p.blocks_per_mcu;
    if (fblk <= 0) return hipSuccess;
    const int per = scaled_frames_per_launch(p);
    if (per < 1) return hipErrorInvalidValue;
    fast_div_setup((unsigned)p.hmax << p.log2n, &p.mw_magic, &p.mw_shift);
    fast_div_setup((unsigned)p.vmax << p.log2n, &p.mh_magic, &p.mh_shift);
    for (int c = 0; c < 3; ++c) {
        fast_div_setup((unsigned)(p.hmax / p.ch[c]), &p.dx_magic[c], &p.dx_shift[c]);
        fast_div_setup((unsigned)(p.vmax / p.cv[c]), &p.dy_magic[c], &p.dy_shift[c]);
    }
    const unsigned gx = ((unsigned)p.Ws + 255u) / 256u, gy = ((unsigned)p.Hs + 3u) / 4u;
    // larger batches go out as several pairs of launches; the samples scratch (the frames of one launch) is reused in stream order
    for (int f0 = 0; f0 < nfr; f0 += per) {
        ScaledDecParams q = p;
        q.n_frames = nfr - f0 < per ? nfr - f0 : per;
        q.coeffs += (size_t)f0 * (size_t)fblk * 64;
        q.r += (size_t)f0 * p.plane_stride; q.g += (size_t)f0 * p.plane_stride; q.b += (size_t)f0 * p.plane_stride;
        const long nblk = fblk * q.n_frames;
        if (p.log2n == 2) scaled::launch_idct<4>(q, nblk, s);
        else if (p.log2n == 1) scaled::launch_idct<2>(q, nblk, s);
        else scaled::launch_idct<1>(q, nblk, s);
        const dim3 grid(gx, gy, (unsigned)q.n_frames);
        if (q.pix_bytes == 3) hipLaunchKernelGGL(scaled::scaled_rgb_kernel<3>, grid, dim3(256), 0, s, q);
        else if (q.pix_bytes == 4) hipLaunchKernelGGL(scaled::scaled_rgb_kernel<4>, grid, dim3(256), 0, s, q);
        else hipLaunchKernelGGL(scaled::scaled_rgb_kernel<0>, grid, dim3(256), 0, s, q);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace jpezy_dev
