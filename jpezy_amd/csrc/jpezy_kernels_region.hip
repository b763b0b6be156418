// jpezy_kernels_region.hip -- region-of-interest decode: a window of the picture, full size or reduced (1/2, 1/4, 1/8), for ANY baseline
// layout the generic pair decodes.  Chroma is replicated, never interpolated, and make_rgb is per pixel, so an output pixel depends only
// on the MCU that covers it: the window is DEFINED as the existing (scaled) decode, sliced.  One launch, no intermediate in
// device memory:
//   region_kernel<N, PIX> : one workgroup = one MCU that intersects the window (grid: window MCU columns, window MCU rows, frame).
//       stage 1   the N x N low-frequency corner of every block of the MCU is dequantised into LDS (32-bit int), then every thread
//                 evaluates samples of it: N*N terms cu*cv * (coef*Q) * cos[u*8/N][x] * cos[v*8/N][y], v outer, u inner, left to right
//                 in FP64 -- scaled_idct_kernel's scheme, with N = 8 as well (there it is the generic pair's reference-order path, which
//                 the fast paths of the full-size kernels are guarded to reproduce) -- and leaves ref_int(sum / 4 + level) in LDS.  No
//                 fast path, no guard band: force_exact / decode_tolerance have nothing to act on, the fallback counter is not advanced.
//       stage 2   the MCU's pixels that lie in the window, four consecutive OUTPUT pixels of a row per thread: block placement,
//                 replication, make_rgb / revise_value and the store forms of scaled_rgb_kernel, stored at (X - x, Y - y).  A group of
//                 four that another MCU shares, or whose address is no multiple of 4, goes out as single bytes.
// Only the coefficient blocks of MCUs that intersect the window are read; no byte outside the w x h output is written.
#include "jpezy_wave.h"
#include "../../include/jpezy_constants.h"

namespace jpezy_dev {
namespace region {

__constant__ double c_cos[64] = JPEZY_COS_INIT;
__constant__ unsigned char c_zzinv[64] = JPEZY_ZZ_INV_INIT;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 48;            // 3 components of at most 4 x 4 blocks

__device__ __forceinline__ uint32_t revise(double v) { return (v < 0.0) ? 0u : (v > 255.0) ? 255u : (uint32_t)v; }

// PIX: 0 = planes; 3 / 4 = packed (interleaved) pixels of that many bytes, as in scaled_rgb_kernel.
template <int N, int PIX>
__global__ __launch_bounds__(kThreads) void region_kernel(RegionDecParams p)
{
    constexpr int NN = N * N;
    constexpr unsigned l2 = N == 8 ? 3 : N == 4 ? 2 : N == 2 ? 1 : 0;
    __shared__ int dct[kMaxBlocks * NN];          // dequantised corner of every block, [block][v * N + u]
    __shared__ int smp[kMaxBlocks * NN];          // samples, [block][y * N + x]
    const unsigned ux = (unsigned)p.ux0 + blockIdx.x, uy = (unsigned)p.uy0 + blockIdx.y;
    const size_t f = blockIdx.z;
    const size_t mcu = (f * (size_t)p.mcu_rows + uy) * (size_t)p.mcu_cols + ux;
    const int16_t* co = p.coeffs + mcu * (size_t)p.blocks_per_mcu * 64;
    const int nsmp = p.blocks_per_mcu * NN;

    // ---- stage 1: the MCU's samples ----
    for (int i = threadIdx.x; i < nsmp; i += kThreads) {      // ref :645-650, 32-bit int
        const int k = i / NN, s = i % NN;
        int comp = 0;
        if (k >= p.blk_start[1]) comp = 1;
        if (k >= p.blk_start[2]) comp = 2;
        const int nat = (s / N) * 8 + s % N;
        dct[i] = (int)co[k * 64 + c_zzinv[nat]] * p.qt[comp * 64 + nat];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nsmp; i += kThreads) {
        const int k = i / NN, s = i % NN;
        const int y = s / N, x = s % N;
        const int* d = dct + k * NN;
        double cx[N], cy[N];
#pragma unroll
        for (int u = 0; u < N; ++u) { cx[u] = c_cos[(u * 8 / N) * 8 + x]; cy[u] = c_cos[(u * 8 / N) * 8 + y]; }
        double sum = 0;
#pragma unroll
        for (int v = 0; v < N; ++v) {
            const double cv = (!v) ? JPEZY_INV_SQRT2 : 1.0;
#pragma unroll
            for (int u = 0; u < N; ++u) {
                const double cu = (!u) ? JPEZY_INV_SQRT2 : 1.0;
                sum += cu * cv * d[v * N + u] * cx[u] * cy[v];
            }
        }
        smp[i] = ref_int(sum / 4 + p.level);
    }
    __syncthreads();

    // ---- stage 2: the MCU's pixels inside the window ----
    const int mw = p.hmax << l2, mh = p.vmax << l2;
    const int X0 = max((int)ux * mw, p.x), X1 = min((int)(ux + 1) * mw, p.x + p.w);      // picture coordinates
    const int Y0 = max((int)uy * mh, p.y), Y1 = min((int)(uy + 1) * mh, p.y + p.h);
    if (X1 <= X0 || Y1 <= Y0) return;
    const int ox_lo = X0 - p.x, ox_hi = X1 - p.x;                                       // output columns [ox_lo, ox_hi)
    const int g0 = ox_lo >> 2, ng = ((ox_hi - 1) >> 2) - g0 + 1, nitems = ng * (Y1 - Y0);
    uint8_t* const out_r = p.r + f * p.plane_stride;
    uint8_t* const out_g = p.g + f * p.plane_stride;
    uint8_t* const out_b = p.b + f * p.plane_stride;
    for (int i = threadIdx.x; i < nitems; i += kThreads) {
        const int gy = i / ng, gx = i - gy * ng;
        const int Y = Y0 + gy;
        const unsigned oy = (unsigned)(Y - p.y), iy = (unsigned)(Y - (int)uy * mh);
        const int ox0 = max((g0 + gx) * 4, ox_lo), ox1 = min((g0 + gx) * 4 + 4, ox_hi);
        const unsigned npx = (unsigned)(ox1 - ox0);                                     // 4: ox0 is a multiple of 4
        // decode_mcu (ref :504-528) with N for 8: block (kx, ky) of a component is written at (kx*N, ky*N) as a rectangle of
        // N*dupx x N*dupy samples, ky outer, kx inner, the last write to a position stays; what is never written keeps 0 / 0x80
        unsigned rowblk[3], rowsmp[3];
        bool rowok[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned cvv = (unsigned)p.cv[c], dupy = (unsigned)p.vmax / cvv;
            const unsigned ky = min(cvv - 1u, iy >> l2), yu = iy - (ky << l2);          // last block row written over iy
            rowok[c] = c < p.ncomp && yu < (dupy << l2);
            rowblk[c] = (unsigned)p.blk_start[c] + ky * (unsigned)p.ch[c];
            rowsmp[c] = (yu / dupy) << l2;
        }
        uint32_t rw = 0, gw = 0, bw = 0;
        for (unsigned j = 0; j < npx; ++j) {
            const unsigned ix = (unsigned)(p.x + ox0 - (int)ux * mw) + j;
            int sv[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sv[c] = c ? 0x80 : 0;                                                  // ref :104-105
                if (!rowok[c]) continue;
                const unsigned chh = (unsigned)p.ch[c], dupx = (unsigned)p.hmax / chh;
                const unsigned kx = min(chh - 1u, ix >> l2), xu = ix - (kx << l2);
                if (xu < (dupx << l2)) sv[c] = smp[((rowblk[c] + kx) << (2 * l2)) + rowsmp[c] + xu / dupx];
            }
            const double yp = sv[0], up = sv[1], vp = sv[2];
            uint32_t r, g, b;
            if (!p.gray) {                                                             // make_rgb, ref :531-578, 672-676
                r = revise(yp + (vp - 0x80) * 1.4020);
                g = revise(yp - (up - 0x80) * 0.3441 - (vp - 0x80) * 0.7139);
                b = revise(yp + (up - 0x80) * 1.7718);
            } else {
                r = g = b = revise(yp);
            }
            rw |= r << (8 * j); gw |= g << (8 * j); bw |= b << (8 * j);
        }
        if (PIX != 0) {
            const bool blue_first = out_b < out_r;                   // r, g, b: the channel bytes of pixel (0, 0)
            uint8_t* px = (blue_first ? out_b : out_r) + (size_t)oy * p.row_stride + (size_t)ox0 * PIX;
            const uint32_t fw = blue_first ? bw : rw, tw = blue_first ? rw : bw;
            auto byte = [](uint32_t w, unsigned j) { return (w >> (8 * j)) & 0xFFu; };
            if (npx == 4 && ((uintptr_t)px & 3u) == 0) {
                if (PIX == 3) {
                    typedef unsigned v3u __attribute__((ext_vector_type(3)));
                    typedef v3u v3u_a4 __attribute__((aligned(4)));
                    v3u v;
                    v.x = byte(fw, 0) | byte(gw, 0) << 8 | byte(tw, 0) << 16 | byte(fw, 1) << 24;
                    v.y = byte(gw, 1) | byte(tw, 1) << 8 | byte(fw, 2) << 16 | byte(gw, 2) << 24;
                    v.z = byte(tw, 2) | byte(fw, 3) << 8 | byte(gw, 3) << 16 | byte(tw, 3) << 24;
                    *reinterpret_cast<v3u_a4*>(px) = v;
                } else {
                    typedef unsigned v4u __attribute__((ext_vector_type(4)));
                    typedef v4u v4u_a4 __attribute__((aligned(4)));
                    v4u v;
                    v.x = byte(fw, 0) | byte(gw, 0) << 8 | byte(tw, 0) << 16 | 0xFF000000u;
                    v.y = byte(fw, 1) | byte(gw, 1) << 8 | byte(tw, 1) << 16 | 0xFF000000u;
                    v.z = byte(fw, 2) | byte(gw, 2) << 8 | byte(tw, 2) << 16 | 0xFF000000u;
                    v.w = byte(fw, 3) | byte(gw, 3) << 8 | byte(tw, 3) << 16 | 0xFF000000u;
                    *reinterpret_cast<v4u_a4*>(px) = v;
                }
            } else {
                for (unsigned j = 0; j < npx; ++j) {
                    px[j * PIX] = (uint8_t)byte(fw, j); px[j * PIX + 1] = (uint8_t)byte(gw, j); px[j * PIX + 2] = (uint8_t)byte(tw, j);
                    if (PIX == 4) px[j * PIX + 3] = 0xFF;
                }
            }
            continue;
        }
        // planes: rows are w apart and frames plane_stride, neither need be a multiple of 4 -- the word store goes by the addresses
        const size_t off = (size_t)oy * (unsigned)p.w + (unsigned)ox0;
        if (npx == 4 && ((((uintptr_t)(out_r + off)) | ((uintptr_t)(out_g + off)) | ((uintptr_t)(out_b + off))) & 3u) == 0) {
            *reinterpret_cast<uint32_t*>(out_r + off) = rw;
            *reinterpret_cast<uint32_t*>(out_g + off) = gw;
            *reinterpret_cast<uint32_t*>(out_b + off) = bw;
        } else {
            for (unsigned j = 0; j < npx; ++j) {
                out_r[off + j] = (uint8_t)(rw >> (8 * j)); out_g[off + j] = (uint8_t)(gw >> (8 * j)); out_b[off + j] = (uint8_t)(bw >> (8 * j));
            }
        }
    }
}

template <int N>
void launch(const RegionDecParams& q, const dim3& grid, hipStream_t s)
{
    if (q.pix_bytes == 3) hipLaunchKernelGGL((region_kernel<N, 3>), grid, dim3(kThreads), 0, s, q);
    else if (q.pix_bytes == 4) hipLaunchKernelGGL((region_kernel<N, 4>), grid, dim3(kThreads), 0, s, q);
    else hipLaunchKernelGGL((region_kernel<N, 0>), grid, dim3(kThreads), 0, s, q);
}

}  // namespace region

hipError_t launch_dequant_idct_region(const RegionDecParams& p, hipStream_t s)
{
    if (p.log2n < 0 || p.log2n > 3 || p.blocks_per_mcu < 1 || p.blocks_per_mcu > region::kMaxBlocks) return hipErrorInvalidValue;
    if (p.ucols < 1 || p.urows < 1 || p.urows > 65535) return hipErrorInvalidValue;
    const int nfr = p.n_frames < 1 ? 1 : p.n_frames;
    const size_t fcoef = (size_t)p.mcu_cols * p.mcu_rows * p.blocks_per_mcu * 64;
    constexpr int per = 65535;                                 // the frame index is grid.z: larger batches go out as several launches
    for (int f0 = 0; f0 < nfr; f0 += per) {
        RegionDecParams q = p;
        q.n_frames = nfr - f0 < per ? nfr - f0 : per;
        q.coeffs += (size_t)f0 * fcoef;
        q.r += (size_t)f0 * p.plane_stride; q.g += (size_t)f0 * p.plane_stride; q.b += (size_t)f0 * p.plane_stride;
        const dim3 grid((unsigned)p.ucols, (unsigned)p.urows, (unsigned)q.n_frames);
        if (p.log2n == 3) region::launch<8>(q, grid, s);
        else if (p.log2n == 2) region::launch<4>(q, grid, s);
        else if (p.log2n == 1) region::launch<2>(q, grid, s);
        else region::launch<1>(q, grid, s);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace jpezy_dev
