// jpezy_kernels_windows.hip -- a batch of crop windows: the windows of MANY files in one launch.  The files share a layout (sampling factors,
// components, precision) and a scale; size, window, destination and quantiser tables are each file's own (include/jpezy_hip.h, BATCH OF
// WINDOWS).
//   windows_kernel<N, PIX> : one workgroup = one MCU that intersects some file's window; the grid is 1-D over the sum of the files' window
//       MCUs.  A workgroup finds its file by a binary search over the files' first-workgroup indices (WindowDesc::wg0) -- the index and every
//       descriptor field depend on blockIdx alone, so they are wave-uniform and live in scalar registers -- and then runs the two stages of
//       region_kernel (jpezy_kernels_region.hip) on that MCU:
//       stage 1   the N x N low-frequency corner of every block of the MCU is dequantised into LDS (32-bit int) with the file's own
//                 dequantiser set, then every thread evaluates samples of it: N*N terms cu*cv * (coef*Q) * cos[u*8/N][x] * cos[v*8/N][y],
//                 v outer, u inner, left to right in FP64, ref_int(sum / 4 + level) into LDS.  No fast path, no guard band.
//       stage 2   the MCU's pixels that lie in the window, four consecutive OUTPUT pixels of a row per thread: block placement, replication,
//                 make_rgb / revise_value, stored at (X - x, Y - y) of the file's slot.  A group of four that another MCU shares, or whose
//                 address is no multiple of 4, goes out as single bytes.
// The body of the two stages is region_kernel's, statement for statement, as a copy: sharing it through a header moved the register
// allocation of region_kernel's N = 4 instances, so that kernel stays as it is.  A change to the arithmetic belongs in both.
// Only the coefficient blocks of MCUs that intersect a window are read; no byte outside a file's w x h rectangle is written.
#include "jpezy_wave.h"
#include "../../include/jpezy_constants.h"

namespace jpezy_dev {
namespace windows {

static __constant__ double c_cos[64] = JPEZY_COS_INIT;
static __constant__ unsigned char c_zzinv[64] = JPEZY_ZZ_INV_INIT;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 48;            // 3 components of at most 4 x 4 blocks

__device__ __forceinline__ uint32_t revise(double v) { return (v < 0.0) ? 0u : (v > 255.0) ? 255u : (uint32_t)v; }

// The window of one picture as a workgroup sees it: MCU (ux, uy) of the picture at scale 8 / N, the window {x, y, w, h} in that picture's
// coordinates, the MCU's coefficients, the picture's dequantisers [3 comps][64] and the bytes of the window's pixel (0, 0).
struct McuView {
    const int16_t* co;
    const int* qt;
    unsigned ux, uy;
    int x, y, w, h;
    uint8_t *out_r, *out_g, *out_b;       // planes: rows w apart; packed: the channel bytes of the first pixel, rows row_stride apart
    size_t row_stride;
    bool blue_first;                      // packed: blue is byte 0 of a pixel
};

// p: the launch's layout constants.  dct, smp: kMaxBlocks * N * N ints of LDS each.  PIX: 3 / 4 = packed pixels of that many bytes (0, planes:
// region_kernel's third form, kept so that the body stays a copy; no instance of it is launched here).
template <int N, int PIX>
__device__ __forceinline__ void decode_mcu_window(const WindowsParams& p, const McuView& m, int* dct, int* smp)
{
    constexpr int NN = N * N;
    constexpr unsigned l2 = N == 8 ? 3 : N == 4 ? 2 : N == 2 ? 1 : 0;
    const int16_t* co = m.co;
    const unsigned ux = m.ux, uy = m.uy;
    const int nsmp = p.blocks_per_mcu * NN;

    // ---- stage 1: the MCU's samples ----
    for (int i = threadIdx.x; i < nsmp; i += kThreads) {      // ref :645-650, 32-bit int
        const int k = i / NN, s = i % NN;
        int comp = 0;
        if (k >= p.blk_start[1]) comp = 1;
        if (k >= p.blk_start[2]) comp = 2;
        const int nat = (s / N) * 8 + s % N;
        dct[i] = (int)co[k * 64 + c_zzinv[nat]] * m.qt[comp * 64 + nat];
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
    const int X0 = max((int)ux * mw, m.x), X1 = min((int)(ux + 1) * mw, m.x + m.w);      // picture coordinates
    const int Y0 = max((int)uy * mh, m.y), Y1 = min((int)(uy + 1) * mh, m.y + m.h);
    if (X1 <= X0 || Y1 <= Y0) return;
    const int ox_lo = X0 - m.x, ox_hi = X1 - m.x;                                       // output columns [ox_lo, ox_hi)
    const int g0 = ox_lo >> 2, ng = ((ox_hi - 1) >> 2) - g0 + 1, nitems = ng * (Y1 - Y0);
    uint8_t* const out_r = m.out_r;
    uint8_t* const out_g = m.out_g;
    uint8_t* const out_b = m.out_b;
    for (int i = threadIdx.x; i < nitems; i += kThreads) {
        const int gy = i / ng, gx = i - gy * ng;
        const int Y = Y0 + gy;
        const unsigned oy = (unsigned)(Y - m.y), iy = (unsigned)(Y - (int)uy * mh);
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
            const unsigned ix = (unsigned)(m.x + ox0 - (int)ux * mw) + j;
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
            const bool blue_first = m.blue_first;
            uint8_t* px = (blue_first ? out_b : out_r) + (size_t)oy * m.row_stride + (size_t)ox0 * PIX;
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
        const size_t off = (size_t)oy * (unsigned)m.w + (unsigned)ox0;
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

// the file of workgroup wg: the last descriptor whose first workgroup is <= wg (wg0 ascending, desc[0].wg0 == first workgroup of the launch)
__device__ __forceinline__ unsigned find_file(const WindowDesc* __restrict__ desc, unsigned n, unsigned wg)
{
    unsigned lo = 0, hi = n;                      // invariant: desc[lo].wg0 <= wg, and (hi == n or desc[hi].wg0 > wg)
    while (hi - lo > 1) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (desc[mid].wg0 <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

template <int N, int PIX>
__global__ __launch_bounds__(kThreads) void windows_kernel(WindowsParams p)
{
    constexpr int NN = N * N;
    __shared__ int dct[kMaxBlocks * NN];          // dequantised corner of every block, [block][v * N + u]
    __shared__ int smp[kMaxBlocks * NN];          // samples, [block][y * N + x]
    const unsigned wg = p.wg_base + blockIdx.x;
    // (uniform by construction; readfirstlane tells the compiler so, and the descriptor is then read with scalar loads)
    const unsigned fi = (unsigned)__builtin_amdgcn_readfirstlane((int)find_file(p.desc, p.n_desc, wg));
    const WindowDesc d = p.desc[fi];
    const unsigned local = wg - d.wg0, ucols = (unsigned)d.ucols;
    const unsigned row = local / ucols, col = local - row * ucols;
    const unsigned ux = (unsigned)d.ux0 + col, uy = (unsigned)d.uy0 + row;
    const size_t mcu = (size_t)uy * (size_t)d.mcu_cols + ux;
    uint8_t* const px0 = p.pix + d.out_off;
    const McuView m = { p.coeffs + d.coeff_off + mcu * (size_t)p.blocks_per_mcu * 64, p.qsets + (size_t)d.qset * 192, ux, uy, d.x, d.y, d.w, d.h,
                        px0 + (p.swap_rb ? 2 : 0), px0 + 1, px0 + (p.swap_rb ? 0 : 2), p.row_stride, p.swap_rb != 0 };
    decode_mcu_window<N, PIX>(p, m, dct, smp);
}

template <int N>
void launch(const WindowsParams& q, unsigned n_wg, hipStream_t s)
{
    if (q.pix_bytes == 3) hipLaunchKernelGGL((windows_kernel<N, 3>), dim3(n_wg), dim3(kThreads), 0, s, q);
    else hipLaunchKernelGGL((windows_kernel<N, 4>), dim3(n_wg), dim3(kThreads), 0, s, q);
}

}  // namespace windows

// total_wg: the workgroups of the call, desc[k].wg0 counted from 0.  A launch takes at most 2^24 - 1 of them -- far below 2^31, and its
// global size (workgroups x 256 threads) stays below 2^32 --, larger calls go out as several launches that start at wg_base.
hipError_t launch_dequant_idct_windows(const WindowsParams& p, unsigned long long total_wg, hipStream_t s)
{
    if (p.log2n < 0 || p.log2n > 3 || p.blocks_per_mcu < 1 || p.blocks_per_mcu > windows::kMaxBlocks) return hipErrorInvalidValue;
    if ((p.pix_bytes != 3 && p.pix_bytes != 4) || p.n_desc < 1 || total_wg < 1 || total_wg > 0xFFFFFFFFull) return hipErrorInvalidValue;
    constexpr unsigned long long per = (1ull << 24) - 1;
    for (unsigned long long w0 = 0; w0 < total_wg; w0 += per) {
        WindowsParams q = p;
        q.wg_base = (unsigned)w0;
        const unsigned n_wg = (unsigned)(total_wg - w0 < per ? total_wg - w0 : per);
        if (p.log2n == 3) windows::launch<8>(q, n_wg, s);
        else if (p.log2n == 2) windows::launch<4>(q, n_wg, s);
        else if (p.log2n == 1) windows::launch<2>(q, n_wg, s);
        else windows::launch<1>(q, n_wg, s);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace jpezy_dev
