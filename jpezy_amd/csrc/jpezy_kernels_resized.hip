// jpezy_kernels_resized.hip -- a batch of windows, resized: the second stage behind windows_kernel / region_kernel.  The packed pixels of
// MANY windows of different sizes, each brought to the launch's out_w x out_h by the separable triangle filter of include/jpezy_hip.h,
// BATCH OF WINDOWS, RESIZED, in 32-bit integer fixed point.
//   resample_kernel<PIX> : one workgroup = one tile of kResampleTileW x kResampleTileH output pixels of one file; the grid is 1-D over the
//       sum of the files' tiles.  A workgroup finds its file by windows_kernel's binary search over the files' first-workgroup indices
//       (ResampleDesc::wg0): the index and every descriptor field depend on blockIdx alone, so they are wave-uniform and live in scalar
//       registers.  A thread owns four consecutive OUTPUT pixels of a row.  For each of them it walks the column's vertical taps, and
//       for every such source row evaluates the horizontal pass at that column (the byte t of the definition: (2^21 + sum K * src) >> 22,
//       clipped), then accumulates K * t: the vertical pass over exactly the bytes a separate horizontal pass would have stored.  Both
//       tap loops are runtime loops over the tables' counts, so every ratio runs the same code and nothing is staged in LDS: a source of
//       4096 columns to one pixel is a loop of 8192 taps, not a tile that has to fit.  The price is that a horizontal byte is evaluated
//       once per output row that uses it (about twice when an axis shrinks, DESIGN.md 4.15 has the count).
//       Stores: the four pixels as one 12- or 16-byte store when all four exist and the address is a multiple of 4, single bytes
//       otherwise (windows_kernel's stage 2).  Byte 3 of a 32-bit pixel is 0xFF and is never read.
// No byte outside a file's out_w * PIX x out_h rectangle is written; the source is read inside the file's w x h window only (the tables
// hold first + count <= size, jpezy_resize_taps).
#include "jpezy_wave.h"

namespace jpezy_dev {
namespace resized {

constexpr int kThreads = 256;
constexpr int kGroupsX = kResampleTileW / 4;          // threads across a tile row
static_assert(kGroupsX * kResampleTileH == kThreads, "one thread per group of four output pixels of the tile");

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// the file of workgroup wg: the last descriptor whose first workgroup is <= wg (wg0 ascending, desc[0].wg0 == first workgroup of the launch)
__device__ __forceinline__ unsigned find_file(const ResampleDesc* __restrict__ desc, unsigned n, unsigned wg)
{
    unsigned lo = 0, hi = n;                      // invariant: desc[lo].wg0 <= wg, and (hi == n or desc[hi].wg0 > wg)
    while (hi - lo > 1) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (desc[mid].wg0 <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

template <int PIX>
__global__ __launch_bounds__(kThreads) void resample_kernel(ResampleParams p)
{
    const unsigned wg = p.wg_base + blockIdx.x;
    // (uniform by construction; readfirstlane tells the compiler so, and the descriptor is then read with scalar loads)
    const unsigned fi = (unsigned)__builtin_amdgcn_readfirstlane((int)find_file(p.desc, p.n_desc, wg));
    const ResampleDesc d = p.desc[fi];
    const unsigned tiles_x = ((unsigned)p.out_w + kResampleTileW - 1) / kResampleTileW;
    const unsigned local = wg - d.wg0;
    const unsigned ty = local / tiles_x, tx = local - ty * tiles_x;
    const int ox0 = (int)(tx * kResampleTileW + (threadIdx.x % kGroupsX) * 4);
    const int oy = (int)(ty * kResampleTileH + threadIdx.x / kGroupsX);
    if (ox0 >= p.out_w || oy >= p.out_h) return;
    const int npx = min(4, p.out_w - ox0);

    const uint8_t* __restrict__ const src = p.src + d.src_off;
    const int* __restrict__ const xfc = p.taps + d.xfc;
    const int* __restrict__ const xw = p.taps + d.xw;
    const unsigned yfc = (unsigned)p.taps[d.yfc + (unsigned)oy];
    const int fy = (int)(yfc & 0xFFFFu), ny = (int)(yfc >> 16);
    const int* __restrict__ const wy = p.taps + d.yw + (size_t)oy * (unsigned)d.ky;

    uint32_t w0 = 0, w1 = 0, w2 = 0;              // byte j of w0 / w1 / w2: channel byte 0 / 1 / 2 of pixel j
    for (int j = 0; j < npx; ++j) {
        const int col = d.mirror ? p.out_w - 1 - (ox0 + j) : ox0 + j;           // the column of the unmirrored result
        const unsigned fc = (unsigned)xfc[col];
        const int fx = (int)(fc & 0xFFFFu), nx = (int)(fc >> 16);
        const int* __restrict__ const wx = xw + (size_t)col * (unsigned)d.kx;
        int v0 = 1 << 21, v1 = 1 << 21, v2 = 1 << 21;
        for (int jy = 0; jy < ny; ++jy) {
            const uint8_t* __restrict__ row = src + (size_t)(fy + jy) * p.src_stride + (size_t)fx * PIX;
            int h0 = 1 << 21, h1 = 1 << 21, h2 = 1 << 21;
            for (int jx = 0; jx < nx; ++jx) {
                const int k = wx[jx];
                if (PIX == 4) {
                    const uint32_t px = *reinterpret_cast<const uint32_t*>(row + jx * 4);       // (src_off, src_stride: multiples of 4)
                    h0 += k * (int)(px & 0xFFu); h1 += k * (int)((px >> 8) & 0xFFu); h2 += k * (int)((px >> 16) & 0xFFu);
                } else {
                    h0 += k * (int)row[jx * 3]; h1 += k * (int)row[jx * 3 + 1]; h2 += k * (int)row[jx * 3 + 2];
                }
            }
            const int ky = wy[jy];
            v0 += ky * clip8(h0 >> 22); v1 += ky * clip8(h1 >> 22); v2 += ky * clip8(h2 >> 22);
        }
        w0 |= (uint32_t)clip8(v0 >> 22) << (8 * j); w1 |= (uint32_t)clip8(v1 >> 22) << (8 * j); w2 |= (uint32_t)clip8(v2 >> 22) << (8 * j);
    }

    uint8_t* px = p.dst + d.dst_off + (size_t)oy * p.dst_stride + (size_t)ox0 * PIX;
    auto byte = [](uint32_t w, unsigned j) { return (w >> (8 * j)) & 0xFFu; };
    if (npx == 4 && ((uintptr_t)px & 3u) == 0) {
        if (PIX == 3) {
            typedef unsigned v3u __attribute__((ext_vector_type(3)));
            typedef v3u v3u_a4 __attribute__((aligned(4)));
            v3u v;
            v.x = byte(w0, 0) | byte(w1, 0) << 8 | byte(w2, 0) << 16 | byte(w0, 1) << 24;
            v.y = byte(w1, 1) | byte(w2, 1) << 8 | byte(w0, 2) << 16 | byte(w1, 2) << 24;
            v.z = byte(w2, 2) | byte(w0, 3) << 8 | byte(w1, 3) << 16 | byte(w2, 3) << 24;
            *reinterpret_cast<v3u_a4*>(px) = v;
        } else {
            typedef unsigned v4u __attribute__((ext_vector_type(4)));
            typedef v4u v4u_a4 __attribute__((aligned(4)));
            v4u v;
            v.x = byte(w0, 0) | byte(w1, 0) << 8 | byte(w2, 0) << 16 | 0xFF000000u;
            v.y = byte(w0, 1) | byte(w1, 1) << 8 | byte(w2, 1) << 16 | 0xFF000000u;
            v.z = byte(w0, 2) | byte(w1, 2) << 8 | byte(w2, 2) << 16 | 0xFF000000u;
            v.w = byte(w0, 3) | byte(w1, 3) << 8 | byte(w2, 3) << 16 | 0xFF000000u;
            *reinterpret_cast<v4u_a4*>(px) = v;
        }
    } else {
        for (int j = 0; j < npx; ++j) {
            px[j * PIX] = (uint8_t)byte(w0, j); px[j * PIX + 1] = (uint8_t)byte(w1, j); px[j * PIX + 2] = (uint8_t)byte(w2, j);
            if (PIX == 4) px[j * PIX + 3] = 0xFF;
        }
    }
}

}  // namespace resized

// total_wg: the workgroups of the call, desc[k].wg0 counted from 0.  A launch takes at most 2^24 - 1 of them (launch_dequant_idct_windows'
// rule: its global size stays below 2^32), larger calls go out as several launches that start at wg_base.
hipError_t launch_resample(const ResampleParams& p, unsigned long long total_wg, hipStream_t s)
{
    if ((p.pix_bytes != 3 && p.pix_bytes != 4) || p.n_desc < 1 || total_wg < 1 || total_wg > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (p.out_w < 1 || p.out_h < 1 || p.out_w > 65535 || p.out_h > 65535 || (p.src_stride & 3u)) return hipErrorInvalidValue;
    constexpr unsigned long long per = (1ull << 24) - 1;
    for (unsigned long long w0 = 0; w0 < total_wg; w0 += per) {
        ResampleParams q = p;
        q.wg_base = (unsigned)w0;
        const unsigned n_wg = (unsigned)(total_wg - w0 < per ? total_wg - w0 : per);
        if (q.pix_bytes == 3) hipLaunchKernelGGL((resized::resample_kernel<3>), dim3(n_wg), dim3(resized::kThreads), 0, s, q);
        else hipLaunchKernelGGL((resized::resample_kernel<4>), dim3(n_wg), dim3(resized::kThreads), 0, s, q);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace jpezy_dev
