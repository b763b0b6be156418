// jpezy_resample_core.h -- what resample_kernel<PIX> (jpezy_kernels_resized.hip) and resample_tensor_kernel<DT, C>
// (jpezy_kernels_resized_tensor.hip) share: the tiling, the search for a workgroup's file and the two tap loops that leave a thread's four
// output pixels in registers.  The kernels differ in their store stage only.
#pragma once
#include "jpezy_wave.h"

namespace jpezy_dev {
namespace resized {

constexpr int kThreads = 256;
constexpr int kGroupsX = kResampleTileW / 4;          // threads across a tile row
static_assert(kGroupsX * kResampleTileH == kThreads, "one thread per group of four output pixels of the tile");

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// the descriptor of the workgroup's file (uniform by construction; readfirstlane tells the compiler so, and the descriptor is then read
// with scalar loads)
__device__ __forceinline__ const ResampleDesc& workgroup_file(const ResampleParams& p)
{
    return p.desc[(unsigned)__builtin_amdgcn_readfirstlane((int)find_file(p.desc, p.n_desc, p.wg_base + blockIdx.x))];
}

// The thread's group of output pixels of the file d: the first pixel (ox0, oy), how many of the four exist (npx), and their bytes -- byte j
// of w0 / w1 / w2: channel byte 0 / 1 / 2 of pixel j.  false: the thread lies outside the output (nothing is set).
template <int PIX>
__device__ __forceinline__ bool resample_four(const ResampleParams& p, const ResampleDesc& d, int& ox0, int& oy, int& npx, uint32_t& w0, uint32_t& w1,
                                              uint32_t& w2)
{
    const unsigned wg = p.wg_base + blockIdx.x;
    const unsigned tiles_x = ((unsigned)p.out_w + kResampleTileW - 1) / kResampleTileW;
    const unsigned local = wg - d.wg0;
    const unsigned ty = local / tiles_x, tx = local - ty * tiles_x;
    ox0 = (int)(tx * kResampleTileW + (threadIdx.x % kGroupsX) * 4);
    oy = (int)(ty * kResampleTileH + threadIdx.x / kGroupsX);
    if (ox0 >= p.out_w || oy >= p.out_h) return false;
    npx = min(4, p.out_w - ox0);

    const uint8_t* __restrict__ const src = p.src + d.src_off;
    const int* __restrict__ const xfc = p.taps + d.xfc;
    const int* __restrict__ const xw = p.taps + d.xw;
    const unsigned yfc = (unsigned)p.taps[d.yfc + (unsigned)oy];
    const int fy = (int)(yfc & 0xFFFFu), ny = (int)(yfc >> 16);
    const int* __restrict__ const wy = p.taps + d.yw + (size_t)oy * (unsigned)d.ky;

    w0 = 0; w1 = 0; w2 = 0;
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
    return true;
}

}  // namespace resized
}  // namespace jpezy_dev
