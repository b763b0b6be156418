// jpezy_resample_core.h -- what resample_kernel<PIX> (jpezy_kernels_resized.hip) and resample_tensor_kernel<DT, C>
// (jpezy_kernels_resized_tensor.hip) share: the tiling, the search for a workgroup's file and the two tap loops that leave a thread's four
// output pixels in registers -- in the direct form (resample_four) and in the two-pass form through LDS (resample_four_tiled).  The
// kernels differ in their store stage only.
#pragma once
#include "jpezy_wave.h"

namespace jpezy_dev {
namespace resized {

constexpr int kThreads = 256;
constexpr int kGroupsX = kResampleTileW / 4;          // threads across a tile row
static_assert(kGroupsX * kResampleTileH == kThreads, "one thread per group of four output pixels of the tile");

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// clip8(acc >> 22), clamped BEFORE the shift: acc < 0 gives 0, acc >= 2^30 gives 255, and 0 .. 2^30 - 1 shifted right is 0 .. 255.  The
// two-pass form packs four such bytes with constant shifts, and from clip8(a >> 22) | clip8(b >> 22) << 8 the compiler selects
// v_ashr_pk_u8_i32, whose result on the MI355X kept the upper 16 bits of whatever the destination register held before (seen as
// stray bits of a weight in byte 2 of the BGRA kernel's third channel; tests/test_gpu_resize_filters.py pins the bytes).  A logical
// shift of a clamped value is not that pattern.
__device__ __forceinline__ uint32_t clip8_of_acc(int acc) { return (uint32_t)(acc < 0 ? 0 : acc > 0x3FFFFFFF ? 0x3FFFFFFF : acc) >> 22; }

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

// The two-pass form of resample_four: the same bytes, the horizontal pass evaluated ONCE per source row of the tile and
// kept in LDS, not once per output row that uses it.  Called by every thread of the workgroup (it holds a barrier); the caller's branch
// on ResampleDesc::tiled is wave-uniform, the descriptor being read with scalar loads.
//   Pass 1  the tile's source rows: row0 = first[oy0] to first[oy1] + count[oy1] (oy0, oy1 the tile's first and last output row; first
//           and first + count never decrease with the row, so every output row of the tile reads inside that span).  The span is read
//           from the file's own y table and is at most kResampleTileRows (the host set ResampleDesc::tiled from the same table; a
//           span that is larger all the same takes the direct loop, so the buffer's bound does not rest on the host alone).  A work
//           item is (source row, group of four columns); the 256 threads loop over span * 16 of them.  The columns are those of the
//           UNMIRRORED result: slot c of the tile is column u0 + c, u0 = tx0 (not mirrored) or out_w - 1 - (tx0 + 63) (mirrored; the
//           tile's output columns reversed).  Slots outside 0..out_w-1 hold 0 and are never stored.  The horizontal taps come from
//           global memory in a runtime loop (any nx), exactly resample_four's inner loop.
//   LDS     word (row r, channel c, group g) at r * kTilePitch + c * 16 + g, byte j = column slot 4g + j: the form w0 / w1 / w2 have.
//   Pass 2  after ONE barrier a thread walks its row's vertical taps: per tap one ds_read_b32 per channel and four multiply-adds each.
//           A mirrored file reads group 15 - g and reverses the four bytes of each word at the hand-over (output pixel j of group g is
//           slot 63 - 4g - j).
//   Banks   ds_write_b32 / ds_read_b32 bank = word % 32, conflicts among the 32 lanes of a half-wave.  Pass 1: a half-wave writes two
//           consecutive rows x 16 groups of one channel: words r * 48 + c * 16 + g and (r + 1) * 48 + c * 16 + g, and 48 = 16 (mod 32)
//           puts the two rows on the two halves of the banks: conflict-free.  Pass 2: a half-wave is two output rows oy, oy + 1 x 16
//           groups, reading source rows a distance D = first[oy + 1] - first[oy] apart at the same tap: D = 0 is one address per
//           bank (broadcast), D odd is conflict-free by the same 48 = 16 (mod 32), D even and not 0 is 2-way.  No row pitch serves
//           both D = 1 and D = 2 (P = 16 and 2P = 16 mod 32 exclude each other) and D = 1 is what pass 1 always writes, so the pitch
//           is the unpadded 48.  The 2-way case (ratios near 2) costs one LDS cycle more on 3 reads beside 12 multiply-adds and their
//           byte extracts per tap: the loop stays VALU-bound.
constexpr int kTilePitch = 3 * kGroupsX;              // 32-bit words per source row in LDS
constexpr int kTileWords = kResampleTileRows * kTilePitch;

template <int PIX>
__device__ __forceinline__ bool resample_four_tiled(const ResampleParams& p, const ResampleDesc& d, uint32_t* __restrict__ lds, int& ox0, int& oy,
                                                    int& npx, uint32_t& w0, uint32_t& w1, uint32_t& w2)
{
    const unsigned wg = p.wg_base + blockIdx.x;
    const unsigned tiles_x = ((unsigned)p.out_w + kResampleTileW - 1) / kResampleTileW;
    const unsigned local = wg - d.wg0;
    const unsigned ty = local / tiles_x, tx = local - ty * tiles_x;
    const int tx0 = (int)(tx * kResampleTileW), oy0 = (int)(ty * kResampleTileH);
    const int oy1 = min(oy0 + kResampleTileH, p.out_h) - 1;
    const unsigned yfc0 = (unsigned)p.taps[d.yfc + (unsigned)oy0], yfc1 = (unsigned)p.taps[d.yfc + (unsigned)oy1];
    const int row0 = (int)(yfc0 & 0xFFFFu);
    const int span = (int)(yfc1 & 0xFFFFu) + (int)(yfc1 >> 16) - row0;
    if (span > kResampleTileRows) return resample_four<PIX>(p, d, ox0, oy, npx, w0, w1, w2);      // (uniform: both from scalar loads)

    const uint8_t* __restrict__ const src = p.src + d.src_off;
    const int* __restrict__ const xfc = p.taps + d.xfc;
    const int* __restrict__ const xw = p.taps + d.xw;
    const int u0 = d.mirror ? p.out_w - kResampleTileW - tx0 : tx0;
    for (int it = (int)threadIdx.x; it < span * kGroupsX; it += kThreads) {
        const int r = it / kGroupsX, g = it % kGroupsX;
        const uint8_t* __restrict__ const row = src + (size_t)(row0 + r) * p.src_stride;
        uint32_t a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int u = u0 + 4 * g + j;
            if (u < 0 || u >= p.out_w) continue;
            const unsigned fc = (unsigned)xfc[u];
            const int fx = (int)(fc & 0xFFFFu), nx = (int)(fc >> 16);
            const int* __restrict__ const wx = xw + (size_t)u * (unsigned)d.kx;
            const uint8_t* __restrict__ const at = row + (size_t)fx * PIX;
            int h0 = 1 << 21, h1 = 1 << 21, h2 = 1 << 21;
            for (int jx = 0; jx < nx; ++jx) {
                const int k = wx[jx];
                if (PIX == 4) {
                    const uint32_t px = *reinterpret_cast<const uint32_t*>(at + jx * 4);        // (src_off, src_stride: multiples of 4)
                    h0 += k * (int)(px & 0xFFu); h1 += k * (int)((px >> 8) & 0xFFu); h2 += k * (int)((px >> 16) & 0xFFu);
                } else {
                    h0 += k * (int)at[jx * 3]; h1 += k * (int)at[jx * 3 + 1]; h2 += k * (int)at[jx * 3 + 2];
                }
            }
            a0 |= clip8_of_acc(h0) << (8 * j); a1 |= clip8_of_acc(h1) << (8 * j); a2 |= clip8_of_acc(h2) << (8 * j);
        }
        uint32_t* const at = lds + r * kTilePitch + g;
        at[0] = a0; at[kGroupsX] = a1; at[2 * kGroupsX] = a2;
    }
    __syncthreads();

    const int g = (int)(threadIdx.x % kGroupsX);
    ox0 = tx0 + g * 4;
    oy = oy0 + (int)(threadIdx.x / kGroupsX);
    if (ox0 >= p.out_w || oy >= p.out_h) return false;
    npx = min(4, p.out_w - ox0);
    const unsigned yfc = (unsigned)p.taps[d.yfc + (unsigned)oy];
    const int fy = (int)(yfc & 0xFFFFu), ny = (int)(yfc >> 16);
    const int* __restrict__ const wy = p.taps + d.yw + (size_t)oy * (unsigned)d.ky;
    const uint32_t* __restrict__ const col = lds + (fy - row0) * kTilePitch + (d.mirror ? kGroupsX - 1 - g : g);
    int v0[4], v1[4], v2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v0[j] = v1[j] = v2[j] = 1 << 21;
    for (int jy = 0; jy < ny; ++jy) {
        const int ky = wy[jy];
        const uint32_t t0 = col[jy * kTilePitch], t1 = col[jy * kTilePitch + kGroupsX], t2 = col[jy * kTilePitch + 2 * kGroupsX];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v0[j] += ky * (int)((t0 >> (8 * j)) & 0xFFu); v1[j] += ky * (int)((t1 >> (8 * j)) & 0xFFu); v2[j] += ky * (int)((t2 >> (8 * j)) & 0xFFu);
        }
    }
    w0 = 0; w1 = 0; w2 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        w0 |= clip8_of_acc(v0[j]) << (8 * j); w1 |= clip8_of_acc(v1[j]) << (8 * j); w2 |= clip8_of_acc(v2[j]) << (8 * j);
    }
    if (d.mirror) { w0 = __builtin_bswap32(w0); w1 = __builtin_bswap32(w1); w2 = __builtin_bswap32(w2); }
    return true;
}

}  // namespace resized
}  // namespace jpezy_dev
