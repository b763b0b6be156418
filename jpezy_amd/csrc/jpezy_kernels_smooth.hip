// jpezy_kernels_smooth.hip -- the second stage of the any-layout decode with SMOOTH chroma upsampling (include/jpezy_hip.h, CHROMA
// UPSAMPLING).  The first stage is generic_idct_kernel of jpezy_kernels_generic.hip, unchanged: it leaves the integer
// samples [block][64] in the context's scratch.  smooth_rgb_kernel stands where generic_rgb_kernel stands and differs from it in one
// thing: a component whose replication factor is (2,1), (1,2) or (2,2) is brought to picture size with the triangle filter over its
// native plane (libjpeg's h2v1 / h1v2 / h2v2 "fancy" upsamplers) instead of by replication.  The reference has no such mode
// (decode_mcu replicates, ref decoder/jpezy_decoder.hpp:504-528); the definition is this project's own.  Every other component is
// placed exactly as generic_rgb_kernel places it, and make_rgb / revise_value are the reference's FP64 expressions (ref :531-578,
// 672-676), left to right.
#include "jpezy_pixel_out.h"

namespace jpezy_dev {
namespace smooth {

// what the launcher derives from the layout for the smoothed components
struct SmoothParams {
    int fx[3], fy[3];                                       // replication factors of a smoothed component; fx == 0: not smoothed
    int wc[3], hc[3];                                       // its native plane: ceil(W * H_c / hmax) x ceil(H * V_c / vmax)
    unsigned ch_magic[3], ch_shift[3], cv_magic[3], cv_shift[3];   // fast_div by H_c, V_c
};

// make_rgb / revise_value in the reference's FP64 order (ref :531-578, 672-676) and generic_rgb_kernel's store stage
template <int PIX>
__device__ __forceinline__ void colour_store(const GenericDecParams& p, const int (&smp)[3][4], unsigned x0, unsigned y, unsigned npx)
{
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

constexpr unsigned T_PITCH = 272;      // ints per tile row: (256 / fx) / 4 + 2 groups of four columns, fx = 1 at most -> 264, padded

// One thread: four consecutive pixels of a row, as in generic_rgb_kernel; a workgroup: 256 pixels of four rows.  The workgroup first
// brings its part of every smoothed component's native plane into LDS, with a halo of one sample row above and below (fy == 2) and
// one group of four columns left and right, coordinates clamped to the plane and samples clamped to bytes: every sample row is read
// once, with 16-byte loads, instead of by each of the threads whose pixels depend on it.  A thread then takes, from each of the one
// or two tile rows its output row depends on, the columns its four pixels depend on: with fx == 2 those are i-1 .. i+2, i = x0 / 2
// even (one 8-byte and two 4-byte LDS reads), with fx == 1 the four columns x0 .. x0+3 (one 16-byte read).  Coordinates are
// clamped before a block is looked up, so nothing outside the plane (and so nothing outside the samples scratch) is read.  The form
// in which every thread loaded its samples from global memory took twice the time (docs/rejected_experiments/r16_smooth_direct_loads.patch).
template <int PIX = 0>
__global__ __launch_bounds__(256) void smooth_rgb_kernel(GenericDecParams p, SmoothParams sp)
{
    __shared__ __attribute__((aligned(16))) int tile[3][4][T_PITCH];
    const unsigned x0 = (blockIdx.x * 64u + (threadIdx.x & 63u)) * 4u;
    const unsigned y = blockIdx.y * 4u + (threadIdx.x >> 6);
    const bool active = y < (unsigned)p.H && x0 < (unsigned)p.W;
    {   // batch form: blockIdx.z is the frame
        const size_t f = blockIdx.z;
        p.samples += f * ((size_t)p.mcu_cols * p.mcu_rows * p.blocks_per_mcu * 64);
        p.r += f * p.plane_stride; p.g += f * p.plane_stride; p.b += f * p.plane_stride;
    }
    {
        // ---- the workgroup's part of every smoothed component's native plane, with its halo, clamped to bytes, into LDS ----
        // tile row t: native row cy0 + t, tile column u: native column cx0 + u, both clamped to the plane.  Four rows always: the two
        // sample rows of the workgroup's four pixel rows and one above and below (fy == 2), or its four sample rows (fy == 1).  Columns
        // go in groups of four from four left of the workgroup's first to the group right of its last: one 16-byte load per group
        // where the group lies inside the plane, clamped single loads at the plane's edges.
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= p.ncomp || (c && p.gray) || sp.fx[c] == 0) continue;
            const unsigned chh = (unsigned)p.ch[c], cvv = (unsigned)p.cv[c];
            const int wc = sp.wc[c], hc = sp.hc[c];
            const int cx0 = (int)(blockIdx.x * 256u / (unsigned)sp.fx[c]) - 4;
            const int cy0 = (int)(blockIdx.y * 4u / (unsigned)sp.fy[c]) - (sp.fy[c] == 2 ? 1 : 0);
            const unsigned ngrp = 64u / (unsigned)sp.fx[c] + 2u;                         // 34 or 66
            for (unsigned idx = threadIdx.x; idx < 4u * ngrp; idx += 256u) {
                const unsigned t = (idx >= ngrp) + (idx >= 2u * ngrp) + (idx >= 3u * ngrp), g = idx - t * ngrp;
                const unsigned nr = (unsigned)min(max(cy0 + (int)t, 0), hc - 1);
                const unsigned by = nr >> 3;
                const unsigned my = fast_div(by, sp.cv_magic[c], sp.cv_shift[c]), ky = by - my * cvv;
                const size_t rowbase = ((size_t)my * p.mcu_cols * (size_t)p.blocks_per_mcu + (unsigned)p.blk_start[c] + ky * chh) * 64 + (nr & 7u) * 8u;
                auto at = [&](int col) -> const int* {
                    const unsigned cc = (unsigned)min(max(col, 0), wc - 1), bx = cc >> 3;
                    const unsigned mx = fast_div(bx, sp.ch_magic[c], sp.ch_shift[c]), kx = bx - mx * chh;
                    return p.samples + rowbase + ((size_t)mx * p.blocks_per_mcu + kx) * 64 + (cc & 7u);
                };
                const int nc0 = cx0 + 4 * (int)g;                                        // a multiple of 4: the group lies in one block row
                int4 v;
                if (nc0 >= 0 && nc0 + 3 < wc) v = *reinterpret_cast<const int4*>(at(nc0));
                else v = make_int4(*at(nc0), *at(nc0 + 1), *at(nc0 + 2), *at(nc0 + 3));
                *reinterpret_cast<int4*>(&tile[c][t][4u * g]) = make_int4(clamp8(v.x), clamp8(v.y), clamp8(v.z), clamp8(v.w));
            }
        }
    }
    __syncthreads();
    if (!active) return;
    const unsigned mw = (unsigned)p.hmax * 8u, mh = (unsigned)p.vmax * 8u;
    const unsigned uy = fast_div(y, p.mh_magic, p.mh_shift), iy = y - uy * mh;
    const unsigned ux = fast_div(x0, p.mw_magic, p.mw_shift), ix0 = x0 - ux * mw;   // the four pixels sit in one MCU
    const size_t mcu_blk = ((size_t)uy * p.mcu_cols + ux) * (size_t)p.blocks_per_mcu;
    const unsigned npx = min(4u, (unsigned)p.W - x0);
    int smp[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int init = c ? 0x80 : 0;                                                  // missing components read 0x80 (ref :104-105)
        smp[c][0] = smp[c][1] = smp[c][2] = smp[c][3] = init;
        if (c >= p.ncomp || (c && p.gray)) continue;                                    // gray: chroma is not looked at
        const unsigned chh = (unsigned)p.ch[c], cvv = (unsigned)p.cv[c];
        if (sp.fx[c] == 0) {
            // ---- not smoothed: generic_rgb_kernel's placement (decode_mcu, ref :504-528), the integer sample unclamped ----
            const unsigned dupy = (unsigned)p.vmax / cvv, dupx = (unsigned)p.hmax / chh;
            const unsigned ky = min(cvv - 1u, iy >> 3), yu = iy - ky * 8u;              // last block row written over iy
            if (yu >= 8u * dupy) continue;
            const unsigned rowblk = (unsigned)p.blk_start[c] + ky * chh;
            const unsigned rowsmp = fast_div(yu, p.dy_magic[c], p.dy_shift[c]) * 8u;
            if (chh == (unsigned)p.hmax) {
                const int4 v = *reinterpret_cast<const int4*>(p.samples + (mcu_blk + rowblk + (ix0 >> 3)) * 64 + rowsmp + (ix0 & 7u));
                smp[c][0] = v.x; smp[c][1] = v.y; smp[c][2] = v.z; smp[c][3] = v.w;
            } else if (chh == 1u && dupx == 4u) {
                smp[c][0] = smp[c][1] = smp[c][2] = smp[c][3] = p.samples[(mcu_blk + rowblk) * 64 + rowsmp + (ix0 >> 2)];
            } else {                                    // the other legal factors: the last block written over each pixel
                for (unsigned j = 0; j < 4; ++j) {
                    const unsigned ix = ix0 + j;
                    const unsigned kx = min(chh - 1u, ix >> 3), xu = ix - kx * 8u;
                    if (xu < 8u * dupx) smp[c][j] = p.samples[(mcu_blk + rowblk + kx) * 64 + rowsmp + fast_div(xu, p.dx_magic[c], p.dx_shift[c])];
                }
            }
            continue;
        }
        // ---- smoothed: the triangle filter over the native plane wc x hc, coordinates clamped to it ----
        const bool h2 = sp.fx[c] == 2, v2 = sp.fy[c] == 2;
        // the tile holds clamped coordinates already: rows (ly >> 1) + 1 and its neighbour (above for even y, below for odd y; fy == 2)
        // or ly (fy == 1), columns from four left of the workgroup's first
        const unsigned ly = threadIdx.x >> 6, lx = threadIdx.x & 63u;
        const unsigned t0 = v2 ? (ly >> 1) + 1u : ly, t1 = v2 ? ((ly & 1u) ? t0 + 1u : t0 - 1u) : t0;
        const unsigned tc = (h2 ? lx * 2u : lx * 4u) + 4u;
        int val[2][4];                                                                  // [row][column i-1, i, i+1, i+2]  /  [row][x0 .. x0+3]
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k == 1 && !v2) break;
            const int* trow = tile[c][k ? t1 : t0];
            if (h2) {
                const int2 v = *reinterpret_cast<const int2*>(trow + tc);
                val[k][0] = trow[tc - 1u]; val[k][1] = v.x; val[k][2] = v.y; val[k][3] = trow[tc + 2u];
            } else {
                const int4 v = *reinterpret_cast<const int4*>(trow + tc);
                val[k][0] = v.x; val[k][1] = v.y; val[k][2] = v.z; val[k][3] = v.w;
            }
        }
        if (h2 && v2) {
            int S[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) S[j] = 3 * val[0][j] + val[1][j];
            smp[c][0] = (3 * S[1] + S[0] + 8) >> 4;
            smp[c][1] = (3 * S[1] + S[2] + 7) >> 4;
            smp[c][2] = (3 * S[2] + S[1] + 8) >> 4;
            smp[c][3] = (3 * S[2] + S[3] + 7) >> 4;
        } else if (h2) {
            smp[c][0] = (3 * val[0][1] + val[0][0] + 1) >> 2;
            smp[c][1] = (3 * val[0][1] + val[0][2] + 2) >> 2;
            smp[c][2] = (3 * val[0][2] + val[0][1] + 1) >> 2;
            smp[c][3] = (3 * val[0][2] + val[0][3] + 2) >> 2;
        } else {
            const int rnd = (y & 1u) ? 2 : 1;
#pragma unroll
            for (int j = 0; j < 4; ++j) smp[c][j] = (3 * val[0][j] + val[1][j] + rnd) >> 2;
        }
    }
    colour_store<PIX>(p, smp, x0, y, npx);
}

}  // namespace smooth

// the second stage of launch_dequant_idct_generic for JPEZY_UPSAMPLE_SMOOTH: q is what generic_rgb_kernel would be launched with
hipError_t launch_smooth_rgb(const GenericDecParams& q, dim3 grid, hipStream_t s)
{
    smooth::SmoothParams sp;
    for (int c = 0; c < 3; ++c) {
        sp.fx[c] = sp.fy[c] = 0;
        sp.wc[c] = sp.hc[c] = 1;
        const int ch = c < q.ncomp ? q.ch[c] : 1, cv = c < q.ncomp ? q.cv[c] : 1;
        fast_div_setup((unsigned)ch, &sp.ch_magic[c], &sp.ch_shift[c]);
        fast_div_setup((unsigned)cv, &sp.cv_magic[c], &sp.cv_shift[c]);
        if (c >= q.ncomp || q.hmax % ch || q.vmax % cv) continue;
        const int fx = q.hmax / ch, fy = q.vmax / cv;
        if (!((fx == 2 && fy == 1) || (fx == 1 && fy == 2) || (fx == 2 && fy == 2))) continue;
        sp.fx[c] = fx; sp.fy[c] = fy;
        sp.wc[c] = (int)(((long)q.W * ch + q.hmax - 1) / q.hmax);
        sp.hc[c] = (int)(((long)q.H * cv + q.vmax - 1) / q.vmax);
    }
    if (q.pix_bytes == 3) hipLaunchKernelGGL(smooth::smooth_rgb_kernel<3>, grid, dim3(256), 0, s, q, sp);
    else if (q.pix_bytes == 4) hipLaunchKernelGGL(smooth::smooth_rgb_kernel<4>, grid, dim3(256), 0, s, q, sp);
    else hipLaunchKernelGGL(smooth::smooth_rgb_kernel<0>, grid, dim3(256), 0, s, q, sp);
    return hipGetLastError();
}

}  // namespace jpezy_dev
