// jpezy_kernels_region.hip -- decode of WINDOWS of pictures, full size or reduced (1/2, 1/4, 1/8), for ANY baseline layout the generic pair
// decodes: the region-of-interest decode of one picture (or of a batch of frames of one size) and the batch of crop windows of MANY files,
// each with replicated or with SMOOTH (triangle-filter) chroma.  An output pixel depends only on the MCU that covers it and, smoothed, on a
// ring of one sample around it: the window is DEFINED as the existing (scaled) decode, sliced.  One launch, no
// intermediate in device memory; one workgroup = one MCU that intersects a window.  Four entry kernels find their MCU and run ONE body:
//   region_kernel<N, PIX, ORIENT> : grid = (window MCU columns, window MCU rows, frame)
//   windows_kernel<N, PIX>        : the windows of MANY files in one launch (include/jpezy_hip.h, BATCH OF WINDOWS).  The
//                                   files share a layout and a scale; size, window, destination and quantiser tables are each file's own.
//                                   The grid is 1-D over the sum of the files' window MCUs; a workgroup finds its file by a binary search
//                                   over the files' first-workgroup indices (WindowDesc::wg0) -- the index and every descriptor field depend
//                                   on blockIdx alone, so they are wave-uniform and live in scalar registers.
//   region_smooth_kernel<N, PIX>  : region_kernel's grid  } a component whose replication factor is (2,1), (1,2) or (2,2) is brought to
//   windows_smooth_kernel<N, PIX> : windows_kernel's grid } picture size with the triangle filter of jpezy_kernels_smooth.hip over its
//                                   native plane AT THE REQUESTED SCALE, P_s: the N x N samples of the component's own blocks, N = 8 /
//                                   scale, cut to ceil(Ws / fx) x ceil(Hs / fy) and clamped to bytes (include/jpezy_hip.h, SMOOTH
//                                   UPSAMPLING OF WINDOWS).  Every other component is placed by replication.
// decode_mcu_window<N, PIX, SMOOTH, ORIENT>, the body:
//       stage 1   the N x N low-frequency corner of every block of the MCU is dequantised into LDS (32-bit int) with the file's own
//                 dequantisers, then every thread evaluates samples of it: N*N terms cu*cv * (coef*Q) * cos[u*8/N][x] * cos[v*8/N][y], v
//                 outer, u inner, left to right in FP64 -- scaled_idct_kernel's scheme, with N = 8 as well (there it is the generic pair's
//                 reference-order path, which the fast paths of the full-size kernels are guarded to reproduce) -- and leaves
//                 ref_int(sum / 4 + level) in LDS.  No fast path, no guard band: force_exact / decode_tolerance have nothing to act on, the
//                 fallback counter is not advanced.
//                 SMOOTH: the ring samples of stage 1b are items of the same index range, behind the MCU's own: they fill the waves the
//                 last pass over the own samples leaves idle.
//       stage 1b  SMOOTH only.  Per smoothed component a tile of (H_c*N + 2) x (V_c*N + 2) bytes-as-ints in LDS: the MCU's rectangle of P_s
//                 and a ring of one sample around it.  The tile holds CLAMPED coordinates: position (tx, ty) is P_s at (clamp(bx0 + tx - 1,
//                 0, wc - 1), clamp(by0 + ty - 1, 0, hc - 1)) -- the plane's true extent, which may end inside the MCU --, so stage 2 clamps
//                 nothing.  The coordinate is clamped BEFORE any address is formed; a clamped coordinate inside the MCU's own rectangle is
//                 served from stage 1's samples, any other is one sample evaluated with stage 1's expression from the neighbouring MCU's
//                 coefficient block and the file's own dequantiser.  Ring samples only, never whole neighbour blocks.  wc <= mcu_cols *
//                 H_c * N and hc <= mcu_rows * V_c * N, so no coefficient outside the file's own MCU grid is read.
//       stage 2   the MCU's pixels that lie in the window, four consecutive OUTPUT pixels of a row per thread: block placement and
//                 replication as scaled_rgb_kernel does them (SMOOTH: a smoothed component's value is the integer filter over its tile),
//                 then the pixel-output stage of jpezy_pixel_out.h, stored at (X - x, Y - y).  A group of four that another MCU shares, or
//                 whose address is no multiple of 4, goes out as single bytes.
// With SMOOTH = false stage 1b, the tile and the filter branch are not in the instance, and the workgroup's LDS is the two sample arrays.
// ORIENT, a third property of the body and of the four entry kernels (include/jpezy_hip_orientation.h): the window is one
// of the picture mirrored / rotated / transposed as an EXIF orientation says.  Stages 1 and 1b do not change; stage 2 walks the MCU's
// footprint in the ORIENTED window and reads the same samples through the map.  ORIENT = false instances are the code they were.
// Only the coefficient blocks of MCUs that intersect a window (SMOOTH: and single coefficients' blocks of their neighbours) are read; no byte
// outside a window's w x h output is written.
#include "jpezy_pixel_out.h"
#include "../../include/jpezy_constants.h"

namespace jpezy_dev {
namespace region {

// (external linkage on purpose: a `static` table is reached through the GOT under -fPIC, one more dependent scalar load in front of every
// workgroup's first table read -- measured at 1 % of region_kernel<8> on large windows)
__constant__ double c_cos[64] = JPEZY_COS_INIT;
__constant__ unsigned char c_zzinv[64] = JPEZY_ZZ_INV_INIT;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 48;            // 3 components of at most 4 x 4 blocks
// ints of one component's tile: a smoothed component has at most 4 x 2 or 2 x 4 blocks in an MCU (a factor of 2 along one axis at least)
constexpr int tile_ints(int n) { return (4 * n + 2) * (2 * n + 2); }

// the smoothed components of one picture at the launch's scale: fx == 0: not smoothed (placed by replication)
struct SmoothView {
    int fx[3], fy[3];                     // replication factors
    int wc[3], hc[3];                     // P_s: ceil(Ws / fx) x ceil(Hs / fy)
};
// what a layout alone decides (the batch form: Ws, Hs are each file's own)
struct SmoothFactors {
    int fx[3], fy[3];
};

// The window of one picture as a workgroup sees it: MCU (ux, uy) of the picture at scale 8 / N, the window {x, y, w, h} in that picture's
// coordinates, the MCU's coefficients, the picture's dequantisers [3 comps][64] and the bytes of the window's pixel (0, 0).  For the ring
// of the smooth form: the picture's MCU grid, co0 = the coefficients of its MCU (0, 0).
struct McuView {
    const int16_t* co;
    const int16_t* co0;
    const int* qt;
    unsigned ux, uy, mcu_cols;
    int x, y, w, h;
    uint8_t *out_r, *out_g, *out_b;       // planes: rows w apart; packed: the channel bytes of the first pixel, rows row_stride apart
    size_t row_stride;
    bool blue_first;                      // packed: blue is byte 0 of a pixel
    // ORIENT instances only (include/jpezy_hip_orientation.h): {x, y, w, h} is the SOURCE-side rectangle of the oriented window, and the
    // output pixel of source pixel (sx, sy) is (u, v) -- transposed: (v, u) -- with u = sx - x, mirrored: x + w - 1 - sx, and v likewise
    int orient;                           // kOrientTranspose | kOrientMirrorX | kOrientMirrorY; wave-uniform
};
constexpr int kOrientTranspose = 1, kOrientMirrorX = 2, kOrientMirrorY = 4;

// one sample (x, y) of a block: N*N terms cu*cv * d(v * N + u) * cos[u*8/N][x] * cos[v*8/N][y], v outer, u inner, left to right in FP64
template <int N, class Get>
__device__ __forceinline__ int sample_at(Get d, int x, int y, int level)
{
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
            sum += cu * cv * d(v * N + u) * cx[u] * cy[v];
        }
    }
    return ref_int(sum / 4 + level);
}

// p: the launch's layout constants (RegionDecParams or WindowsParams: the fields both have).  dct, smp: kMaxBlocks * N * N ints of LDS each.
// SMOOTH: sv says which components are smoothed, tile: 3 * tile_ints(N) ints of LDS; neither is looked at otherwise.
// PIX: 0 = planes; 3 / 4 = packed (interleaved) pixels of that many bytes, as in scaled_rgb_kernel.
// ORIENT: stage 2 walks the MCU's footprint in the ORIENTED window (m.orient); false: the instance is the code it was without the property.
template <int N, int PIX, bool SMOOTH, bool ORIENT, class Params>
__device__ __forceinline__ void decode_mcu_window(const Params& p, const McuView& m, const SmoothView& sv, int* dct, int* smp, int* tile)
{
    constexpr int NN = N * N;
    constexpr unsigned l2 = N == 8 ? 3 : N == 4 ? 2 : N == 2 ? 1 : 0;
    [[maybe_unused]] constexpr int kTile = tile_ints(N);
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

    // ---- stage 1 (samples) and stage 1b (the ring) as ONE index range: the MCU's own samples first, then the ring samples of all smoothed
    // components, densely.  A ring sample costs what an own sample costs (one N*N-term sum); in one range the ring fills the waves the last
    // pass over the own samples leaves idle (4:2:0, N = 8: 384 + 72 items are two passes of 256 threads, as 384 alone are) ----
    [[maybe_unused]] auto pick = [](const int (&a)[3], int c) { return c == 0 ? a[0] : c == 1 ? a[1] : a[2]; };
    [[maybe_unused]] auto own = [&](int c, int lx, int ly) {                 // the MCU's own sample (lx, ly) of component c's rectangle
        const int blk = pick(p.blk_start, c) + (ly >> l2) * pick(p.ch, c) + (lx >> l2);
        return smp[(blk << (2 * l2)) + ((ly & (N - 1)) << l2) + (lx & (N - 1))];
    };
    int nring[3] = { 0, 0, 0 };
    if constexpr (SMOOTH) {
#pragma unroll
        for (int c = 0; c < 3; ++c) nring[c] = (sv.fx[c] != 0 && !(c && p.gray)) ? 2 * ((p.ch[c] << l2) + 2) + 2 * (p.cv[c] << l2) : 0;
    }
    const int nall = nsmp + nring[0] + nring[1] + nring[2];
    // ring item r of component c -> its tile position and its CLAMPED plane coordinate relative to the MCU's rectangle; true: the
    // coordinate lies inside the rectangle (the sample is one of stage 1's)
    [[maybe_unused]] auto ring_item = [&](int i, int& c, int& at, int& px, int& py, int& lx, int& ly) {
        c = (i >= nring[0]) + (i >= nring[0] + nring[1]);
        const int r = i - (c > 0 ? nring[0] : 0) - (c > 1 ? nring[1] : 0);
        const int cw = pick(p.ch, c) << l2, chn = pick(p.cv, c) << l2, pitch = cw + 2;
        const int bx0 = (int)ux * cw, by0 = (int)uy * chn;
        int tx, ty;
        if (r < 2 * pitch) {                                  // the row above and the row below, corners included
            ty = r < pitch ? 0 : chn + 1;
            tx = r < pitch ? r : r - pitch;
        } else {                                              // the column left and the column right
            const int q = r - 2 * pitch;
            tx = q < chn ? 0 : cw + 1;
            ty = 1 + (q < chn ? q : q - chn);
        }
        // clamped to the plane before any address is formed
        px = min(max(bx0 + tx - 1, 0), pick(sv.wc, c) - 1);
        py = min(max(by0 + ty - 1, 0), pick(sv.hc, c) - 1);
        lx = px - bx0; ly = py - by0;
        at = c * kTile + ty * pitch + tx;
        return lx >= 0 && lx < cw && ly >= 0 && ly < chn;
    };
    for (int i = threadIdx.x; i < nall; i += kThreads) {
        if (!SMOOTH || i < nsmp) {
            const int k = i / NN, s = i % NN;
            const int* d = dct + k * NN;
            smp[i] = sample_at<N>([d](int j) { return d[j]; }, s % N, s / N, p.level);
            continue;
        }
        if constexpr (SMOOTH) {
            int c, at, px, py, lx, ly;
            if (ring_item(i - nsmp, c, at, px, py, lx, ly)) continue;          // one of the MCU's own: taken below, once they exist
            // px < wc <= mcu_cols * cw and py < hc <= mcu_rows * chn: an MCU of the picture's own grid
            const int cw = pick(p.ch, c) << l2, chn = pick(p.cv, c) << l2;
            const unsigned nux = min((unsigned)px / (unsigned)cw, m.mcu_cols - 1u), nuy = (unsigned)py / (unsigned)chn;
            const unsigned kx = ((unsigned)px - nux * (unsigned)cw) >> l2, ky = ((unsigned)py - nuy * (unsigned)chn) >> l2;
            const size_t blk = ((size_t)nuy * m.mcu_cols + nux) * (size_t)p.blocks_per_mcu + (unsigned)pick(p.blk_start, c) + ky * (unsigned)pick(p.ch, c) + kx;
            const int16_t* nco = m.co0 + blk * 64;
            const int* q = m.qt + c * 64;
            tile[at] = clamp8(sample_at<N>([nco, q](int j) { const int nat = (j / N) * 8 + j % N; return (int)nco[c_zzinv[nat]] * q[nat]; }, px & (N - 1),
                                           py & (N - 1), p.level));
        }
    }
    __syncthreads();

    if constexpr (SMOOTH) {
        // ---- the rest of the tiles from the MCU's own samples, clamped to bytes ----
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (nring[c] == 0) continue;
            // the MCU's rectangle of P_s; the plane may end inside it: the coordinate is clamped, the sample stays one of the MCU's own
            const int cw = p.ch[c] << l2, chn = p.cv[c] << l2, pitch = cw + 2;
            const int bx0 = (int)ux * cw, by0 = (int)uy * chn;
            for (int i = threadIdx.x; i < cw * chn; i += kThreads) {
                const int ty = i / cw, tx = i - ty * cw;
                const int lx = min(bx0 + tx, sv.wc[c] - 1) - bx0, ly = min(by0 + ty, sv.hc[c] - 1) - by0;
                tile[c * kTile + (ty + 1) * pitch + tx + 1] = clamp8(own(c, lx, ly));
            }
        }
        for (int i = threadIdx.x; i < nring[0] + nring[1] + nring[2]; i += kThreads) {      // ring positions whose clamped coordinate is the MCU's own
            int c, at, px, py, lx, ly;
            if (ring_item(i, c, at, px, py, lx, ly)) tile[at] = clamp8(own(c, lx, ly));
        }
        __syncthreads();
    }

    // ---- stage 2: the MCU's pixels inside the window ----
    const int mw = p.hmax << l2, mh = p.vmax << l2;
    const int X0 = max((int)ux * mw, m.x), X1 = min((int)(ux + 1) * mw, m.x + m.w);      // picture coordinates
    const int Y0 = max((int)uy * mh, m.y), Y1 = min((int)(uy + 1) * mh, m.y + m.h);
    if (X1 <= X0 || Y1 <= Y0) return;
    if constexpr (ORIENT) {
        // The footprint of the MCU's source pixels [X0, X1) x [Y0, Y1) in the oriented window: columns [c_lo, c_hi), rows [r_lo, r_hi) of
        // the output -- a rectangle of mh x mw pixels at most when transposed.  A thread owns four consecutive pixels of an OUTPUT row and
        // maps each back to its source (ix, iy) in the MCU; what the un-oriented form precomputes per row is per pixel here.
        const bool tr = (m.orient & kOrientTranspose) != 0, fx = (m.orient & kOrientMirrorX) != 0, fy = (m.orient & kOrientMirrorY) != 0;
        const int u_lo = fx ? m.x + m.w - X1 : X0 - m.x, u_hi = fx ? m.x + m.w - X0 : X1 - m.x;
        const int v_lo = fy ? m.y + m.h - Y1 : Y0 - m.y, v_hi = fy ? m.y + m.h - Y0 : Y1 - m.y;
        const int c_lo = tr ? v_lo : u_lo, c_hi = tr ? v_hi : u_hi, r_lo = tr ? u_lo : v_lo, r_hi = tr ? u_hi : v_hi;
        const int out_w = tr ? m.h : m.w;                                               // planes: rows are the oriented window's width apart
        const int g0 = c_lo >> 2, ng = ((c_hi - 1) >> 2) - g0 + 1, nitems = ng * (r_hi - r_lo);
        const int sx_org = (fx ? m.x + m.w - 1 : m.x) - (int)ux * mw, sy_org = (fy ? m.y + m.h - 1 : m.y) - (int)uy * mh;   // (ix, iy) of u = 0, v = 0
        for (int i = threadIdx.x; i < nitems; i += kThreads) {
            const int gy = i / ng, gx = i - gy * ng;
            const int oy = r_lo + gy;
            const int ox0 = max((g0 + gx) * 4, c_lo), ox1 = min((g0 + gx) * 4 + 4, c_hi);
            const unsigned npx = (unsigned)(ox1 - ox0);
            uint32_t rw = 0, gw = 0, bw = 0;
            for (unsigned j = 0; j < npx; ++j) {
                const int ox = ox0 + (int)j;
                const int u = tr ? oy : ox, v = tr ? ox : oy;
                const unsigned ix = (unsigned)(fx ? sx_org - u : sx_org + u), iy = (unsigned)(fy ? sy_org - v : sy_org + v);    // inside the MCU
                int sv3[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    sv3[c] = c ? 0x80 : 0;                                             // ref :104-105
                    if constexpr (SMOOTH) {
                        if (sv.fx[c] != 0) {
                            if (c && p.gray) continue;
                            const bool h2 = sv.fx[c] == 2, v2 = sv.fy[c] == 2, odd = (ix & 1u) != 0, oddy = (iy & 1u) != 0;
                            const int pitch = (p.ch[c] << l2) + 2;
                            const int ti = h2 ? (int)(ix >> 1) + 1 : (int)ix + 1, tn = h2 ? (odd ? ti + 1 : ti - 1) : ti;
                            const int tj = v2 ? (int)(iy >> 1) + 1 : (int)iy + 1;
                            const int trw = c * kTile + tj * pitch, trn = v2 ? trw + (oddy ? pitch : -pitch) : trw;
                            const int a = tile[trw + ti];
                            if (h2 && v2) {
                                const int Si = 3 * a + tile[trn + ti], Sn = 3 * tile[trw + tn] + tile[trn + tn];
                                sv3[c] = (3 * Si + Sn + (odd ? 7 : 8)) >> 4;
                            } else if (h2) {
                                sv3[c] = (3 * a + tile[trw + tn] + (odd ? 2 : 1)) >> 2;
                            } else {
                                sv3[c] = (3 * a + tile[trn + ti] + (oddy ? 2 : 1)) >> 2;
                            }
                            continue;
                        }
                    }
                    // decode_mcu's placement (ref :504-528), as below, for this pixel's own row
                    const unsigned cvv = (unsigned)p.cv[c], dupy = (unsigned)p.vmax / cvv;
                    const unsigned ky = min(cvv - 1u, iy >> l2), yu = iy - (ky << l2);
                    if (!(c < p.ncomp && yu < (dupy << l2))) continue;
                    const unsigned chh = (unsigned)p.ch[c], dupx = (unsigned)p.hmax / chh;
                    const unsigned kx = min(chh - 1u, ix >> l2), xu = ix - (kx << l2);
                    if (xu < (dupx << l2))
                        sv3[c] = smp[(((unsigned)p.blk_start[c] + ky * chh + kx) << (2 * l2)) + ((yu / dupy) << l2) + xu / dupx];
                }
                uint32_t r, g, b;
                make_rgb(p.gray, sv3[0], sv3[1], sv3[2], r, g, b);                     // ref :531-578, 672-676
                rw |= r << (8 * j); gw |= g << (8 * j); bw |= b << (8 * j);
            }
            if constexpr (PIX != 0) {
                uint8_t* px = (m.blue_first ? m.out_b : m.out_r) + (size_t)(unsigned)oy * m.row_stride + (size_t)(unsigned)ox0 * PIX;
                store_packed4<PIX>(px, npx, m.blue_first ? bw : rw, gw, m.blue_first ? rw : bw);
            } else {
                const size_t off = (size_t)(unsigned)oy * (unsigned)out_w + (unsigned)ox0;
                store_planes4(m.out_r, m.out_g, m.out_b, off, npx, rw, gw, bw, planes_word_aligned(m.out_r, m.out_g, m.out_b, off));
            }
        }
        return;
    }
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
        // a smoothed component: the tile rows of this output row -- its own sample row and, fy == 2, the nearer neighbour (above for an
        // even row, below for an odd one); mh is even then, so iy has Y's parity
        [[maybe_unused]] int trow[3], trown[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned cvv = (unsigned)p.cv[c], dupy = (unsigned)p.vmax / cvv;
            const unsigned ky = min(cvv - 1u, iy >> l2), yu = iy - (ky << l2);          // last block row written over iy
            rowok[c] = c < p.ncomp && yu < (dupy << l2);
            rowblk[c] = (unsigned)p.blk_start[c] + ky * (unsigned)p.ch[c];
            rowsmp[c] = (yu / dupy) << l2;
            if constexpr (SMOOTH) {
                const int pitch = (p.ch[c] << l2) + 2;
                const int tj = sv.fy[c] == 2 ? (int)(iy >> 1) + 1 : (int)iy + 1;
                trow[c] = c * kTile + tj * pitch;
                trown[c] = sv.fy[c] == 2 ? trow[c] + ((iy & 1u) ? pitch : -pitch) : trow[c];
            }
        }
        uint32_t rw = 0, gw = 0, bw = 0;
        for (unsigned j = 0; j < npx; ++j) {
            const unsigned ix = (unsigned)(m.x + ox0 - (int)ux * mw) + j;
            int sv3[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sv3[c] = c ? 0x80 : 0;                                                 // ref :104-105
                if constexpr (SMOOTH) {
                    if (sv.fx[c] != 0) {
                        if (c && p.gray) continue;                                     // gray: chroma is not looked at
                        // the triangle filter (libjpeg's h2v1 / h1v2 / h2v2 fancy upsamplers) over the tile; mw is even with fx == 2
                        const bool h2 = sv.fx[c] == 2, v2 = sv.fy[c] == 2, odd = (ix & 1u) != 0;
                        const int ti = h2 ? (int)(ix >> 1) + 1 : (int)ix + 1, tn = h2 ? (odd ? ti + 1 : ti - 1) : ti;
                        const int a = tile[trow[c] + ti];
                        if (h2 && v2) {
                            const int Si = 3 * a + tile[trown[c] + ti], Sn = 3 * tile[trow[c] + tn] + tile[trown[c] + tn];
                            sv3[c] = (3 * Si + Sn + (odd ? 7 : 8)) >> 4;
                        } else if (h2) {
                            sv3[c] = (3 * a + tile[trow[c] + tn] + (odd ? 2 : 1)) >> 2;
                        } else {
                            sv3[c] = (3 * a + tile[trown[c] + ti] + ((iy & 1u) ? 2 : 1)) >> 2;
                        }
                        continue;
                    }
                }
                if (!rowok[c]) continue;
                const unsigned chh = (unsigned)p.ch[c], dupx = (unsigned)p.hmax / chh;
                const unsigned kx = min(chh - 1u, ix >> l2), xu = ix - (kx << l2);
                if (xu < (dupx << l2)) sv3[c] = smp[((rowblk[c] + kx) << (2 * l2)) + rowsmp[c] + xu / dupx];
            }
            uint32_t r, g, b;
            make_rgb(p.gray, sv3[0], sv3[1], sv3[2], r, g, b);                         // ref :531-578, 672-676
            rw |= r << (8 * j); gw |= g << (8 * j); bw |= b << (8 * j);
        }
        if constexpr (PIX != 0) {
            uint8_t* px = (m.blue_first ? out_b : out_r) + (size_t)oy * m.row_stride + (size_t)ox0 * PIX;
            store_packed4<PIX>(px, npx, m.blue_first ? bw : rw, gw, m.blue_first ? rw : bw);
        } else {
            // planes: rows are w apart and frames plane_stride, neither need be a multiple of 4 -- the word store goes by the addresses
            const size_t off = (size_t)oy * (unsigned)m.w + (unsigned)ox0;
            store_planes4(out_r, out_g, out_b, off, npx, rw, gw, bw, planes_word_aligned(out_r, out_g, out_b, off));
        }
    }
}

// ---- the MCU of a workgroup ----

// region form: MCU (ux0 + blockIdx.x, uy0 + blockIdx.y) of frame blockIdx.z; r, g, b: the channel bytes of pixel (0, 0)
template <bool ORIENT>
__device__ __forceinline__ McuView region_view(const RegionDecParams& p)
{
    const unsigned ux = (unsigned)p.ux0 + blockIdx.x, uy = (unsigned)p.uy0 + blockIdx.y;
    const size_t f = blockIdx.z;
    const int16_t* co0 = p.coeffs + f * (size_t)p.mcu_rows * (size_t)p.mcu_cols * (size_t)p.blocks_per_mcu * 64;
    const size_t mcu = (size_t)uy * (size_t)p.mcu_cols + ux;
    return { co0 + mcu * (size_t)p.blocks_per_mcu * 64, co0, p.qt, ux, uy, (unsigned)p.mcu_cols, p.x, p.y, p.w, p.h,
             p.r + f * p.plane_stride, p.g + f * p.plane_stride, p.b + f * p.plane_stride, p.row_stride, p.b < p.r, ORIENT ? p.orient : 0 };
}

// batch form: workgroup wg of the call is MCU wg - wg0 of file d's window, row by row
template <bool ORIENT>
__device__ __forceinline__ McuView windows_view(const WindowsParams& p, const WindowDesc& d, unsigned wg)
{
    const unsigned local = wg - d.wg0, ucols = (unsigned)d.ucols;
    const unsigned row = local / ucols, col = local - row * ucols;
    const unsigned ux = (unsigned)d.ux0 + col, uy = (unsigned)d.uy0 + row;
    const size_t mcu = (size_t)uy * (size_t)d.mcu_cols + ux;
    uint8_t* const px0 = p.pix + d.out_off;
    const int16_t* co0 = p.coeffs + d.coeff_off;
    // ORIENT: the file's three bits ride in the spare high bits of qset (WindowDesc); the un-oriented instances read the field as it is
    const int qset = ORIENT ? (d.qset & kWindowQsetMask) : d.qset;
    return { co0 + mcu * (size_t)p.blocks_per_mcu * 64, co0, p.qsets + (size_t)qset * 192, ux, uy, (unsigned)d.mcu_cols, d.x, d.y, d.w, d.h,
             px0 + (p.swap_rb ? 2 : 0), px0 + 1, px0 + (p.swap_rb ? 0 : 2), p.row_stride, p.swap_rb != 0,
             ORIENT ? (int)((unsigned)d.qset >> kWindowOrientShift) : 0 };
}

template <int N, int PIX, bool ORIENT>
__global__ __launch_bounds__(kThreads) void region_kernel(RegionDecParams p)
{
    constexpr int NN = N * N;
    __shared__ int dct[kMaxBlocks * NN];          // dequantised corner of every block, [block][v * N + u]
    __shared__ int smp[kMaxBlocks * NN];          // samples, [block][y * N + x]
    decode_mcu_window<N, PIX, false, ORIENT>(p, region_view<ORIENT>(p), SmoothView{}, dct, smp, nullptr);
}

template <int N, int PIX, bool ORIENT>
__global__ __launch_bounds__(kThreads) void region_smooth_kernel(RegionDecParams p, SmoothView sv)
{
    constexpr int NN = N * N;
    __shared__ int dct[kMaxBlocks * NN];
    __shared__ int smp[kMaxBlocks * NN];
    __shared__ int tile[3 * tile_ints(N)];        // per smoothed component: its rectangle of P_s and the ring, clamped to bytes
    decode_mcu_window<N, PIX, true, ORIENT>(p, region_view<ORIENT>(p), sv, dct, smp, tile);
}

// PIX: 3 / 4 only -- the batch has no plane form, and no <N, 0> instance exists
template <int N, int PIX, bool ORIENT>
__global__ __launch_bounds__(kThreads) void windows_kernel(WindowsParams p)
{
    constexpr int NN = N * N;
    __shared__ int dct[kMaxBlocks * NN];
    __shared__ int smp[kMaxBlocks * NN];
    const unsigned wg = p.wg_base + blockIdx.x;
    // (uniform by construction; readfirstlane tells the compiler so, and the descriptor is then read with scalar loads)
    const unsigned fi = (unsigned)__builtin_amdgcn_readfirstlane((int)find_file(p.desc, p.n_desc, wg));
    const WindowDesc d = p.desc[fi];
    decode_mcu_window<N, PIX, false, ORIENT>(p, windows_view<ORIENT>(p, d, wg), SmoothView{}, dct, smp, nullptr);
}

// WindowDesc::pad = { Ws, Hs } of the file at the launch's scale (windows_kernel does not read them)
template <int N, int PIX, bool ORIENT>
__global__ __launch_bounds__(kThreads) void windows_smooth_kernel(WindowsParams p, SmoothFactors sf)
{
    constexpr int NN = N * N;
    __shared__ int dct[kMaxBlocks * NN];
    __shared__ int smp[kMaxBlocks * NN];
    __shared__ int tile[3 * tile_ints(N)];
    const unsigned wg = p.wg_base + blockIdx.x;
    const unsigned fi = (unsigned)__builtin_amdgcn_readfirstlane((int)find_file(p.desc, p.n_desc, wg));       // scalar, as in windows_kernel
    const WindowDesc d = p.desc[fi];
    SmoothView sv;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        sv.fx[c] = sf.fx[c]; sv.fy[c] = sf.fy[c];
        sv.wc[c] = sf.fx[c] ? ((int)d.pad[0] + sf.fx[c] - 1) / sf.fx[c] : 1;
        sv.hc[c] = sf.fx[c] ? ((int)d.pad[1] + sf.fy[c] - 1) / sf.fy[c] : 1;
    }
    decode_mcu_window<N, PIX, true, ORIENT>(p, windows_view<ORIENT>(p, d, wg), sv, dct, smp, tile);
}

// ---- launchers ----

// which components the layout smooths (DESIGN.md 4.13's rule); false: a smoothed component's tile would not fit (no legal layout)
template <class Params>
bool smooth_factors(const Params& p, SmoothFactors* sf)
{
    const int n = 1 << p.log2n;
    for (int c = 0; c < 3; ++c) {
        sf->fx[c] = sf->fy[c] = 0;
        if (c >= p.ncomp || p.ch[c] < 1 || p.cv[c] < 1 || p.hmax % p.ch[c] || p.vmax % p.cv[c]) continue;
        const int fx = p.hmax / p.ch[c], fy = p.vmax / p.cv[c];
        if (!((fx == 2 && fy == 1) || (fx == 1 && fy == 2) || (fx == 2 && fy == 2))) continue;
        if ((p.ch[c] * n + 2) * (p.cv[c] * n + 2) > tile_ints(n)) return false;
        sf->fx[c] = fx; sf->fy[c] = fy;
    }
    return true;
}

// q.orient != 0: the ORIENT instances; the un-oriented ones are launched exactly as they were
template <int N, int PIX>
void launch_region_pix(const RegionDecParams& q, const SmoothView* sv, const dim3& grid, hipStream_t s)
{
    if (q.orient) {
        if (sv) hipLaunchKernelGGL((region_smooth_kernel<N, PIX, true>), grid, dim3(kThreads), 0, s, q, *sv);
        else hipLaunchKernelGGL((region_kernel<N, PIX, true>), grid, dim3(kThreads), 0, s, q);
    } else if (sv) hipLaunchKernelGGL((region_smooth_kernel<N, PIX, false>), grid, dim3(kThreads), 0, s, q, *sv);
    else hipLaunchKernelGGL((region_kernel<N, PIX, false>), grid, dim3(kThreads), 0, s, q);
}

template <int N>
void launch_region(const RegionDecParams& q, const SmoothView* sv, const dim3& grid, hipStream_t s)
{
    if (q.pix_bytes == 3) launch_region_pix<N, 3>(q, sv, grid, s);
    else if (q.pix_bytes == 4) launch_region_pix<N, 4>(q, sv, grid, s);
    else launch_region_pix<N, 0>(q, sv, grid, s);
}

template <int N, int PIX, bool ORIENT>
void launch_windows_pix(const WindowsParams& q, const SmoothFactors* sf, unsigned n_wg, hipStream_t s)
{
    if (sf) hipLaunchKernelGGL((windows_smooth_kernel<N, PIX, ORIENT>), dim3(n_wg), dim3(kThreads), 0, s, q, *sf);
    else hipLaunchKernelGGL((windows_kernel<N, PIX, ORIENT>), dim3(n_wg), dim3(kThreads), 0, s, q);
}

template <int N>
void launch_windows(const WindowsParams& q, const SmoothFactors* sf, unsigned n_wg, hipStream_t s, bool oriented)
{
    if (oriented) {
        if (q.pix_bytes == 3) launch_windows_pix<N, 3, true>(q, sf, n_wg, s);
        else launch_windows_pix<N, 4, true>(q, sf, n_wg, s);
    } else if (q.pix_bytes == 3) launch_windows_pix<N, 3, false>(q, sf, n_wg, s);
    else launch_windows_pix<N, 4, false>(q, sf, n_wg, s);
}

// sv: null = replicated chroma.  The frame index is grid.z: batches above 65,535 frames go out as several launches.
hipError_t launch_region_frames(const RegionDecParams& p, const SmoothView* sv, hipStream_t s)
{
    const int nfr = p.n_frames < 1 ? 1 : p.n_frames;
    const size_t fcoef = (size_t)p.mcu_cols * p.mcu_rows * p.blocks_per_mcu * 64;
    constexpr int per = 65535;
    for (int f0 = 0; f0 < nfr; f0 += per) {
        RegionDecParams q = p;
        q.n_frames = nfr - f0 < per ? nfr - f0 : per;
        q.coeffs += (size_t)f0 * fcoef;
        q.r += (size_t)f0 * p.plane_stride; q.g += (size_t)f0 * p.plane_stride; q.b += (size_t)f0 * p.plane_stride;
        const dim3 grid((unsigned)p.ucols, (unsigned)p.urows, (unsigned)q.n_frames);
        if (p.log2n == 3) launch_region<8>(q, sv, grid, s);
        else if (p.log2n == 2) launch_region<4>(q, sv, grid, s);
        else if (p.log2n == 1) launch_region<2>(q, sv, grid, s);
        else launch_region<1>(q, sv, grid, s);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// sf: null = replicated chroma.  total_wg: the workgroups of the call, desc[k].wg0 counted from 0.  A launch takes at most 2^24 - 1 of them
// -- far below 2^31, and its global size (workgroups x 256 threads) stays below 2^32 --, larger calls go out as several launches that start
// at wg_base.
hipError_t launch_windows_workgroups(const WindowsParams& p, const SmoothFactors* sf, unsigned long long total_wg, hipStream_t s, bool oriented)
{
    constexpr unsigned long long per = (1ull << 24) - 1;
    for (unsigned long long w0 = 0; w0 < total_wg; w0 += per) {
        WindowsParams q = p;
        q.wg_base = (unsigned)w0;
        const unsigned n_wg = (unsigned)(total_wg - w0 < per ? total_wg - w0 : per);
        if (p.log2n == 3) launch_windows<8>(q, sf, n_wg, s, oriented);
        else if (p.log2n == 2) launch_windows<4>(q, sf, n_wg, s, oriented);
        else if (p.log2n == 1) launch_windows<2>(q, sf, n_wg, s, oriented);
        else launch_windows<1>(q, sf, n_wg, s, oriented);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace region

hipError_t launch_dequant_idct_region(const RegionDecParams& p, hipStream_t s)
{
    if (p.log2n < 0 || p.log2n > 3 || p.blocks_per_mcu < 1 || p.blocks_per_mcu > region::kMaxBlocks) return hipErrorInvalidValue;
    if (p.ucols < 1 || p.urows < 1 || p.urows > 65535) return hipErrorInvalidValue;
    return region::launch_region_frames(p, nullptr, s);
}

// launch_dequant_idct_region's checks and frame loop; Ws x Hs: the picture at the launch's scale
hipError_t launch_dequant_idct_region_smooth(const RegionDecParams& p, int Ws, int Hs, hipStream_t s)
{
    if (p.log2n < 0 || p.log2n > 3 || p.blocks_per_mcu < 1 || p.blocks_per_mcu > region::kMaxBlocks) return hipErrorInvalidValue;
    if (p.ucols < 1 || p.urows < 1 || p.urows > 65535 || Ws < 1 || Hs < 1) return hipErrorInvalidValue;
    // the window's MCUs and the plane extents must lie in the picture's own MCU grid: the ring reads by them
    const int mw = p.hmax << p.log2n, mh = p.vmax << p.log2n;
    if (p.ux0 < 0 || p.uy0 < 0 || p.ux0 + p.ucols > p.mcu_cols || p.uy0 + p.urows > p.mcu_rows) return hipErrorInvalidValue;
    if (Ws > p.mcu_cols * mw || Hs > p.mcu_rows * mh || p.x + p.w > Ws || p.y + p.h > Hs) return hipErrorInvalidValue;
    region::SmoothFactors sf;
    if (!region::smooth_factors(p, &sf)) return hipErrorInvalidValue;
    region::SmoothView sv;
    for (int c = 0; c < 3; ++c) {
        sv.fx[c] = sf.fx[c]; sv.fy[c] = sf.fy[c];
        sv.wc[c] = sf.fx[c] ? (Ws + sf.fx[c] - 1) / sf.fx[c] : 1;
        sv.hc[c] = sf.fx[c] ? (Hs + sf.fy[c] - 1) / sf.fy[c] : 1;
    }
    return region::launch_region_frames(p, &sv, s);
}

hipError_t launch_dequant_idct_windows(const WindowsParams& p, unsigned long long total_wg, hipStream_t s, bool oriented)
{
    if (p.log2n < 0 || p.log2n > 3 || p.blocks_per_mcu < 1 || p.blocks_per_mcu > region::kMaxBlocks) return hipErrorInvalidValue;
    if ((p.pix_bytes != 3 && p.pix_bytes != 4) || p.n_desc < 1 || total_wg < 1 || total_wg > 0xFFFFFFFFull) return hipErrorInvalidValue;
    return region::launch_windows_workgroups(p, nullptr, total_wg, s, oriented);
}

// launch_dequant_idct_windows' checks and launch loop; every descriptor carries its file's Ws, Hs in pad[0], pad[1] (the caller's to set and
// to keep inside the file's MCU grid)
hipError_t launch_dequant_idct_windows_smooth(const WindowsParams& p, unsigned long long total_wg, hipStream_t s, bool oriented)
{
    if (p.log2n < 0 || p.log2n > 3 || p.blocks_per_mcu < 1 || p.blocks_per_mcu > region::kMaxBlocks) return hipErrorInvalidValue;
    if ((p.pix_bytes != 3 && p.pix_bytes != 4) || p.n_desc < 1 || total_wg < 1 || total_wg > 0xFFFFFFFFull) return hipErrorInvalidValue;
    region::SmoothFactors sf;
    if (!region::smooth_factors(p, &sf)) return hipErrorInvalidValue;
    return region::launch_windows_workgroups(p, &sf, total_wg, s, oriented);
}

}  // namespace jpezy_dev
