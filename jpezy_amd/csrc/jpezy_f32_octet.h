// jpezy_f32_octet.h -- the f32 encode kernel body for the samplings whose MCU is one block high (4:4:4, 4:2:2), instantiated by
// jpezy_kernels_f32_444.hip and jpezy_kernels_f32_422.hip.  The arithmetic is the quad kernel's (jpezy_f32_quad.h): fdct8p, luma8,
// chroma_px2 / chroma_px_ref, lds_column, quant_block_column, resolve_coef, block_column_f64, the DC paths and the three precision
// levels with their guard bands are CALLED from there, not restated -- the F32Column records and delta1 are per (table, block column)
// and do not know the sampling (a chroma sample has the same range either way).  What is this file's own: the work unit, the LDS
// geometry, the load step, the pass over one kind of block, the store and the launcher.
//
// Work unit: an OCTET of 8 horizontally adjacent MCUs per wave, lane = 8 * row + MCU (row 0..7).  A sampling describes its MCU in a
// unit struct U:
//     BPM    blocks per MCU, LUMA of them luma; block b of an MCU is of table b >= LUMA
//     NW     pixel words per lane and channel: the MCU is 4 NW pixels wide, a lane holds 4 NW bytes of each plane
//     WAVES  waves per SIMD the register allocation aims at (the kernel's launch bound)
//     load_packed<PIX>(src, swap_rb, R, G, B)    4 NW packed pixels (PIX bytes each) -> NW words per channel
//     samples<COMP>(R, G, B, S)                  the lane's 8 samples of pass COMP into S[COMP], A[k] = (s[k], s[7-k]) as fdct8p takes them
// (a unit whose input is not RGB pixels has OWN_SOURCE and load<ALIGNED>(..) in load_packed's place: the source hook, OwnSource below).
// A wave makes BPM passes, each over the eight blocks of one kind: the lane's 8 samples -> row pass -> transpose tile -> column pass ->
// quantiser -> staged block; then the queued coefficients, then BPM whole-line stores per lane: 8 BPM blocks, 1 KB x BPM of contiguous
// output per wave.  The integer samples of all passes stay in registers (8 BPM) for levels 2 and 3, as YL / YR / CS do in the quad.
//
// LDS per wave: transpose tile 8 MCUs x 68 dwords (rows 8 dwords apart; 68 == 4 mod 32: the column reads of a 32-lane group -- 8 MCUs x
// 4 adjacent columns -- hit banks 4 m + c, all different; a row's two 16-byte writes over 8 lanes cover 32 banks once) = 2176 bytes, one
// pass at a time; behind it the staging area of 8 BPM blocks x STG_BLK; behind that the queue.  4:4:4: 6400 bytes, the quad's; 4:2:2:
// 7552 bytes, 30208 per workgroup: five workgroups, 20 waves, fit the CU's 160 KB -- more than the 12 the register allocation admits.
#pragma once
#include <type_traits>
#include <utility>
#include "jpezy_f32_onequad.h"   // load_packed16

namespace jpezy_dev {
namespace f32 {

constexpr int O_PITCH = 8;
constexpr int O_MCU = 68;
constexpr int O_TILE_BYTES = 8 * O_MCU * 4;                 // 2176
constexpr int OWPB = 4;                                     // waves (octets) per workgroup; they share nothing

template <class U>
struct Octet {
    static constexpr int BLOCKS = 8 * U::BPM;
    static constexpr int STG_BYTES = BLOCKS * STG_BLK;
    static constexpr int WAVE_DWORDS = (O_TILE_BYTES + STG_BYTES) / 4 + JPEZY_QUEUE_DWORDS;
    static constexpr int MCU_COEFFS = U::BPM * 64;
    static_assert(O_TILE_BYTES >= BLOCKS * 64, "the per-lane evaluator keeps the octet's samples as bytes in the tile");
    static_assert(O_TILE_BYTES % 16 == 0 && STG_BLK % 16 == 0, "16-byte reads of the staged blocks");
    static_assert(((BLOCKS - 1) << 6 | 63) < 65536, "a queue entry (block, natural position) fits 16 bits");
};

// 8 packed pixels (24 or 32 bytes, 8-byte / 16-byte aligned) -> two words per channel: load_packed16 (jpezy_f32_onequad.h) with half the
// words and its selectors.  (One template over the word count moves two scalar selects in the 4:2:0 packed kernels; those stay as they are.)
template <int PIX>
__device__ __forceinline__ void load_packed8(const uint8_t* src, bool swap_rb, uint32_t* R, uint32_t* G, uint32_t* B)
{
    if (PIX == 3) {
        const uint32_t a1 = swap_rb ? 0x00000502u : 0x00060300u, a2 = swap_rb ? 0x07040100u : 0x05020100u;   // red
        const uint32_t c1 = swap_rb ? 0x00060300u : 0x00000502u, c2 = swap_rb ? 0x05020100u : 0x07040100u;   // blue
        const uint2* s2 = reinterpret_cast<const uint2*>(src);
        const uint2 v0 = s2[0], v1 = s2[1], v2 = s2[2];
        const uint32_t w[6] = { v0.x, v0.y, v1.x, v1.y, v2.x, v2.y };
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const uint32_t w0 = w[3 * q], w1 = w[3 * q + 1], w2 = w[3 * q + 2];
            R[q] = __builtin_amdgcn_perm(w2, __builtin_amdgcn_perm(w1, w0, a1), a2);
            G[q] = __builtin_amdgcn_perm(w2, __builtin_amdgcn_perm(w1, w0, 0x00070401u), 0x06020100u);
            B[q] = __builtin_amdgcn_perm(w2, __builtin_amdgcn_perm(w1, w0, c1), c2);
        }
    } else {
        const uint32_t a = swap_rb ? 0x07060302u : 0x05040100u, c = swap_rb ? 0x05040100u : 0x07060302u;
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const uint4 v = s4[q];
            const uint32_t u01 = __builtin_amdgcn_perm(v.y, v.x, 0x06020400u), u23 = __builtin_amdgcn_perm(v.w, v.z, 0x06020400u);
            const uint32_t v01 = __builtin_amdgcn_perm(v.y, v.x, 0x00000501u), v23 = __builtin_amdgcn_perm(v.w, v.z, 0x00000501u);
            R[q] = __builtin_amdgcn_perm(u23, u01, a);
            G[q] = __builtin_amdgcn_perm(v23, v01, 0x05040100u);
            B[q] = __builtin_amdgcn_perm(u23, u01, c);
        }
    }
}

// The source hook: a unit whose pixels are not three channels of NW words each (YCbCr 4:2:2 samples, jpezy_kernels_f32_422_ycc.hip) says
// OWN_SOURCE and supplies the load step itself,
//     load<ALIGNED>(p, frame, mcu_x, y, R, G, B)    the lane's row segment of row y (clamped) of MCU mcu_x (clamped) -> what samples<> reads
// and, for the launcher, its family's own alignment rule K::aligned(p).  Every other unit takes the load step below.
template <class U, class = void>
struct OwnSource : std::false_type {};
template <class U>
struct OwnSource<U, std::enable_if_t<U::OWN_SOURCE>> : std::true_type {};

// what a lane keeps from pass to pass
struct OctetLane {
    int m, j;                 // MCU of the octet; natural column of the lane's block column
    bool live, dcf;           // MCU inside the picture; the DC closed form holds for both tables
    float* trow;              // the lane's row of the transpose tile
    const float* tcol;        // the lane's column there
    char* sbase;              // the lane's first staged block; the MCU's others are immediates away
    unsigned* queue;
    const F32Column* lcol;    // luma record of column j; chroma 8 further
    uint32_t zz_lo, zz_hi;
    PkCos kc;
};

// ---- 2-5. one pass: samples, row pass, transpose, column pass, quantise + zig-zag into the staging area ----
template <class U, int COMP, int FORCE, bool DCG>
__device__ __forceinline__ void octet_pass(const EncParams& p, const OctetLane& L, const uint32_t* R, const uint32_t* G, const uint32_t* B,
                                           f2 (*S)[4])
{
    constexpr int t = COMP >= U::LUMA ? 1 : 0;
    const F32Column* rec = L.lcol + 8 * t;
    f2 ks[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) ks[k] = f2{ rec->ks[2 * k], rec->ks[2 * k + 1] };
    const f2 dd = f2{ rec->delta1[0], rec->delta1[1] };
    const float th = rec->th;
    U::template samples<COMP>(R, G, B, S);
    __builtin_amdgcn_sched_barrier(0);   // keep the phases apart, as PHASE_FENCE does in the quad: overlapped they need more registers
    {
        f2 X[4];
        fdct8p(S[COMP], X, L.kc);
        f2* dst = reinterpret_cast<f2*>(L.trow);
        dst[0] = X[0]; dst[1] = X[1]; dst[2] = X[2]; dst[3] = X[3];
    }
    wave_sync();
    __builtin_amdgcn_sched_barrier(0);
    f2 col[4], F[4];
    lds_column<O_PITCH>(L.tcol, col);
    wave_sync();                                                          // tile consumed: the next pass' rows may land
    __builtin_amdgcn_sched_barrier(0);
    fdct8p(col, F, L.kc);
    const int dc = DCG ? 0 : L.dcf ? dc_formula(F[0].x, p.dc_rq[t], p.dc_bias[t]) : dc_lookup(F[0].x, t ? p.dcq_chroma : p.dcq_luma);
    quant_block_column<DCG>(F, ks, dd, th, L.j, dc, p.dc_rq[t], p.dc_bias[t], L.live, L.sbase, L.zz_lo, L.zz_hi, COMP * STG_BLK,
                            L.m * U::BPM + COMP, L.queue, FORCE != 0
#ifdef JPEZY_DUMP_T
                            , nullptr
#endif
    );
    __builtin_amdgcn_sched_barrier(0);   // keep the passes apart: overlapped they need more registers
}

// the passes in order, the pass index a compile-time constant: S is only ever indexed by constants (reached through a run-time index
// behind a function boundary the sample array goes to scratch)
template <class U, int FORCE, bool DCG, int... COMP>
__device__ __forceinline__ void octet_passes(const EncParams& p, const OctetLane& L, const uint32_t* R, const uint32_t* G, const uint32_t* B,
                                             f2 (*S)[4], std::integer_sequence<int, COMP...>)
{
    (octet_pass<U, COMP, FORCE, DCG>(p, L, R, G, B, S), ...);
}

// EncParams as the 4:4:4 / 4:2:2 entry points fill it: mcu_cols / mcu_rows count MCUs of 4 NW x 8 pixels, quads_per_row = OCTETS per
// MCU row, coeffs_per_frame = 64 BPM * mcu_cols * mcu_rows.  lds_all: the workgroup's OWPB x Octet<U>::WAVE_DWORDS dwords.
// ALIGNED: W % (4 NW) == 0, bases and strides multiples of 4 NW (packed: of 16): one load of 4 NW bytes of each plane (PIX == 0) or
// 4 NW contiguous packed pixels separated in registers (PIX == 3 / 4).  !ALIGNED (PIX == 0 only): the byte loop with edge clamping over
// the three channel pointers, pixels p.pix_bytes apart (planes: 1) -- planar and packed input alike; the test hooks' instances
// (FORCE != 0) exist in this form only.
template <class U, bool ALIGNED, int FORCE, bool DCG, int PIX>
__device__ __forceinline__ void encode_octet(const EncParams& p, uint32_t* lds_all)
{
    typedef Octet<U> O;
    constexpr int BPM = U::BPM, NW = U::NW;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int mcu_y = (int)fast_div(blockIdx.x, p.gpr_magic, p.gpr_shift);
    const int gx = (int)blockIdx.x - mcu_y * p.groups_per_row;
    const int oct_x = gx * OWPB + wave;
    if (oct_x >= p.quads_per_row) return;                                 // wave-uniform; the waves never meet at a barrier
    const unsigned qidx = (unsigned)(mcu_y * p.quads_per_row + oct_x);
    const int frame = (int)blockIdx.y;
    uint32_t* lds = lds_all + wave * O::WAVE_DWORDS;
    float* ldsf = reinterpret_cast<float*>(lds);
    char* stage = reinterpret_cast<char*>(lds) + O_TILE_BYTES;
    unsigned* queue = lds + (O_TILE_BYTES + O::STG_BYTES) / 4;            // [0] = count, then 16-bit entries
    const int row = lane >> 3, m = lane & 7;
    const bool live = oct_x * 8 + m < p.mcu_cols;
    const int mcu_x = min(oct_x * 8 + m, p.mcu_cols - 1);                 // a dead MCU slot repeats the row's last MCU and stores nothing
    const int W = p.W, H = p.H;
    const DeviceTables* tab = p.tab;
    if (lane == 0) queue[0] = 0;

    // ---- 1. this lane's row segment of 4 NW pixels ----
    uint32_t R[NW], G[NW], B[NW];
    {
        const int y = min(mcu_y * 8 + row, H - 1);                        // clamped extension to whole MCUs, ref :101
        if constexpr (OwnSource<U>::value) {
            U::template load<ALIGNED>(p, frame, mcu_x, y, R, G, B);
        } else {
            const bool packed = p.pix_bytes != 0;                             // wave-uniform
            // W, H <= 65535 and row_stride * H < 2^32 (the entry points): fits 32 bits
            const unsigned rowoff = (unsigned)y * (PIX != 0 || packed ? p.row_stride : (unsigned)W);
            const size_t fo = (size_t)frame * p.plane_stride;
            if (ALIGNED && PIX != 0) {
                U::template load_packed<PIX>(p.pix + fo + (rowoff + (unsigned)mcu_x * (unsigned)(4 * NW * PIX)), p.swap_rb != 0, R, G, B);
            } else if (ALIGNED) {
                typedef uint32_t words __attribute__((ext_vector_type(NW)));
                const unsigned off = rowoff + (unsigned)mcu_x * (unsigned)(4 * NW);
                const words vr = *reinterpret_cast<const words*>(p.r + fo + off);
                const words vg = *reinterpret_cast<const words*>(p.g + fo + off);
                const words vb = *reinterpret_cast<const words*>(p.b + fo + off);
#pragma unroll
                for (int k = 0; k < NW; ++k) { R[k] = vr[k]; G[k] = vg[k]; B[k] = vb[k]; }
            } else {
                const uint8_t* pr = p.r + fo + rowoff;
                const uint8_t* pg = p.g + fo + rowoff;
                const uint8_t* pb = p.b + fo + rowoff;
                const unsigned step = packed ? (unsigned)p.pix_bytes : 1u;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    uint32_t ar = 0, ag = 0, ab = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const unsigned x = (unsigned)min(mcu_x * (4 * NW) + w * 4 + k, W - 1) * step;   // ref :104
                        ar |= (uint32_t)pr[x] << (8 * k);
                        ag |= (uint32_t)pg[x] << (8 * k);
                        ab |= (uint32_t)pb[x] << (8 * k);
                    }
                    R[w] = ar; G[w] = ag; B[w] = ab;
                }
            }
        }
    }

    OctetLane L;
    L.kc = pk_cos();
    asm volatile("" : "+s"(L.kc.k13), "+s"(L.kc.k37), "+s"(L.kc.k51), "+s"(L.kc.k75), "+s"(L.kc.k26));   // as encode_quad_compute
    // the lane at position cq of a block row handles the natural column j = pair_row(cq) (the row pass stores in pair order)
    const int cq = row, j = (int)((0x75316240u >> (4 * cq)) & 7u);
    L.m = m; L.j = j; L.live = live;
    L.dcf = p.dc_rq[0] != 0.f && p.dc_rq[1] != 0.f;
    L.lcol = &tab->f32col[0][(unsigned)j];
    L.zz_lo = L.lcol->zz_lo; L.zz_hi = L.lcol->zz_hi;
    L.queue = queue;
    L.sbase = stage + (m * BPM) * STG_BLK;
    L.trow = ldsf + m * O_MCU + row * O_PITCH;
    L.tcol = ldsf + m * O_MCU + cq;

    f2 S[BPM][4];
    octet_passes<U, FORCE, DCG>(p, L, R, G, B, S, std::make_integer_sequence<int, BPM>());
    wave_sync();

    // ---- 5b. levels 2 and 3 for the queued coefficients (FORCE 1/2: every coefficient of the octet) ----
    const unsigned nq = queue[0];
    if (FORCE == 3 || (FORCE == 0 && nq > (unsigned)QUEUE_CAP)) {
        // the queue-overflow case of encode_quad_compute: every lane evaluates the 8 BPM coefficients of its BPM block columns in the
        // reference's order from the samples, which go to the dead tile as bytes: block (m, comp) at (BPM m + comp) * 64
        signed char* smp = reinterpret_cast<signed char*>(lds);
#pragma unroll
        for (int comp = 0; comp < BPM; ++comp) {
            uint32_t* d = reinterpret_cast<uint32_t*>(smp + (m * BPM + comp) * 64 + row * 8);
            d[0] = pack4(S[comp], 0); d[1] = pack4(S[comp], 4);
        }
        wave_sync();
#pragma unroll 1
        for (int comp = 0; comp < BPM; ++comp) {
            const int blk = m * BPM + comp;
            block_column_f64(smp + blk * 64, j, tab->qt[comp >= U::LUMA ? 1 : 0], stage + blk * STG_BLK);
        }
        if (lane == 0) atomicAdd(p.fallback_count + (qidx & (COUNTER_SHARDS - 1)), (unsigned long long)(O::BLOCKS * 64));
        wave_sync();
    } else {
        const bool all = FORCE != 0;
        const unsigned total = all ? (unsigned)(O::BLOCKS * 64) : nq;
        if (total) {
            const int valid_mcus = min(8, p.mcu_cols - oct_x * 8);
            unsigned done = 0;
#pragma unroll 1
            for (unsigned e = 0; e < total; ++e) {
                const unsigned code = all ? e : reinterpret_cast<const unsigned short*>(queue + 1)[e];
                const int blk = __builtin_amdgcn_readfirstlane((int)(code >> 6)), nat = __builtin_amdgcn_readfirstlane((int)(code & 63));
                const int em = blk / BPM, comp = blk - em * BPM;
                if (em >= valid_mcus) continue;
                const int ei = nat >> 3, ej = nat & 7, tbl = comp >= U::LUMA ? 1 : 0;
                // the 8 lanes that hold the block's rows: lanes em, em + 8, .., em + 56, row y on lane 8 y + em
                float w[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    // comp == 0 ? S[0] : comp == 1 ? S[1] : .. : S[BPM - 1], every index a constant
                    float v = pick(S[BPM - 1], k);
#pragma unroll
                    for (int c = BPM - 2; c >= 0; --c) v = comp == c ? pick(S[c], k) : v;
                    w[k] = v;
                }
                const int Q = tab->qt[tbl][nat];
                const double qinv = tab->qinv[tbl][nat];
                const int zpos = c_zzinv[nat];
                const int qv = resolve_coef<FORCE, false>(w, m == em, row, em, 8, ei, ej, Q, qinv, nullptr);
                if (lane == 0) *reinterpret_cast<int16_t*>(stage + blk * STG_BLK + 2 * zpos) = (int16_t)qv;
                ++done;
            }
            if (lane == 0 && done) atomicAdd(p.fallback_count + (qidx & (COUNTER_SHARDS - 1)), (unsigned long long)done);
            wave_sync();
        }
    }

    // ---- 6. coalesced store: the octet's blocks are contiguous in the coefficient buffer (8 BPM x 128 bytes), BPM 16-byte chunks per lane
    {
        const int valid_chunks = min(8, p.mcu_cols - oct_x * 8) * BPM * 8;
        int16_t* gbase = p.coeffs + (size_t)frame * p.coeffs_per_frame + ((size_t)mcu_y * p.mcu_cols + (size_t)oct_x * 8) * O::MCU_COEFFS;
        uint4* g4 = reinterpret_cast<uint4*>(gbase);
#pragma unroll
        for (int k = 0; k < BPM; ++k) {
            const int c = k * 64 + lane;
            if (c < valid_chunks) {
                const uint4 v = *reinterpret_cast<const uint4*>(stage + (c >> 3) * STG_BLK + (c & 7) * 16);
                nt_store16(g4 + c, v);
            }
        }
    }
}

}  // namespace f32

// ---- the launcher.  K names a kernel family: K::Unit and K::kernel<ALIGNED, FORCE, DCG, PIX>, the __global__ instance ----
template <class K, bool DCG>
static void octet_dispatch(const EncParams& p, bool al, int force, dim3 grid, hipStream_t s)
{
    const dim3 block(64 * f32::OWPB);
    if (force == 1) hipLaunchKernelGGL((K::template kernel<false, 1, DCG, 0>), grid, block, 0, s, p);
    else if (force == 2) hipLaunchKernelGGL((K::template kernel<false, 2, DCG, 0>), grid, block, 0, s, p);
    else if (force == 3) hipLaunchKernelGGL((K::template kernel<false, 3, DCG, 0>), grid, block, 0, s, p);
    else if (!al) hipLaunchKernelGGL((K::template kernel<false, 0, DCG, 0>), grid, block, 0, s, p);
    else if (p.pix_bytes == 3) hipLaunchKernelGGL((K::template kernel<true, 0, DCG, 3>), grid, block, 0, s, p);
    else if (p.pix_bytes == 4) hipLaunchKernelGGL((K::template kernel<true, 0, DCG, 4>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((K::template kernel<true, 0, DCG, 0>), grid, block, 0, s, p);
}

// planar (p.pix_bytes == 0) and packed (3 / 4) input; force as launch_fdct_quant_f32
template <class K>
static hipError_t launch_octets(const EncParams& p0, int force, hipStream_t stream)
{
    constexpr int MCU_W = 4 * K::Unit::NW;                                // bytes of a plane per lane: the planar loads' alignment
    EncParams p = p0;
    if (p.pix_bytes != 0 && p.pix_bytes != 3 && p.pix_bytes != 4) return hipErrorInvalidValue;
    if (p.n_frames > 65535) return hipErrorInvalidValue;                  // grid.y limit; callers chunk larger batches
    bool al;
    if constexpr (f32::OwnSource<typename K::Unit>::value) al = K::aligned(p);
    else if (p.pix_bytes) al = p.W % MCU_W == 0 && p.row_stride % 16 == 0 && p.plane_stride % 16 == 0 && (uintptr_t)p.pix % 16 == 0;
    else al = p.W % MCU_W == 0 && p.plane_stride % MCU_W == 0 && (((uintptr_t)p.r | (uintptr_t)p.g | (uintptr_t)p.b) % MCU_W == 0);
    p.groups_per_row = (p.quads_per_row + f32::OWPB - 1) / f32::OWPB;
    const long groups = (long)p.mcu_rows * p.groups_per_row;
    if (groups <= 0 || p.n_frames <= 0) return hipSuccess;
    fast_div_setup((unsigned)p.groups_per_row, &p.gpr_magic, &p.gpr_shift);
    const dim3 grid((unsigned)groups, (unsigned)p.n_frames);
    if (p.dc_rq[0] != 0.f && p.dc_rq[1] != 0.f) octet_dispatch<K, true>(p, al, force, grid, stream);
    else octet_dispatch<K, false>(p, al, force, grid, stream);
    return hipGetLastError();
}

}  // namespace jpezy_dev
