// jpezy_kernels_transform.hip -- lossless transforms in the coefficient domain: flip, rotate, transpose of [mcu][block][64] zig-zag int16
// fields (include/jpezy_hip.h, LOSSLESS TRANSFORMS).  Every output coefficient is an input coefficient, possibly negated:
// the kernel is data movement, 2 bytes read and 2 bytes written per coefficient, from one buffer to a DIFFERENT one.
//   transform_kernel<SWAP, B> : eight lanes (an octet) per OUTPUT block, 32 blocks per workgroup, blocks in the order of the output buffer
//       (grid: groups of 32 blocks, frame).  An octet works out its block's place in the output's MCU grid and from it the source block
//       (block grid of the component, axes exchanged, axes mirrored: once per block, the same in its eight lanes), reads the source's 128
//       bytes as eight 16-byte loads, and writes the output's 128 bytes as eight 16-byte non-temporal stores: both sides move whole 128-byte
//       lines, a wave eight of them per instruction.  The output side is one contiguous stream; on the source side consecutive blocks are
//       neighbours (no swap: ascending or, mirrored, descending) or a whole MCU row apart (swap).
//       no swap   the zig-zag position stays: lane j holds coefficients 8j .. 8j+7 and negates those that byte j of the sign mask names.
//       swap      position z' of the output is position perm[z'] of the source (the zig-zag image of v <-> u): the octet parks its block in
//                 LDS (one 16-byte store per lane, slots 144 bytes apart so that the four octets of a 32-lane group start on different
//                 banks) and every lane gathers its eight coefficients as 16-bit reads; only the octet's own lanes -- one wave -- touch a
//                 slot, so no workgroup barrier.  Signs as above.
//   The permutation and the two parity masks (odd u, odd v by zig-zag position) are compile-time tables; an operation's mask is one
//   exclusive-or of them.  The DC is in neither.  Negation is two's complement in 16 bits: -32768 stays -32768.
#include "jpezy_wave.h"
#include "../../include/jpezy_constants.h"

namespace jpezy_dev {
namespace xform {

constexpr int kThreads = 256;
constexpr int kOctets = kThreads / 8;     // blocks per workgroup
constexpr int kSlot = 9;                  // uint4 per LDS slot: 128 bytes of block + 16 of padding

struct Tables {
    unsigned char perm[64];               // zig-zag position of the transposed frequency: (v, u) at z' -> (u, v) at perm[z']
    unsigned long long odd_u, odd_v;      // bit z: the horizontal / vertical frequency at zig-zag position z is odd
};

constexpr Tables make_tables()
{
    constexpr unsigned char zz[64] = JPEZY_ZZ_INIT, zzinv[64] = JPEZY_ZZ_INV_INIT;
    Tables t{};
    for (int z = 0; z < 64; ++z) {
        const int v = zz[z] >> 3, u = zz[z] & 7;
        t.perm[z] = zzinv[u * 8 + v];
        if (u & 1) t.odd_u |= 1ull << z;
        if (v & 1) t.odd_v |= 1ull << z;
    }
    return t;
}
constexpr Tables kTables = make_tables();
static_assert(kTables.perm[0] == 0 && kTables.perm[1] == 2 && kTables.perm[2] == 1 && kTables.perm[63] == 63, "the zig-zag image of the transposition");
static_assert(!(kTables.odd_u & 1) && !(kTables.odd_v & 1) && (kTables.odd_u & 2) && (kTables.odd_v & 4), "the DC never changes sign");

__constant__ Tables c_tables = kTables;

struct Args {
    const int16_t* in;
    int16_t* out;
    size_t in_frame, out_frame;
    unsigned long long neg;               // bit z': output position z' is negated
    unsigned blocks;                      // output blocks per frame
    unsigned out_cols, oc_magic, oc_shift;
    unsigned src_pitch, C, R;
    int mirror_x, mirror_y;
};

// the two int16 of w, each negated (mod 2^16) where its bit of n is set
__device__ __forceinline__ uint32_t negate2(uint32_t w, unsigned n)
{
    uint32_t lo = w & 0xFFFFu, hi = w >> 16;
    if (n & 1u) lo = (0u - lo) & 0xFFFFu;
    if (n & 2u) hi = (0u - hi) & 0xFFFFu;
    return lo | (hi << 16);
}

template <bool SWAP, int B>
__global__ __launch_bounds__(kThreads) void transform_kernel(Args a)
{
    __shared__ uint4 tile[SWAP ? kOctets * kSlot : 1];
    const unsigned j = threadIdx.x & 7u, oct = threadIdx.x >> 3;
    const unsigned ob = blockIdx.x * kOctets + oct;
    if (ob >= a.blocks) return;           // (whole octets leave; the rest of the wave meets no workgroup barrier)
    const size_t f = blockIdx.y;

    // the block's place in the output, then its source: per block, the same in the octet's eight lanes
    const unsigned omcu = ob / B, k = ob - omcu * B;
    const unsigned omy = fast_div(omcu, a.oc_magic, a.oc_shift), omx = omcu - omy * a.out_cols;
    const bool quad = B == 6 && k < 4;    // a luma block of a 2 x 2 MCU: the component's block grid is twice the MCU grid
    const unsigned bx = quad ? 2 * omx + (k & 1u) : omx, by = quad ? 2 * omy + (k >> 1) : omy;
    const unsigned gc = quad ? 2 * a.C : a.C, gr = quad ? 2 * a.R : a.R;
    unsigned sx = SWAP ? by : bx, sy = SWAP ? bx : by;
    if (a.mirror_x) sx = gc - 1 - sx;
    if (a.mirror_y) sy = gr - 1 - sy;
    const size_t smcu = quad ? (size_t)(sy >> 1) * a.src_pitch + (sx >> 1) : (size_t)sy * a.src_pitch + sx;
    const unsigned sk = quad ? 2 * (sy & 1u) + (sx & 1u) : k;

    const uint4* src = reinterpret_cast<const uint4*>(a.in + f * a.in_frame + (smcu * B + sk) * 64);
    uint4* dst = reinterpret_cast<uint4*>(a.out + f * a.out_frame + (size_t)ob * 64);
    uint4 v = src[j];
    if (SWAP) {
        tile[oct * kSlot + j] = v;
        wave_sync();
        const uint16_t* blk = reinterpret_cast<const uint16_t*>(&tile[oct * kSlot]);
        const uint2 pp = reinterpret_cast<const uint2*>(c_tables.perm)[j];
        auto pick = [&](uint32_t idx2) { return (uint32_t)blk[idx2 & 0xFFu] | ((uint32_t)blk[(idx2 >> 8) & 0xFFu] << 16); };
        v.x = pick(pp.x);
        v.y = pick(pp.x >> 16);
        v.z = pick(pp.y);
        v.w = pick(pp.y >> 16);
    }
    const unsigned n = (unsigned)(a.neg >> (8u * j)) & 0xFFu;
    v.x = negate2(v.x, n);
    v.y = negate2(v.y, n >> 2);
    v.z = negate2(v.z, n >> 4);
    v.w = negate2(v.w, n >> 6);
    nt_store16(dst + j, v);
}

}  // namespace xform

hipError_t launch_coeff_transform(const XformParams& p, hipStream_t s)
{
    using namespace xform;
    const int B = p.blocks_per_mcu;
    if ((B != 3 && B != 6) || p.C < 1 || p.R < 1 || p.C > p.src_pitch || p.n_frames < 1 || !p.in || !p.out) return hipErrorInvalidValue;
    const unsigned out_cols = (unsigned)(p.swap ? p.R : p.C), out_rows = (unsigned)(p.swap ? p.C : p.R);
    const unsigned long long blocks = (unsigned long long)out_cols * out_rows * (unsigned)B;
    if (blocks > 0xFFFFFFFFull - kOctets) return hipErrorInvalidValue;
    Args a;
    a.in_frame = p.in_frame;
    a.out_frame = p.out_frame;
    // the source frequency of output (v, u) is (u, v) after a swap: the mirrored source axis then meets the other parity
    a.neg = (p.mirror_x ? (p.swap ? kTables.odd_v : kTables.odd_u) : 0ull) ^ (p.mirror_y ? (p.swap ? kTables.odd_u : kTables.odd_v) : 0ull);
    a.blocks = (unsigned)blocks;
    a.out_cols = out_cols;
    fast_div_setup(out_cols, &a.oc_magic, &a.oc_shift);
    a.src_pitch = (unsigned)p.src_pitch;
    a.C = (unsigned)p.C;
    a.R = (unsigned)p.R;
    a.mirror_x = p.mirror_x;
    a.mirror_y = p.mirror_y;
    const unsigned groups = (a.blocks + kOctets - 1) / kOctets;
    constexpr int kMaxFrames = 65535;         // the frame index is a grid dimension
    for (int f0 = 0; f0 < p.n_frames; f0 += kMaxFrames) {
        const int nf = p.n_frames - f0 < kMaxFrames ? p.n_frames - f0 : kMaxFrames;
        a.in = p.in + (size_t)f0 * p.in_frame;
        a.out = p.out + (size_t)f0 * p.out_frame;
        const dim3 grid(groups, (unsigned)nf);
        if (p.swap) {
            if (B == 6) hipLaunchKernelGGL((transform_kernel<true, 6>), grid, dim3(kThreads), 0, s, a);
            else hipLaunchKernelGGL((transform_kernel<true, 3>), grid, dim3(kThreads), 0, s, a);
        } else {
            if (B == 6) hipLaunchKernelGGL((transform_kernel<false, 6>), grid, dim3(kThreads), 0, s, a);
            else hipLaunchKernelGGL((transform_kernel<false, 3>), grid, dim3(kThreads), 0, s, a);
        }
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace jpezy_dev
