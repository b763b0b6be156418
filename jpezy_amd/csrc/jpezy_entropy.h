// jpezy_entropy.h -- GPU Huffman coder + bit packer + byte stuffer (internal; see jpezy_entropy.hip)
#pragma once
#include "jpezy_experiment.h"
#include "jpezy_host_codec.h"   // kMaxBlockBits
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace jpezy_dev {
namespace entropy {

// entry = (code << 8) | length in bits;  dc[t][category 0..11], ac[t][(run << 4) | size]   (t: 0 luma, 1 chroma)
// fast[t][(run << 6) | (v + 32)], run 0..15, v -32..31 (v != 0): the AC code of (run, size(v)) with the value bits already
// appended, (bits << 5) | total length (at most 16 + 6 bits) -- one lookup and one append per coefficient instead of
// category -> code lookup -> sign fix -> two appends (round 3; larger values and runs over 15 keep the general path)
struct alignas(16) CodeTables {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
    uint32_t fast[2][1024];
};

struct Job {
    const int16_t* coeffs;        // device, [frame][mcu][bpm][64] zig-zag
    size_t coeffs_per_frame;      // int16 elements
    const CodeTables* tables;     // device
    size_t tables_stride = 0;     // frame f codes with tables[f * tables_stride]; 0: every frame with tables[0] (the Annex-K image)
    unsigned blocks_per_frame;    // coded blocks: `coded` per MCU (gray: the two chroma blocks are coded as zero blocks)
    int bpm;                      // stored blocks per MCU: 6 colour, 4 gray; 3 for 4:4:4; 4 for 4:2:2
    int n_frames;
    unsigned restart = 0;         // MCUs per restart interval that the DEVICE acts on: 0 for none, and 0 too for an interval that holds
                                  // the whole frame (no marker, no reset: only the header differs, and the host writes that)
    // The MCU as a layout: `coded` blocks per MCU of which the first `luma` are luma blocks, then one block each of Cb and Cr; `bpm` of
    // them are stored.  6 / 4 (bpm 6; gray: bpm 4) is 4:2:0, 3 / 1 (bpm 3) is 4:4:4, 4 / 2 (bpm 4) is 4:2:2.  DC predictors: the first luma block of an MCU predicts
    // from the previous MCU's last luma block, a later luma block from the block before, a chroma block from the same index one MCU back.
    // The kernels take the pair as TEMPLATE parameters (the launchers pick the instance): the 4:2:0 instances divide by constants as
    // they always did.
    int coded = 6, luma = 4;
};

// Worst-case bytes of a coded block, 64 x (16-bit code + 10 value bits): the stride of a block in a tile's stream and the unit of
// the worst-case stream size (stream_stride) that the scratch and the frames of a pass are sized by
constexpr unsigned kMaxBlockBytes = 208;
static_assert((jpezy_host::kMaxBlockBits + 7) / 8 <= kMaxBlockBytes, "a coded block must fit the bytes the coder's scratch gives it");

inline size_t tiles256(size_t n) { return (n + 255) / 256; }

// Tiles of a frame with restart intervals (Job::restart != 0): a tile never straddles an interval.  Every interval starts a tile of
// its own and takes restart_tpi() tiles, all of 256 blocks but its last; the frame's last interval may hold fewer MCUs and so fewer
// tiles.  Tile t: interval t / tpi, blocks [first, first + count) of the frame with first = (t / tpi) * 6 * restart + (t % tpi) * 256.
// (CODED: coded blocks per MCU, Job::coded -- a template parameter where kernels call these)
template <unsigned CODED = 6u>
__host__ __device__ inline unsigned restart_tpi(unsigned restart) { return (restart * CODED + 255u) / 256u; }
template <unsigned CODED = 6u>
__host__ __device__ inline unsigned restart_tile_first(unsigned t, unsigned restart)
{
    const unsigned tpi = restart_tpi<CODED>(restart);
    return (t / tpi) * (restart * CODED) + (t % tpi) * 256u;
}
inline unsigned restart_tpi_of(unsigned restart, unsigned coded) { return coded == 3u ? restart_tpi<3u>(restart) : coded == 4u ? restart_tpi<4u>(restart) : restart_tpi<6u>(restart); }
inline size_t restart_intervals(size_t blocks_per_frame, unsigned restart, unsigned coded = 6u) { return (blocks_per_frame / coded + restart - 1) / restart; }
inline size_t restart_tiles(size_t blocks_per_frame, unsigned restart, unsigned coded = 6u)
{
    const size_t ni = restart_intervals(blocks_per_frame, restart, coded);
    return (ni - 1) * restart_tpi_of(restart, coded) + tiles256(blocks_per_frame - (ni - 1) * restart * coded);
}
// the layouts the kernels are instantiated for
inline bool layout_ok(const Job& job)
{
    return (job.coded == 6 && job.luma == 4 && (job.bpm == 6 || job.bpm == 4)) || (job.coded == 3 && job.luma == 1 && job.bpm == 3) ||
           (job.coded == 4 && job.luma == 2 && job.bpm == 4);
}
// tiles of a frame, either way
inline size_t job_tiles(const Job& job)
{
    return job.restart ? restart_tiles(job.blocks_per_frame, job.restart, (unsigned)job.coded) : tiles256(job.blocks_per_frame);
}

// device-resident form of launch_stuff: whole files (header, stuffed stream, EOI), sizes and per-frame verdicts on the device
struct FilePlan {
    const uint8_t* hdr = nullptr;       // nullptr: streams only (the host adds header and EOI)
    size_t hdr_len = 0;
    const unsigned* latched = nullptr;  // [frames] Scratch::latched (launch_stuff sets it)
    long long* sizes = nullptr;         // [frames] file size, or JPEZY_E_FORMAT (-5) / JPEZY_E_NOSPACE (-6)
    const unsigned long long* markers = nullptr;   // restart intervals: Scratch::markers (launch_stuff sets it); selects the stuffing
                                                   // kernel that places RSTn markers
};

// The device arrays of one pass (job.n_frames frames), scratch_sizes() bytes each.  "tile": the blocks of one coding workgroup, 256 of a
// frame or, with restart intervals, of an interval (restart_tiles); "chunk": 64 bytes of a frame's unstuffed stream, "piece": 256 chunks.
struct Scratch {
    uint32_t* tile_stream;            // [frame][tile] the tile's blocks coded back to back (MSB-first words), room for 256 x kMaxBlockBytes
    uint32_t* tile_total;             // [frame][tile] bits
    unsigned long long* tile_base;    // [frame][tiles + 1] frame-relative bit offsets           } not read when the assembling kernel
    uint32_t* first_tile;             // [frame][ft_stride] the tile a piece's first bit lies in } scans the tile totals itself
    unsigned ft_stride;               // pieces of a stream: u_stride / assemble_piece_bytes()
    unsigned long long* restart_pad;  // [frame][interval] restart intervals: launch_tile_bases' scratch
    unsigned long long* bytes;        // [frame] length of the unstuffed stream
    uint32_t* U;                      // [frame] unstuffed streams, u_stride bytes apart (stream_stride)
    size_t u_stride;
    uint32_t* ff_loc;                 // [frame][chunk] bytes the stuffing pass adds in front of the chunk inside its piece (restart intervals:
                                      //                the top three bits hold the number mod 8 of the chunk's first marker)
    uint32_t* ff_piece;               // [frame][piece] ... and in the whole piece: a prefix sum in two levels whose upper level every
                                      //                stuffing workgroup adds up for itself
    unsigned long long* markers;      // [frame][chunk] restart intervals: bit j = an RSTn marker follows byte j of the chunk
    unsigned* status;                 // [frame] |= 1 for a coefficient outside the code tables; zero before launch_code_tiles
    unsigned* latched;                // [frame] nullptr: status stays as the coder left it, for the host to read.  Otherwise the consumer
                                      //         of the tile totals moves it here (latched[f] = status[f], status[f] = 0) for launch_stuff
};
struct ScratchSizes {
    size_t tile_stream, tile_total, tile_base, first_tile, restart_pad, bytes, U, ff_loc, ff_piece, markers, flags;   // (flags: status, latched)
};
// bytes of every array of Scratch for job (job.n_frames frames); 0 for an array the pass does not use: no offsets and no first-tile
// table when the assembling kernel scans the tile totals itself (frames of at most ASM_SELF_TILES tiles without restart intervals),
// no pads and no markers without restart intervals.  any_tables: as launch_assemble takes it.
ScratchSizes scratch_sizes(const Job& job, bool any_tables);
size_t stream_stride(const Job& job);       // Scratch::u_stride: the worst-case stream of a frame (a pad byte behind every restart interval), in whole pieces
size_t max_pass_frames(const Job& job);     // frames of a pass: worst-case streams of 1 GiB together (at least one frame)

size_t scan_tmp_elems(size_t n);  // uint64 scratch elements launch_scan_u32 needs for n inputs
size_t chunk_bytes();             // granularity of the stuffing pass (64)
size_t assemble_piece_bytes();    // bytes of U one assembling / stuffing workgroup handles (16 KB)

// out[0..n) exclusive prefix sums, out[n] the total
hipError_t launch_scan_u32(const uint32_t* in, unsigned long long* out, size_t n, unsigned long long* tmp, hipStream_t s);

// One pass, all launches on one stream (see jpezy_entropy.hip), each choosing its kernel by job.restart and the self-scan rule:
// 1. every block is coded once into its tile's stream; tile_total; status
hipError_t launch_code_tiles(const Job& job, const Scratch& sc, hipStream_t s);
// 2. tile_base, bytes, first_tile; latches status.  With restart intervals every interval but the last ends on a byte.  Nothing to
//    launch when the assembling kernel scans the tile totals itself: it then publishes bytes and latches status.
hipError_t launch_tile_bases(const Job& job, const Scratch& sc, hipStream_t s);
// 3. U, ff_loc, ff_piece, markers.  With restart intervals the counts are the bytes the stuffing pass ADDS: one per 0xFF byte and two
//    per RSTn marker (a marker belongs to the chunk that holds the last byte of its interval).
//    any_tables: tables other than Annex K's (codes as short as one bit): a wider tile window for large frames
hipError_t launch_assemble(const Job& job, const Scratch& sc, bool any_tables, hipStream_t s);
// 4. the stuffed streams, out_stride apart, or (plan.hdr) whole files with their sizes
hipError_t launch_stuff(const Job& job, const Scratch& sc, uint8_t* out, size_t out_stride, FilePlan plan, hipStream_t s);
// dst[f] = bytes stuffing adds to frame f (the host-delivered form sizes its output buffer from it)
hipError_t launch_ff_frame_totals(const Job& job, const Scratch& sc, unsigned long long* dst, hipStream_t s);

// Symbol statistics for per-image optimised tables (jpezy_huffstat.hip): hist[frame][k][sym] += the number of times the coder
// emits symbol sym from table k (DHT order: 0 YDc, 1 CDc, 2 YAc, 3 CAc) for the frame -- what code_block sees, out-of-range values
// counted as the clamped symbol with status[frame] |= 1.  hist must be zero before the launch (job.tables is not read).
// job.restart: the DC predictors are zero at every interval's start, as the coder has them.
hipError_t launch_symbol_histogram(const Job& job, unsigned long long* hist, unsigned* status, hipStream_t s);
// hist[0 .. n_frames * 4 * 256) = 0 on stream s, by a kernel (a memset node does not survive the replay of a captured graph)
hipError_t launch_zero_histogram(unsigned long long* hist, int n_frames, hipStream_t s);

}  // namespace entropy
}  // namespace jpezy_dev
