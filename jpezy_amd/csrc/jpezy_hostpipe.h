// jpezy_hostpipe.h -- streaming of the host-buffer entry points (internal; used by jpezy_capi.hip).
//
// jpezy_fdct_quant / jpezy_dequant_idct / jpezy_encode_jpeg take HOST buffers: what encoder::encode and decoder::decode hand
// over (ref encoder/jpezy_encoder.hpp:24-28, 58-67: the planes are std::vectors the object copied at construction, so a caller's
// buffers are fresh for every image).  Round 2 staged the whole batch -- one pageable copy in, the kernel, one copy out, one
// synchronisation: 5.7 ms per 4096x4096 frame around a 0.03 ms kernel, device memory proportional to the batch.
//
// Here a call is cut into chunks of a few MB (MCU-row bands of a large frame, or several small frames) that flow through a ring
// of RING slots, each a pinned host buffer + a device buffer per direction:
//
//   feeder threads   memcpy caller -> pinned slot, hipMemcpyAsync H2D on the upload stream, event
//   calling thread   waits (stream-side) for the upload, launches the kernel on the context's stream, event,
//                    hipMemcpyAsync D2H on the download stream, event
//   drainer threads  wait for the download, memcpy pinned slot -> caller
//
// so that the upload of chunk c + 1, the kernel of chunk c and the download of chunk c - 1 overlap, PCIe runs in both directions
// at once, and the device footprint is the ring, not the batch.  The caller's memory is never handed to the DMA engines: pinning
// fresh pages costs as much as copying them (tools/ubench/host_xfer.cpp: 1.7 ms per 2 x 48 MB registered, 0.6 ms per 48 MB copied
// by four threads), and a library-owned ring behaves the same whether or not the caller reuses its buffers.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "jpezy_owners.h"

namespace jpezy_host {

using jpezy_capi::DevBuf;
using jpezy_capi::PinBuf;
using jpezy_capi::Stream;
using jpezy_capi::Event;
using jpezy_capi::Joiner;

struct Segment {
    void* host;          // caller memory (source for uploads, destination for downloads)
    size_t bytes;
    size_t slot_off;     // offset inside the slot's pinned / device buffer
};

struct ChunkPlan {
    std::vector<Segment> in, out;
};

class HostPipe {
public:
    static constexpr int RING = 4;

    // kernel(c, d_in, d_out, stream): enqueue chunk c's launches on `stream` (inputs at d_in + Segment::slot_off, outputs likewise);
    // returns a hipError_t.  plan(c): the chunk's segments.  Returns hipSuccess or the first error (message in *err).
    hipError_t run(int device, hipStream_t compute, int n_chunks, size_t max_in, size_t max_out,
                   const std::function<ChunkPlan(int)>& plan,
                   const std::function<hipError_t(int, uint8_t*, uint8_t*, hipStream_t)>& kernel, std::string* err)
    {
        if (n_chunks <= 0) return hipSuccess;
        hipError_t e = reserve(max_in, max_out);
        if (e != hipSuccess) { if (err) *err = "host pipeline: allocating the staging ring failed"; return e; }
        std::vector<ChunkPlan> plans((size_t)n_chunks);
        for (int c = 0; c < n_chunks; ++c) plans[(size_t)c] = plan(c);

        if (n_chunks == 1) {
            // a call that fits one chunk (small frames): nothing to overlap -- the plain staged copy on the calling thread,
            // without six thread starts and their event round trips
            uint8_t *d_in = dev_in_[0].as<uint8_t>(), *d_out = dev_out_[0].as<uint8_t>();
            for (const Segment& sg : plans[0].in) std::memcpy(pin_in_[0].p + sg.slot_off, sg.host, sg.bytes);
            for (const Segment& sg : plans[0].in) {
                e = hipMemcpyAsync(d_in + sg.slot_off, pin_in_[0].p + sg.slot_off, sg.bytes, hipMemcpyHostToDevice, compute);
                if (e != hipSuccess) { if (err) *err = "host pipeline: hipMemcpyAsync (upload) failed"; return e; }
            }
            e = kernel(0, d_in, d_out, compute);
            for (const Segment& sg : plans[0].out) {
                if (e != hipSuccess) break;
                e = hipMemcpyAsync(pin_out_[0].p + sg.slot_off, d_out + sg.slot_off, sg.bytes, hipMemcpyDeviceToHost, compute);
            }
            const hipError_t es = hipStreamSynchronize(compute);
            if (e == hipSuccess) e = es;
            if (e != hipSuccess) { if (err) *err = std::string("host pipeline: ") + hipGetErrorString(e); return e; }
            for (const Segment& sg : plans[0].out) std::memcpy(sg.host, pin_out_[0].p + sg.slot_off, sg.bytes);
            return hipSuccess;
        }

        // per-chunk progress: 0 nothing, 1 upload issued, 2 download issued, 3 delivered to the caller
        std::vector<std::atomic<int>> state((size_t)n_chunks);
        for (auto& s : state) s.store(0);
        std::atomic<int> failed{ 0 };
        std::mutex mu;
        std::condition_variable cv;
        auto set_state = [&](int c, int v) { { std::lock_guard<std::mutex> lk(mu); state[(size_t)c].store(v); } cv.notify_all(); };
        auto wait_state = [&](int c, int v) {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return state[(size_t)c].load() >= v || failed.load(); });
            return !failed.load();
        };
        auto fail = [&](hipError_t code, const char* what) {
            int expected = 0;
            if (failed.compare_exchange_strong(expected, (int)code) && err) *err = std::string("host pipeline: ") + what + ": " + hipGetErrorString(code);
            cv.notify_all();
        };

        // three memcpy threads per direction (one core copies ~26 GB/s, PCIe moves ~56 GB/s each way: tools/ubench/host_xfer.cpp)
        const int n_feed = std::min(n_chunks, 3), n_drain = std::min(n_chunks, 3);
        auto feeder = [&](int id) {
            if (hipSetDevice(device) != hipSuccess) { fail(hipErrorInvalidDevice, "hipSetDevice"); return; }
            for (int c = id; c < n_chunks && !failed.load(); c += n_feed) {
                const int slot = c % RING;
                // the slot's input buffers are free once the kernel of the chunk that used them last has run
                if (c >= RING) {
                    if (!wait_state(c - RING, 2)) return;                 // its kernel has been enqueued (the event is recorded)
                    hipError_t e2 = hipEventSynchronize(ev_k_[slot]);
                    if (e2 != hipSuccess) { fail(e2, "hipEventSynchronize"); return; }
                }
                for (const Segment& sg : plans[(size_t)c].in) std::memcpy(pin_in_[slot].p + sg.slot_off, sg.host, sg.bytes);
                {
                    std::lock_guard<std::mutex> lk(up_mu_);               // one stream, several feeders: keep copy + event together
                    for (const Segment& sg : plans[(size_t)c].in) {
                        hipError_t e2 = hipMemcpyAsync(dev_in_[slot].as<uint8_t>() + sg.slot_off, pin_in_[slot].p + sg.slot_off, sg.bytes, hipMemcpyHostToDevice, s_up_);
                        if (e2 != hipSuccess) { fail(e2, "hipMemcpyAsync (upload)"); return; }
                    }
                    hipError_t e2 = hipEventRecord(ev_up_[slot], s_up_);
                    if (e2 != hipSuccess) { fail(e2, "hipEventRecord"); return; }
                }
                set_state(c, 1);
            }
        };
        auto drainer = [&](int id) {
            if (hipSetDevice(device) != hipSuccess) { fail(hipErrorInvalidDevice, "hipSetDevice"); return; }
            for (int c = id; c < n_chunks && !failed.load(); c += n_drain) {
                const int slot = c % RING;
                if (!wait_state(c, 2)) return;
                hipError_t e2 = hipEventSynchronize(ev_down_[slot]);
                if (e2 != hipSuccess) { fail(e2, "hipEventSynchronize"); return; }
                for (const Segment& sg : plans[(size_t)c].out) std::memcpy(sg.host, pin_out_[slot].p + sg.slot_off, sg.bytes);
                set_state(c, 3);
            }
        };
        // Joined on every way out of this scope: an exception below (a thread that cannot be started, an allocation, a
        // throwing kernel callback) first raises `failed` -- the workers' waits all watch it -- and then joins them, instead
        // of destroying joinable threads (std::terminate) before the C-ABI's catch can turn it into an error code.
        Joiner threads{ 0, [&] {
            int expected = 0;
            failed.compare_exchange_strong(expected, (int)hipErrorUnknown);
            cv.notify_all();
        } };
        threads.ts.reserve((size_t)(n_feed + n_drain));
        try {
            for (int k = 0; k < n_feed; ++k) threads.start(feeder, k);
            for (int k = 0; k < n_drain; ++k) threads.start(drainer, k);
        } catch (const std::exception&) {
            fail(hipErrorOutOfMemory, "starting a copy thread");
        }

        for (int c = 0; c < n_chunks && !failed.load(); ++c) {
            const int slot = c % RING;
            if (!wait_state(c, 1)) break;
            if (c >= RING && !wait_state(c - RING, 3)) break;             // the slot's output buffers have been delivered
            hipError_t e2 = hipStreamWaitEvent(compute, ev_up_[slot], 0);
            if (e2 == hipSuccess) e2 = kernel(c, dev_in_[slot].as<uint8_t>(), dev_out_[slot].as<uint8_t>(), compute);
            if (e2 == hipSuccess) e2 = hipEventRecord(ev_k_[slot], compute);
            if (e2 == hipSuccess) e2 = hipStreamWaitEvent(s_down_, ev_k_[slot], 0);
            for (const Segment& sg : plans[(size_t)c].out) {
                if (e2 != hipSuccess) break;
                e2 = hipMemcpyAsync(pin_out_[slot].p + sg.slot_off, dev_out_[slot].as<uint8_t>() + sg.slot_off, sg.bytes, hipMemcpyDeviceToHost, s_down_);
            }
            if (e2 == hipSuccess) e2 = hipEventRecord(ev_down_[slot], s_down_);
            if (e2 != hipSuccess) { fail(e2, "launch / download"); break; }
            set_state(c, 2);
        }
        threads.join();
        if (failed.load()) {
            (void)hipStreamSynchronize(compute);
            (void)hipStreamSynchronize(s_up_);
            (void)hipStreamSynchronize(s_down_);
            return (hipError_t)failed.load();
        }
        return hipStreamSynchronize(compute);        // (every download has been waited for by its drainer)
    }

private:
    // the slots of one direction are regrown together, to one capacity (the last slot is allocated last: it tells whether all were)
    static hipError_t regrow(PinBuf (&pin)[RING], DevBuf (&dev)[RING], size_t n)
    {
        if (n <= pin[RING - 1].cap && n <= dev[RING - 1].cap) return hipSuccess;
        for (int k = 0; k < RING; ++k) { pin[k].release(); dev[k].release(); }
        hipError_t e = hipSuccess;
        for (int k = 0; k < RING && e == hipSuccess; ++k)
            if ((e = pin[k].try_reserve(n)) == hipSuccess) e = dev[k].try_reserve(n);
        return e;
    }

    hipError_t reserve(size_t in, size_t out)
    {
        hipError_t e = s_up_.create();
        if (e == hipSuccess) e = s_down_.create();
        for (int k = 0; k < RING && e == hipSuccess; ++k) {
            e = ev_up_[k].create();
            if (e == hipSuccess) e = ev_k_[k].create();
            if (e == hipSuccess) e = ev_down_[k].create();
        }
        if (e == hipSuccess) e = regrow(pin_in_, dev_in_, in);
        if (e == hipSuccess) e = regrow(pin_out_, dev_out_, out);
        return e;
    }

    PinBuf pin_in_[RING], pin_out_[RING];
    DevBuf dev_in_[RING], dev_out_[RING];
    Event ev_up_[RING], ev_k_[RING], ev_down_[RING];
    Stream s_up_, s_down_;
    std::mutex up_mu_;
};

}  // namespace jpezy_host
