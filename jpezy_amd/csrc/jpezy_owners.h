// jpezy_owners.h -- the error plumbing and the four owning types of the C-ABI's host layer (internal): device buffer, pinned host
// buffer, stream / event, joined threads.  Each has one job, is move-only and releases what it holds in its destructor, so a context,
// a staging ring or a lane frees itself.  What must happen BEFORE a free (hipSetDevice, a synchronisation) belongs in the destructor
// body of the owner's owner: members go after that body, in reverse order of declaration, and nothing here relies on that order.
#pragma once
#include <hip/hip_runtime.h>

#include <exception>
#include <functional>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/jpezy_hip.h"

namespace jpezy_capi {

inline thread_local std::string g_err;

inline int set_err(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}
inline int hip_err(hipError_t e, const char* what)
{
    return set_err(JPEZY_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// Device memory that only grows.  try_reserve: the HIP error; reserve: a jpezy_status with the message set.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DevBuf() { release(); }
    template <class T> T* as() const { return static_cast<T*>(p); }
    hipError_t try_reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) cap = n;
        else p = nullptr;
        return e;
    }
    int reserve(size_t n)
    {
        const hipError_t e = try_reserve(n);
        return e == hipSuccess ? 0 : hip_err(e, "hipMalloc");
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Its pinned-host twin.  A buffer shorter than `need` is freed and allocated again with `alloc` bytes (0: need) -- the caller's
// growth rule.  try_reserve: the HIP error; reserve: a jpezy_status with the message set; reserve_soft: for callers with a pageable
// way round -- false, and HIP's sticky error cleared so that the next checked call does not report this one.
struct PinBuf {
    uint8_t* p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(PinBuf&& o) noexcept { *this = std::move(o); }
    PinBuf& operator=(PinBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~PinBuf() { release(); }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
    hipError_t try_reserve(size_t need, size_t alloc = 0)
    {
        if (need <= cap) return hipSuccess;
        release();
        alloc = alloc > need ? alloc : need;
        const hipError_t e = hipHostMalloc((void**)&p, alloc, hipHostMallocDefault);
        if (e == hipSuccess) cap = alloc;
        else p = nullptr;
        return e;
    }
    int reserve(size_t need, size_t alloc = 0)
    {
        const hipError_t e = try_reserve(need, alloc);
        return e == hipSuccess ? 0 : hip_err(e, "hipHostMalloc");
    }
    bool reserve_soft(size_t need, size_t alloc = 0)
    {
        if (try_reserve(need, alloc) == hipSuccess) return true;
        (void)hipGetLastError();
        return false;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// A stream / an event of the current device; both read as their handle.  create() on a live owner does nothing.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept { *this = std::move(o); }
    Stream& operator=(Stream&& o) noexcept { std::swap(s, o.s); return *this; }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept { *this = std::move(o); }
    Event& operator=(Event&& o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDisableTiming) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

// Threads that are joined on every way out of their scope.  An exception that unwinds past joinable std::threads is
// std::terminate -- inside a C ABI that promises a status instead (JPEZY_CATCH).  on_unwind, when given, runs first if the scope is
// left by an exception while threads still run: it tells workers that wait for the unwinding thread to give up.
struct Joiner {
    std::vector<std::thread> ts;
    std::function<void()> on_unwind;
    explicit Joiner(size_t n = 0, std::function<void()> f = nullptr) : ts(n), on_unwind(std::move(f)) {}   // n: a fixed array of n slots
    Joiner(const Joiner&) = delete;
    Joiner& operator=(const Joiner&) = delete;
    template <class... A> void start(A&&... a) { ts.emplace_back(std::forward<A>(a)...); }
    void join(size_t k) { if (ts[k].joinable()) ts[k].join(); }
    void join() { for (size_t k = 0; k < ts.size(); ++k) join(k); }
    ~Joiner()
    {
        bool running = false;
        for (auto& t : ts) running = running || t.joinable();
        if (running && on_unwind && std::uncaught_exceptions() > 0) on_unwind();
        join();
    }
};

}  // namespace jpezy_capi
