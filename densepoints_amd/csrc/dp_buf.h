// dp_buf.h -- the owning resource types of the host code: device memory that
// only grows (DevBuf), pinned host memory that only grows (HostBuf), an exact
// device allocation (DevMem) and an event (Event), and two things built from
// them: a timed section (Timer) and striped statistics counters
// (StripedCounters).  Each frees in its destructor, moves and does not copy, so
// a context's members need no hand-written cleanup.  Depends on the HIP
// runtime API alone.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace dpk {

// device memory, grown (never shrunk) by reserve(): below 1024 elements to
// 1024, from 1024 on to n + n/4; the old contents are not kept
template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    // a failed allocation leaves the buffer empty
    hipError_t reserve(size_t n)
    {
        if (n <= cap)
            return hipSuccess;
        release();
        size_t want = n < 1024 ? 1024 : n + n / 4;
        hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if (e == hipSuccess)
            cap = want;
        else
            p = nullptr;
        return e;
    }
    void release()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// pinned host memory (grown to k + k/4, never shrunk): device->host copies of a
// result run at DMA speed instead of through a staging buffer.  resize(k) sets
// n = k; a failed allocation leaves the buffer empty with n as it was.
template <typename T> struct HostBuf {
    T *p = nullptr;
    size_t cap = 0, n = 0;
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    HostBuf(HostBuf &&o) noexcept : p(o.p), cap(o.cap), n(o.n) { o.p = nullptr, o.cap = o.n = 0; }
    HostBuf &operator=(HostBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap, n = o.n;
            o.p = nullptr, o.cap = o.n = 0;
        }
        return *this;
    }
    ~HostBuf() { release(); }
    hipError_t resize(size_t k)
    {
        if (k > cap) {
            if (p)
                (void)hipHostFree(p);
            p = nullptr;
            cap = 0;
            const size_t want = k + k / 4;
            hipError_t e = hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault);
            if (e != hipSuccess) {
                p = nullptr;
                return e;
            }
            cap = want;
        }
        n = k;
        return hipSuccess;
    }
    void clear() { n = 0; }
    bool empty() const { return n == 0; }
    T *data() { return p; }
    void release()
    {
        if (p)
            (void)hipHostFree(p);
        p = nullptr;
        cap = n = 0;
    }
};

// one device allocation of exactly the bytes asked for, replaced by alloc()
struct DevMem {
    void *p = nullptr;
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    DevMem(DevMem &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevMem &operator=(DevMem &&o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p;
            o.p = nullptr;
        }
        return *this;
    }
    ~DevMem() { release(); }
    hipError_t alloc(size_t bytes)
    {
        release();
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess)
            p = nullptr;
        return e;
    }
    void release()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
    }
};

// an event: null until create(), or until its first use as a hipEvent_t,
// which creates it with the default flags
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept
    {
        if (this != &o) {
            release();
            e = o.e;
            o.e = nullptr;
        }
        return *this;
    }
    ~Event() { release(); }
    // no-ops on an event that exists
    hipError_t create() { return e ? hipSuccess : hipEventCreate(&e); }
    hipError_t create(unsigned flags) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t()
    {
        (void)create();
        return e;
    }
    void release()
    {
        if (e)
            (void)hipEventDestroy(e);
        e = nullptr;
    }
};

// a timed section of a stream: begin and end record an event each, ms reads
// the time between them once the stream has passed both
struct Timer {
    Event e0, e1;
    hipError_t begin(hipStream_t s) { return hipEventRecord(e0, s); }
    hipError_t end(hipStream_t s) { return hipEventRecord(e1, s); }
    hipError_t ms(double &out)
    {
        float t = 0.0f;
        const hipError_t e = hipEventElapsedTime(&t, e0, e1);
        out = (double)t;
        return e;
    }
};

// `counters` statistics kept `stripes` times on the device, so that the waves'
// adds (wave_count, dp_mapdev.h) spread over as many addresses, and their
// pinned copy; `extra` pinned words behind the copy take the totals a stage
// reads in the same wait
struct StripedCounters {
    DevBuf<unsigned long long> dev;
    HostBuf<unsigned long long> host;
    int stripes = 0, counters = 0;
    size_t words() const { return (size_t)stripes * (size_t)counters; }
    hipError_t reserve(int stripes_, int counters_, size_t extra_words = 0)
    {
        stripes = stripes_, counters = counters_;
        const hipError_t e = dev.reserve(words());
        return e != hipSuccess ? e : host.resize(words() + extra_words);
    }
    hipError_t zero(hipStream_t s) { return hipMemsetAsync(dev.p, 0, sizeof(unsigned long long) * words(), s); }
    // queues the copy; the sums are valid once the stream has passed it
    hipError_t read(hipStream_t s)
    {
        return hipMemcpyAsync(host.p, dev.p, sizeof(unsigned long long) * words(), hipMemcpyDeviceToHost, s);
    }
    unsigned long long *extra() { return host.p + words(); }
    int64_t sum(int k) const
    {
        int64_t t = 0;
        for (int st = 0; st < stripes; ++st)
            t += (int64_t)host.p[st * counters + k];
        return t;
    }
};

} // namespace dpk
