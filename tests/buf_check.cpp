// The owning types of densepoints_amd/csrc/dp_buf.h against counting stand-ins
// for the HIP calls they make (no device, no HIP runtime library); built with
// the host compiler under ASan + UBSan and run by tests/test_buf_cpu.py.
#include "dp_buf.h"

#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

static int g_alloc = 0, g_free = 0, g_ev = 0, g_ev_free = 0, g_fail = 0, g_bad = 0;
static size_t g_bytes = 0; // of the last allocation

static hipError_t take(void **p, size_t bytes)
{
    if (g_fail)
        return hipErrorOutOfMemory;
    ++g_alloc;
    g_bytes = bytes;
    *p = std::malloc(bytes ? bytes : 1);
    return hipSuccess;
}
extern "C" hipError_t hipMalloc(void **p, size_t bytes) { return take(p, bytes); }
extern "C" hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return take(p, bytes); }
extern "C" hipError_t hipFree(void *p) { return ++g_free, std::free(p), hipSuccess; }
extern "C" hipError_t hipHostFree(void *p) { return ++g_free, std::free(p), hipSuccess; }
extern "C" hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned)
{
    return ++g_ev, *e = (hipEvent_t)std::malloc(1), hipSuccess;
}
extern "C" hipError_t hipEventCreate(hipEvent_t *e) { return hipEventCreateWithFlags(e, 0); }
extern "C" hipError_t hipEventDestroy(hipEvent_t e) { return ++g_ev_free, std::free(e), hipSuccess; }

#define CHECK(x) ((x) ? (void)0 : (void)(++g_bad, std::printf("FAIL line %d: %s\n", __LINE__, #x)))

struct Several {
    dpk::DevBuf<double> a, b;
    dpk::HostBuf<int> h;
    dpk::DevMem m;
    dpk::Event e0, e1;
};

int main()
{
    { // DevBuf: below 1024 elements to 1024, from there to n + n/4; never shrinks; no allocation below capacity
        const size_t n[4] = {1, 1024, 1025, 5000}, cap[4] = {1024, 1280, 1281, 6250};
        for (int i = 0; i < 4; ++i) {
            dpk::DevBuf<float> d;
            CHECK(d.p == nullptr && d.cap == 0);
            CHECK(d.reserve(n[i]) == hipSuccess && d.cap == cap[i] && g_bytes == cap[i] * sizeof(float) && d.p);
            const int before = g_alloc;
            float *p = d.p;
            CHECK(d.reserve(n[i] - 1) == hipSuccess && d.reserve(cap[i]) == hipSuccess);
            CHECK(g_alloc == before && d.p == p && d.cap == cap[i]);
            CHECK(d.reserve(cap[i] + 1) == hipSuccess && g_alloc == before + 1 && d.cap == cap[i] + 1 + (cap[i] + 1) / 4);
            g_fail = 1; // a failed growth leaves the buffer empty and returns the error
            CHECK(d.reserve(2 * d.cap) == hipErrorOutOfMemory && d.p == nullptr && d.cap == 0);
            g_fail = 0;
        }
    }
    CHECK(g_alloc == 8 && g_free == 8);
    { // HostBuf: to k + k/4, n follows resize, capacity never shrinks
        dpk::HostBuf<int> h;
        CHECK(h.empty() && h.resize(1000) == hipSuccess && h.n == 1000 && h.cap == 1250 && g_bytes == 1250 * sizeof(int));
        const int before = g_alloc;
        CHECK(h.resize(10) == hipSuccess && h.n == 10 && h.cap == 1250 && g_alloc == before);
        CHECK(h.resize(1250) == hipSuccess && h.n == 1250 && g_alloc == before && h.data() == h.p);
        h.clear();
        CHECK(h.empty() && h.cap == 1250);
        CHECK(h.resize(1251) == hipSuccess && h.n == 1251 && h.cap == 1251 + 1251 / 4 && g_alloc == before + 1);
        g_fail = 1;
        CHECK(h.resize(4000) == hipErrorOutOfMemory && h.p == nullptr && h.cap == 0);
        g_fail = 0;
    }
    CHECK(g_alloc == g_free);
    { // a moved-from object frees nothing; a move onto an owner frees what it held
        const int a0 = g_alloc, f0 = g_free, e0 = g_ev_free;
        dpk::DevBuf<int> a, c;
        CHECK(a.reserve(10) == hipSuccess && c.reserve(10) == hipSuccess);
        int *p = a.p;
        dpk::DevBuf<int> b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.p == p && b.cap == 1024);
        c = std::move(b);
        CHECK(g_free == f0 + 1 && c.p == p && b.p == nullptr);
        a.release(), b.release();
        CHECK(g_free == f0 + 1 && g_alloc == a0 + 2);
        dpk::Event x, y;
        CHECK(x.e == nullptr && x.create(2) == hipSuccess && x.e && x.create() == hipSuccess && g_ev == 1);
        hipEvent_t h = y; // created on first use
        CHECK(h && h == y.e && g_ev == 2);
        dpk::Event z(std::move(x));
        y = std::move(z);
        CHECK(g_ev_free == e0 + 1 && x.e == nullptr && z.e == nullptr && y.e);
    }
    CHECK(g_alloc == g_free && g_ev == g_ev_free);
    { // a struct of several owners and a vector of events free themselves
        Several s;
        CHECK(s.a.reserve(3) == hipSuccess && s.b.reserve(3000) == hipSuccess && s.h.resize(7) == hipSuccess);
        CHECK(s.m.alloc(64) == hipSuccess && s.m.alloc(32) == hipSuccess && s.e0.create() == hipSuccess);
        CHECK(g_bytes == 32 && s.e1.e == nullptr);
        std::vector<dpk::Event> ev(5);
        for (auto &e : ev)
            CHECK(e.create() == hipSuccess);
        ev.resize(40); // reallocates: the events move
        Several t(std::move(s));
        CHECK(s.a.p == nullptr && t.a.p && s.e0.e == nullptr && t.e0.e);
    }
    CHECK(g_alloc == g_free && g_ev == g_ev_free && g_ev == 2 + 1 + 5);
    std::printf("%s: %d allocations, %d events\n", g_bad ? "FAILED" : "ok", g_alloc, g_ev);
    return g_bad ? 1 : 0;
}
