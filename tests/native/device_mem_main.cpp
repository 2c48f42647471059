// pt_device_mem.hpp on the CPU, under AddressSanitizer + UBSan: the plane layout is a pure function of sizes and gives the
// allocation sizes the host layer had when they were written out by hand; the owners free exactly once, an empty owner makes
// no HIP call, a failed allocation leaves nothing behind.  Built and run by tests/test_device_mem_host.py; the six HIP calls
// the header makes are stubbed here and count themselves.
#include "pt_device_mem.hpp"

#include <cstdio>
#include <set>
#include <utility>
#include <vector>

static int g_mallocs = 0, g_frees = 0, g_event_destroys = 0, g_stream_destroys = 0, g_double_frees = 0;
static bool g_fail_malloc = false;
static std::set<void *> g_blocks;   // what the stubbed hipMalloc handed out and hipFree has not seen yet
static char g_arena[64];            // tagged pointers: block k is &g_arena[k] (never dereferenced)

extern "C" {
hipError_t hipMalloc(void **p, size_t) {
    if (g_fail_malloc) return hipErrorOutOfMemory;
    *p = &g_arena[++g_mallocs];
    g_blocks.insert(*p);
    return hipSuccess;
}
hipError_t hipFree(void *p) {
    ++g_frees;
    if (!g_blocks.erase(p)) ++g_double_frees;
    return hipSuccess;
}
hipError_t hipMemcpy(void *, const void *, size_t, hipMemcpyKind) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
    *e = reinterpret_cast<hipEvent_t>(&g_arena[1]);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t) { return ++g_event_destroys, hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) {
    *s = reinterpret_cast<hipStream_t>(&g_arena[2]);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t) { return ++g_stream_destroys, hipSuccess; }
}

namespace ptc {
std::atomic<long> g_live_device_objects{0};
int hip_fail(hipError_t e, const char *) {   // pt_capi.cpp's mapping
    return e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver ? PT_ERR_NO_DEVICE
           : e == hipErrorOutOfMemory                                                            ? PT_ERR_OUT_OF_MEMORY
                                                                                                 : PT_ERR_HIP;
}
}  // namespace ptc

#define EXPECT(cond)                                          \
    do {                                                      \
        if (!(cond)) {                                        \
            std::printf("line %d: %s\n", __LINE__, #cond);    \
            return 1;                                         \
        }                                                     \
    } while (0)

using ptc::AccumPlanes;
using ptc::DeviceBuffer;
using ptc::DeviceEvent;
using ptc::DeviceStream;
using ptc::PlaneLayout;

static long live() { return ptc::g_live_device_objects.load(); }
static size_t up(size_t b) { return (b + 255) / 256 * 256; }

// Adds planes of `bytes` each; every offset must be a multiple of 256 and at or behind the end of the plane before it.
static bool add_planes(PlaneLayout &l, int count, size_t bytes, size_t &prev_end) {
    for (int k = 0; k < count; ++k) {
        const size_t at = l.add(bytes);
        if (at % 256 != 0 || at < prev_end || l.end != at + bytes) return false;
        prev_end = at + bytes;
    }
    return true;
}
static bool add_accum(PlaneLayout &l, size_t n, size_t &prev_end) {
    const AccumPlanes a = AccumPlanes::in(l, n);
    const size_t bytes[3] = {12 * n, 12 * n, 4 * n};
    for (int k = 0; k < 3; ++k) {
        if (a.offset[k] % 256 != 0 || a.offset[k] < prev_end) return false;
        prev_end = a.offset[k] + bytes[k];
    }
    return a.n == n && l.end == prev_end;
}

static int test_layout() {
    for (size_t n : {size_t(1), size_t(63), size_t(64), size_t(65), size_t(2073600)}) {
        const size_t b12 = up(12 * n), b4 = up(4 * n), b16 = up(16 * n);
        {   // pt_denoise_host: six planes of 12 n bytes, three of 4 n, four records of 16 n
            PlaneLayout l;
            size_t e = 0;
            EXPECT(add_planes(l, 6, 12 * n, e) && add_planes(l, 3, 4 * n, e) && add_planes(l, 4, 16 * n, e));
            EXPECT(l.total() == 6 * b12 + 3 * b4 + 4 * b16 && l.total() >= e);
        }
        {   // pt_temporal_create: the frame's and the merged accumulators, five planes of 12 n, three of 4 n, eight records
            PlaneLayout l;
            size_t e = 0;
            EXPECT(add_accum(l, n, e) && add_accum(l, n, e));
            EXPECT(add_planes(l, 5, 12 * n, e) && add_planes(l, 3, 4 * n, e) && add_planes(l, 8, 16 * n, e));
            EXPECT(l.total() == 9 * b12 + 5 * b4 + 8 * b16 && l.total() >= e);
        }
        {   // the temporal stage's denoiser planes: four records, the mean, its count
            PlaneLayout l;
            size_t e = 0;
            EXPECT(add_planes(l, 4, 16 * n, e) && add_planes(l, 1, 12 * n, e) && add_planes(l, 1, 4 * n, e));
            EXPECT(l.total() == 4 * b16 + b12 + b4 && l.total() >= e);
        }
        {   // a session's / a frame's / pt_render_host's band: the triple, unpadded, and 256 bytes of slack
            PlaneLayout l;
            size_t e = 0;
            EXPECT(add_accum(l, n, e));
            EXPECT(l.end + 256 == (2 * ((3 * n + 63) / 64 * 64) + n) * 4 + 256);
        }
    }
    return 0;
}

static int test_owners() {
    {   // empty owners: default constructed, moved from, reset
        DeviceBuffer b, b2(std::move(b));
        DeviceEvent e, e2(std::move(e));
        DeviceStream s, s2(std::move(s));
        b2 = DeviceBuffer();
        e2 = DeviceEvent();
        s2 = DeviceStream();
        b.reset(); e.reset(); s.reset();
        EXPECT(!b && !b2 && !e && !e2 && !s && !s2 && b.bytes() == 0 && b.get<char>() == nullptr);
    }
    EXPECT(g_frees == 0 && g_event_destroys == 0 && g_stream_destroys == 0 && live() == 0);
    {   // move construction and move assignment transfer ownership: one free per allocation
        DeviceBuffer a;
        EXPECT(a.alloc(100, "a") == PT_OK && a && a.bytes() == 100 && live() == 1);
        void *const pa = a.get<void>();
        DeviceBuffer b(std::move(a));
        EXPECT(!a && a.bytes() == 0 && b.get<void>() == pa && b.bytes() == 100 && g_frees == 0 && live() == 1);
        DeviceBuffer c;
        EXPECT(c.alloc(7, "c") == PT_OK && live() == 2);
        void *const pc = c.get<void>();
        c = std::move(b);   // frees c's own block, takes b's
        EXPECT(!b && c.get<void>() == pa && c.bytes() == 100 && g_frees == 1 && !g_blocks.count(pc) && live() == 1);
        EXPECT(c.at<char>(32) == static_cast<char *>(pa) + 32);
        // alloc on an owner that holds memory frees the old block first
        EXPECT(c.alloc(5, "again") == PT_OK && g_frees == 2 && !g_blocks.count(pa) && c.bytes() == 5 && live() == 1);
        // a failing hipMalloc leaves the owner empty and the count as it was without it
        g_fail_malloc = true;
        DeviceBuffer d;
        EXPECT(d.alloc(1, "d") == PT_ERR_OUT_OF_MEMORY && !d && d.bytes() == 0 && live() == 1);
        EXPECT(c.alloc(9, "c") == PT_ERR_OUT_OF_MEMORY && !c && c.bytes() == 0 && g_frees == 3 && live() == 0);
        const std::vector<int> v(5, 1);
        EXPECT(d.upload(v, "v") == PT_ERR_OUT_OF_MEMORY && !d && live() == 0);
        g_fail_malloc = false;
        EXPECT(d.upload(v, "v") == PT_OK && d.bytes() == 5 * sizeof(int) + 256 && live() == 1);
        PlaneLayout l;
        l.add(10);
        l.add(10);
        EXPECT(d.alloc(l, "planes") == PT_OK && d.bytes() == 512 && g_frees == 4 && live() == 1);
    }
    EXPECT(g_frees == 5 && g_frees == g_mallocs && g_blocks.empty() && g_double_frees == 0 && live() == 0);
    {   // events and streams: the same
        DeviceEvent e;
        DeviceStream s;
        EXPECT(e.create("e", hipEventDisableTiming) == PT_OK && s.create("s") == PT_OK && e && s && live() == 2);
        DeviceEvent e2(std::move(e));
        DeviceStream s2;
        s2 = std::move(s);
        EXPECT(!e && !s && e2 && s2 && e2.get() && s2.get() && g_event_destroys == 0 && g_stream_destroys == 0 && live() == 2);
        EXPECT(e2.create("again") == PT_OK && g_event_destroys == 1 && live() == 2);
    }
    EXPECT(g_event_destroys == 2 && g_stream_destroys == 1 && live() == 0);
    return 0;
}

int main() {
    if (test_layout() || test_owners()) return 1;
    std::printf("device mem ok\n");
    return 0;
}
