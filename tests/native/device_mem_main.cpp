// pt_device_mem.hpp on the CPU, under AddressSanitizer + UBSan: the plane layout is a pure function of sizes and gives the
// allocation sizes the host layer had when they were written out by hand; the owners free exactly once, an empty owner makes
// no HIP call, a failed allocation leaves nothing behind; the views of the plane sets lay out what the entry points had, the
// timer owns its two events, and the timed region of pt_capi_internal.hpp records one event on each side of what it is given.
// Built and run by tests/test_device_mem_host.py; the HIP calls the headers make are stubbed here and count themselves.
#include "pt_capi_internal.hpp"
#include "pt_device_mem.hpp"

#include <algorithm>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

static int g_mallocs = 0, g_frees = 0, g_event_destroys = 0, g_stream_destroys = 0, g_double_frees = 0;
static bool g_fail_malloc = false;
static std::set<void *> g_blocks;   // what the stubbed hipMalloc handed out and hipFree has not seen yet
static char g_arena[8192];          // tagged pointers: block k is &g_arena[k] (never dereferenced); room for the views of one pixel
static int g_records = 0, g_syncs = 0, g_copies = 0, g_events = 0, g_calls = 0;   // g_calls: every stubbed call
struct Recorded { hipEvent_t event; hipStream_t stream; };
static std::vector<Recorded> g_recorded;        // hipEventRecord, in order
static hipEvent_t g_synced = nullptr, g_elapsed[2] = {nullptr, nullptr};

extern "C" {
hipError_t hipMalloc(void **p, size_t) {
    ++g_calls;
    if (g_fail_malloc) return hipErrorOutOfMemory;
    *p = &g_arena[++g_mallocs];
    g_blocks.insert(*p);
    return hipSuccess;
}
hipError_t hipFree(void *p) {
    ++g_calls;
    ++g_frees;
    if (!g_blocks.erase(p)) ++g_double_frees;
    return hipSuccess;
}
hipError_t hipMemcpy(void *, const void *, size_t, hipMemcpyKind) { return ++g_calls, ++g_copies, hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
    *e = reinterpret_cast<hipEvent_t>(&g_arena[1 + ++g_events % 4096]);   // (no two live events of a test share a tag)
    return ++g_calls, hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t) { return ++g_calls, ++g_event_destroys, hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    g_recorded.push_back({e, s});
    return ++g_calls, ++g_records, hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) { return g_synced = e, ++g_calls, ++g_syncs, hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b) {
    g_elapsed[0] = a; g_elapsed[1] = b;
    return ++g_calls, *ms = 2.5f, hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) {
    *s = reinterpret_cast<hipStream_t>(&g_arena[2]);
    return ++g_calls, hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t) { return ++g_calls, ++g_stream_destroys, hipSuccess; }
}

namespace ptc {
std::atomic<long> g_live_device_objects{0};
int fail(int code, const std::string &) { return code; }
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
using ptc::BloomPlanes;
using ptc::DenoisePlanes;
using ptc::DeviceBuffer;
using ptc::DeviceEvent;
using ptc::DeviceStream;
using ptc::DeviceTimer;
using ptc::FeaturePlanes;
using ptc::LocalPlanes;
using ptc::MeanPlanes;
using ptc::PlaneLayout;
using ptc::UpsamplePlanes;

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

// The planes of a view as (offset, bytes), for the same checks: whatever order the view adds them in, each starts on a multiple
// of 256 at or behind the end of the plane before it, and the last one added ends the layout.
using Spans = std::vector<std::pair<size_t, size_t>>;
static Spans spans(const MeanPlanes &m) { return {{m.offset[0], 12 * m.n}, {m.offset[1], 4 * m.n}}; }
static Spans spans(const FeaturePlanes &f) {
    Spans s = {{f.offset[0], 12 * f.n}, {f.offset[1], 12 * f.n}, {f.offset[2], 12 * f.n}, {f.offset[3], 4 * f.n}};
    if (f.traced) s.insert(s.end(), {{f.offset[4], 12 * f.n}, {f.offset[5], 12 * f.n}, {f.offset[6], 4 * f.n}});
    return s;
}
static Spans spans(const DenoisePlanes &w) {
    Spans s = spans(w.out);
    for (size_t o : w.offset) s.push_back({o, 16 * w.out.n});
    return s;
}
static Spans spans(const UpsamplePlanes &w) {
    Spans s = {{w.offset[0], 16 * w.n_lo}, {w.offset[1], 16 * w.n_lo}, {w.offset[2], 16 * w.n_lo}};
    if (w.own_mean) s.push_back({w.offset[3], 12 * w.n_lo});
    return s;
}
static size_t pixels(const MeanPlanes &m) { return m.n; }
static size_t pixels(const FeaturePlanes &f) { return f.n; }
static size_t pixels(const DenoisePlanes &w) { return w.out.n; }
static size_t pixels(const UpsamplePlanes &w) { return w.n_lo; }
static bool spans_ok(Spans s, const PlaneLayout &l, size_t &prev_end) {
    std::sort(s.begin(), s.end());
    for (const auto &p : s) {
        if (p.first % 256 != 0 || p.first < prev_end) return false;
        prev_end = p.first + p.second;
    }
    return l.end == prev_end;
}
template <class View, class... More>
static bool add_view(PlaneLayout &l, size_t n, size_t &prev_end, size_t planes, More... more) {
    const View v = View::in(l, n, more...);
    return pixels(v) == n && spans(v).size() == planes && spans_ok(spans(v), l, prev_end);
}

// The views as the entry points compose them: the totals are the sums those places wrote out by hand.
static int test_views() {
    for (size_t n : {size_t(1), size_t(63), size_t(64), size_t(65), size_t(2073600)}) {
        const size_t b12 = up(12 * n), b4 = up(4 * n), b16 = up(16 * n);
        {   // pt_denoise_host: the accumulators, the uploaded features, the denoiser's planes
            PlaneLayout l;
            size_t e = 0;
            EXPECT(add_accum(l, n, e));
            const FeaturePlanes f = FeaturePlanes::uploaded_in(l, n);
            EXPECT(f.n == n && !f.traced && spans(f).size() == 4 && spans_ok(spans(f), l, e));
            EXPECT(add_view<DenoisePlanes>(l, n, e, 6));
            EXPECT(l.total() == 6 * b12 + 3 * b4 + 4 * b16 && l.total() >= e);
        }
        {   // pt_temporal_create: the frame's and the merged accumulators, the view's features, the frame counts, eight records
            PlaneLayout l;
            size_t e = 0;
            EXPECT(add_accum(l, n, e) && add_accum(l, n, e) && add_view<FeaturePlanes>(l, n, e, 7));
            EXPECT(add_planes(l, 1, 4 * n, e) && add_planes(l, 8, 16 * n, e));
            EXPECT(l.total() == 9 * b12 + 5 * b4 + 8 * b16 && l.total() >= e);
        }
        {   // the temporal stage's denoiser planes
            PlaneLayout l;
            size_t e = 0;
            EXPECT(add_view<DenoisePlanes>(l, n, e, 6));
            EXPECT(l.total() == 4 * b16 + b12 + b4 && l.total() >= e);
        }
        {   // the display's filter planes: the view's features, the denoiser's planes
            PlaneLayout l;
            size_t e = 0;
            EXPECT(add_view<FeaturePlanes>(l, n, e, 7) && add_view<DenoisePlanes>(l, n, e, 6));
            EXPECT(l.total() == 6 * b12 + 3 * b4 + 4 * b16 && l.total() >= e);
        }
        for (size_t s : {size_t(2), size_t(3), size_t(4)}) {
            if (n % (s * s)) continue;
            const size_t n_lo = n / (s * s);
            {   // a scaled present: the output's features, mean and count; the low mean and the records
                PlaneLayout l;
                size_t e = 0;
                EXPECT(add_view<FeaturePlanes>(l, n, e, 7) && add_view<MeanPlanes>(l, n, e, 2) && add_view<UpsamplePlanes>(l, n_lo, e, 4, true));
                EXPECT(l.total() == 6 * b12 + 3 * b4 + up(12 * n_lo) + 3 * up(16 * n_lo) && l.total() >= e);
            }
            {   // pt_upsample_host: the low image, the uploaded features, the output's mean and count, the records
                PlaneLayout l;
                size_t e = 0;
                EXPECT(add_view<MeanPlanes>(l, n_lo, e, 2));
                const FeaturePlanes f = FeaturePlanes::uploaded_in(l, n);
                EXPECT(f.n == n && spans(f).size() == 4 && spans_ok(spans(f), l, e));
                EXPECT(add_view<MeanPlanes>(l, n, e, 2) && add_view<UpsamplePlanes>(l, n_lo, e, 3, false));
                EXPECT(l.total() == up(12 * n_lo) + up(4 * n_lo) + 4 * b12 + 2 * b4 + 3 * up(16 * n_lo) && l.total() >= e);
            }
        }
    }
    {   // bind makes pointers of the offsets; what a view did not lay out stays NULL; a NULL side skips its plane's copy
        PlaneLayout l;
        FeaturePlanes f = FeaturePlanes::in(l, 1), g = FeaturePlanes::uploaded_in(l, 1);
        DenoisePlanes w = DenoisePlanes::in(l, 1);
        UpsamplePlanes u = UpsamplePlanes::in(l, 1, true), v = UpsamplePlanes::in(l, 1, false);
        DeviceBuffer b;
        EXPECT(l.total() <= sizeof g_arena - 64 && b.alloc(l, "views") == PT_OK);
        f.bind(b); g.bind(b); w.bind(b); u.bind(b); v.bind(b);
        char *const base = b.get<char>();
        EXPECT((char *)f.position == base + f.offset[0] && (char *)f.normal == base + f.offset[1] && (char *)f.albedo == base + f.offset[2]);
        EXPECT((char *)f.hit == base + f.offset[3] && (char *)f.origins == base + f.offset[4] && (char *)f.directions == base + f.offset[5]);
        EXPECT((char *)f.hit_t == base + f.offset[6]);
        EXPECT(!g.origins && !g.directions && !g.hit_t && (char *)g.position == base + g.offset[0] && (char *)g.hit == base + g.offset[3]);
        EXPECT((char *)w.rec_a0 == base + w.offset[0] && (char *)w.rec_c == base + w.offset[3] && (char *)w.out.rgb == base + w.out.offset[0]);
        EXPECT((char *)w.out.count == base + w.out.offset[1]);
        EXPECT((char *)u.rec_a == base + u.offset[0] && (char *)u.rec_c == base + u.offset[2] && (char *)u.mean_lo == base + u.offset[3] && !v.mean_lo);
        EXPECT((char *)v.rec_b == base + v.offset[1]);
        float x[3] = {0, 0, 0};
        int32_t i = 0;
        g_copies = 0;
        FeaturePlanes some, all;
        some.hit = all.hit = &i;
        some.position = all.position = all.normal = all.albedo = all.hit_t = x;
        EXPECT(f.download(some) == PT_OK && g_copies == 2 && f.download(all) == PT_OK && g_copies == 7);
        EXPECT(g.upload(x, x, x, &i) == PT_OK && g_copies == 11 && g.download(all) == PT_OK && g_copies == 15);   // (g has no hit_t plane)
        EXPECT(w.out.download(x, nullptr) == PT_OK && g_copies == 16 && w.out.upload(x, &i) == PT_OK && g_copies == 18);
    }
    EXPECT(live() == 0);
    return 0;
}

// Bloom's and local exposure's views against what ensure_bloom / bloom_host_impl and ensure_local / local_host_impl laid out by
// hand before the views existed: `12 n | 16 records` and `12 n | 4 n | 4 n`, for the one-shot entry points behind the uploaded
// mean image `12 n | 4 n` and the exposure scalar `4`.  Every expected number is written out here (each a multiple of 256 at or
// behind the end of the plane before it); the record counts are what pt::bloom_pyramid_records gave for the image and the levels.
static int test_stage_views() {
    struct BloomCase { size_t n, records, display_pyramid, display_total, host_count, host_e, host_out, host_pyramid, host_total; };
    const BloomCase bloom[] = {
        {1, 1, 256, 512, 256, 512, 768, 1024, 1280},                          // 1 x 1, one level
        {1, 8, 256, 512, 256, 512, 768, 1024, 1280},                          // 1 x 1, eight levels
        {35, 12, 512, 768, 512, 768, 1024, 1536, 1792},                       // 7 x 5, one level: 4 x 3
        {35, 22, 512, 1024, 512, 768, 1024, 1536, 2048},                      // 7 x 5, eight levels: 12 + 4 + 6 x 1
        {2150, 751, 25856, 37888, 25856, 34560, 34816, 60672, 72704},         // 50 x 43, five levels: 550 + 143 + 42 + 12 + 4
        {2150, 754, 25856, 38144, 25856, 34560, 34816, 60672, 72960},         // 50 x 43, eight levels: ... + 3 x 1
    };
    const int calls = g_calls;
    for (const BloomCase &c : bloom) {
        {   // DisplayDevice::ensure_bloom
            PlaneLayout l;
            const BloomPlanes w = BloomPlanes::in(l, c.n, c.records);
            EXPECT(w.n == c.n && w.offset[0] == 0 && w.offset[1] == c.display_pyramid && l.total() == c.display_total);
            EXPECT(l.end == c.display_pyramid + 16 * c.records && !w.out_rgb && !w.pyramid);
        }
        {   // pt_bloom_host
            PlaneLayout l;
            const MeanPlanes in = MeanPlanes::in(l, c.n);
            const size_t o_e = l.add(4);
            const BloomPlanes w = BloomPlanes::in(l, c.n, c.records);
            EXPECT(in.offset[0] == 0 && in.offset[1] == c.host_count && o_e == c.host_e);
            EXPECT(w.offset[0] == c.host_out && w.offset[1] == c.host_pyramid && l.total() == c.host_total);
        }
    }
    struct LocalCase { size_t n, display[3], display_total, host_count, host_e, host[3], host_total; };
    const LocalCase local[] = {
        {1, {0, 256, 512}, 768, 256, 512, {768, 1024, 1280}, 1536},
        {35, {0, 512, 768}, 1024, 512, 768, {1024, 1536, 1792}, 2048},
        {2150, {0, 25856, 34560}, 43264, 25856, 34560, {34816, 60672, 69376}, 78080},
    };
    for (const LocalCase &c : local) {
        {   // DisplayDevice::ensure_local
            PlaneLayout l;
            const LocalPlanes w = LocalPlanes::in(l, c.n);
            EXPECT(w.n == c.n && w.offset[0] == c.display[0] && w.offset[1] == c.display[1] && w.offset[2] == c.display[2]);
            EXPECT(l.total() == c.display_total && l.end == c.display[2] + 4 * c.n && !w.out_rgb && !w.base[0] && !w.base[1]);
        }
        {   // pt_local_host
            PlaneLayout l;
            const MeanPlanes in = MeanPlanes::in(l, c.n);
            const size_t o_e = l.add(4);
            const LocalPlanes w = LocalPlanes::in(l, c.n);
            EXPECT(in.offset[0] == 0 && in.offset[1] == c.host_count && o_e == c.host_e);
            EXPECT(w.offset[0] == c.host[0] && w.offset[1] == c.host[1] && w.offset[2] == c.host[2] && l.total() == c.host_total);
        }
    }
    EXPECT(g_calls == calls);   // in() is arithmetic
    {   // bind makes pointers of the offsets, and makes no HIP call either
        PlaneLayout l;
        MeanPlanes in = MeanPlanes::in(l, 1);
        l.add(4);
        BloomPlanes b = BloomPlanes::in(l, 1, 8);
        LocalPlanes w = LocalPlanes::in(l, 1);
        DeviceBuffer d;
        EXPECT(l.total() == 1280 + 768 && l.total() <= sizeof g_arena - 64 && d.alloc(l, "stage views") == PT_OK);
        const int bound = g_calls;
        in.bind(d); b.bind(d); w.bind(d);
        char *const base = d.get<char>();
        EXPECT(g_calls == bound && (char *)b.out_rgb == base + 768 && (char *)b.pyramid == base + 1024);
        EXPECT((char *)w.out_rgb == base + 1280 && (char *)w.base[0] == base + 1536 && (char *)w.base[1] == base + 1792);
    }
    EXPECT(live() == 0);
    return 0;
}

// ptc::timed: begin, the callable, end on the stream given; one wait; the two events are the call's own on both ways out.
static int test_timed() {
    const hipStream_t stream = reinterpret_cast<hipStream_t>(&g_arena[3]);
    const long before = live();
    const int destroyed = g_event_destroys;
    g_recorded.clear();
    g_records = g_syncs = 0;
    float ms = 0.0f;
    int ran = 0;
    bool inside_ok = false;
    int rc = ptc::timed(stream, "timed", &ms, [&]() -> int {
        ++ran;
        inside_ok = g_records == 1 && g_syncs == 0 && live() == before + 2;   // begin is behind us, end and the wait are not
        return PT_OK;
    });
    EXPECT(rc == PT_OK && ran == 1 && inside_ok && ms == 2.5f);
    EXPECT(g_records == 2 && g_recorded.size() == 2 && g_recorded[0].stream == stream && g_recorded[1].stream == stream);
    EXPECT(g_recorded[0].event != g_recorded[1].event && g_syncs == 1 && g_synced == g_recorded[1].event);
    EXPECT(g_elapsed[0] == g_recorded[0].event && g_elapsed[1] == g_recorded[1].event);
    EXPECT(live() == before && g_event_destroys == destroyed + 2);
    // the callable fails: its status comes back, nothing more is recorded, nothing is waited for
    ms = -1.0f;
    rc = ptc::timed(stream, "timed", &ms, [&]() -> int { return ++ran, static_cast<int>(PT_ERR_UNSUPPORTED); });
    EXPECT(rc == PT_ERR_UNSUPPORTED && ran == 2 && ms == -1.0f && g_records == 3 && g_recorded[2].stream == stream && g_syncs == 1);
    EXPECT(live() == before && g_event_destroys == destroyed + 4);
    return 0;
}

static int test_timer() {
    const int destroyed = g_event_destroys;
    {
        DeviceTimer empty, moved_to(std::move(empty));   // (no event: no HIP call)
        EXPECT(g_event_destroys == destroyed && live() == 0);
        DeviceTimer t;
        EXPECT(t.create("timer") == PT_OK && live() == 2);
        EXPECT(t.create("again") == PT_OK && live() == 2 && g_event_destroys == destroyed + 2);   // the first pair went
        float ms = 0.0f;
        EXPECT(t.begin(nullptr) == hipSuccess && t.end(nullptr) == hipSuccess && g_records == 2 && g_syncs == 0);
        EXPECT(t.wait_ms(&ms) == hipSuccess && g_syncs == 1 && ms == 2.5f);
        DeviceTimer u(std::move(t));
        EXPECT(live() == 2 && g_event_destroys == destroyed + 2);
        moved_to = std::move(u);
        EXPECT(live() == 2 && g_event_destroys == destroyed + 2);
    }
    EXPECT(g_event_destroys == destroyed + 4 && live() == 0);
    return 0;
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
    if (test_layout() || test_owners() || test_views() || test_stage_views() || test_timer() || test_timed()) return 1;
    std::printf("device mem ok\n");
    return 0;
}
