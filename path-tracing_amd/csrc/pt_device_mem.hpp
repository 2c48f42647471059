// Owners of what the host layer holds on a device: one hipMalloc, one event, one stream, the event pair of a timed region -- and the
// one spelling of "one allocation cut into 256-byte aligned planes": PlaneLayout, and a view for every set of planes that more than one
// place lays out (accumulators, mean and count, first-hit features, the work planes of the denoiser, the upsampler, bloom, local exposure).
// Host only; nothing here is part of the ABI.
// An owner frees in its destructor, on whatever device is current: the handle that holds it (pt_scene, pt_session, pt_frame,
// pt_temporal) makes its own device current first -- in its destructor's body, which runs before the members go.  An empty
// owner (default constructed, moved from, reset) makes no HIP call, so a scene without a device never touches the runtime.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdint>
#include <initializer_list>
#include <utility>
#include <vector>

#include "../../include/pt_hip.h"

namespace ptc {

int hip_fail(hipError_t e, const char *what);

// Owners that hold something right now (defined in pt_capi.cpp; the test builds export it as pt_test_live_device_objects):
// a leak of device memory fails no other test.
extern __attribute__((visibility("hidden"))) std::atomic<long> g_live_device_objects;   // (no symbol of the shared library)
inline void count_live(long d) { g_live_device_objects.fetch_add(d, std::memory_order_relaxed); }
inline void released(hipError_t) { count_live(-1); }   // (a handle is gone whatever its destroying call answered)
inline int hip_status(hipError_t e, const char *what) { return e == hipSuccess ? static_cast<int>(PT_OK) : hip_fail(e, what); }
// How every alloc / create ends: the new handle counted, or the owner left empty and the error reported.
template <class H>
int created(hipError_t e, H &handle, const char *what) {
    if (e == hipSuccess) count_live(1);
    else handle = nullptr;
    return hip_status(e, what);
}

// Offsets of planes in one allocation, each plane starting on a multiple of 256 bytes.  A pure function of the sizes added.
struct PlaneLayout {
    size_t end = 0;   // of the last plane added (not rounded up)
    size_t add(size_t bytes) { const size_t at = total(); end = at + bytes; return at; }
    size_t total() const { return (end + 255) / 256 * 256; }   // every plane a whole number of 256-byte units
};

// One hipMalloc.  Move-only; alloc frees what it held before, a failed alloc leaves it empty.
class DeviceBuffer {
    void *p_ = nullptr;
    size_t bytes_ = 0;

public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { DeviceBuffer old(std::move(*this)); std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); return *this; }
    ~DeviceBuffer() { reset(); }
    void reset() {
        if (p_) released(hipFree(std::exchange(p_, nullptr)));
        bytes_ = 0;
    }
    int alloc(size_t bytes, const char *what) {
        reset();
        const int rc = created(hipMalloc(&p_, bytes), p_, what);
        if (rc == PT_OK) bytes_ = bytes;
        return rc;
    }
    int alloc(const PlaneLayout &l, const char *what) { return alloc(l.total(), what); }
    // A table, with the bytes of slack behind it that the kernels may read into.
    template <class T>
    int upload(const std::vector<T> &v, const char *what, size_t slack = 256) {
        const int rc = alloc(v.size() * sizeof(T) + slack, what);
        if (rc != PT_OK || v.empty()) return rc;
        return hip_status(hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), what);
    }
    template <class T> T *get() const { return static_cast<T *>(p_); }
    template <class T> T *at(size_t offset) const { return reinterpret_cast<T *>(static_cast<char *>(p_) + offset); }   // (PlaneLayout::add)
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }
};

// One hipEvent_t, the same way.
class DeviceEvent {
    hipEvent_t ev_ = nullptr;

public:
    DeviceEvent() = default;
    DeviceEvent(DeviceEvent &&o) noexcept : ev_(std::exchange(o.ev_, nullptr)) {}
    DeviceEvent &operator=(DeviceEvent &&o) noexcept { DeviceEvent old(std::move(*this)); std::swap(ev_, o.ev_); return *this; }
    ~DeviceEvent() { reset(); }
    void reset() { if (ev_) released(hipEventDestroy(std::exchange(ev_, nullptr))); }
    int create(const char *what, unsigned flags = hipEventDefault) {
        reset();
        return created(hipEventCreateWithFlags(&ev_, flags), ev_, what);
    }
    hipEvent_t get() const { return ev_; }
    explicit operator bool() const { return ev_ != nullptr; }
};

// One non-blocking hipStream_t.
class DeviceStream {
    hipStream_t s_ = nullptr;

public:
    DeviceStream() = default;
    DeviceStream(DeviceStream &&o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    DeviceStream &operator=(DeviceStream &&o) noexcept { DeviceStream old(std::move(*this)); std::swap(s_, o.s_); return *this; }
    ~DeviceStream() { reset(); }
    void reset() { if (s_) released(hipStreamDestroy(std::exchange(s_, nullptr))); }
    int create(const char *what) {
        reset();
        return created(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking), s_, what);
    }
    hipStream_t get() const { return s_; }
    explicit operator bool() const { return s_ != nullptr; }
};

// The two events of a timed region: begin, the launches, end on one stream; wait_ms waits for the end and gives the time between.
// (The three answer as the runtime does, for PT_HIP_TRY.)
class DeviceTimer {
    DeviceEvent ev0_, ev1_;

public:
    int create(const char *what) {
        const int rc = ev0_.create(what);
        return rc != PT_OK ? rc : ev1_.create(what);
    }
    hipError_t begin(hipStream_t stream) const { return hipEventRecord(ev0_.get(), stream); }
    hipError_t end(hipStream_t stream) const { return hipEventRecord(ev1_.get(), stream); }
    hipError_t wait_ms(float *ms) const {
        const hipError_t e = hipEventSynchronize(ev1_.get());
        return e != hipSuccess ? e : hipEventElapsedTime(ms, ev0_.get(), ev1_.get());
    }
};

// ---- views: planes of one allocation, laid out by in() and made pointers by bind().  They own nothing. ----------------------
// Their copies are plain synchronous ones, the runtime's fast path for pageable memory, in the order written; a NULL pointer on
// either side skips its plane.
struct PlaneCopy {
    void *dst;
    const void *src;
    size_t bytes;
};
inline int copy_planes(hipMemcpyKind kind, std::initializer_list<PlaneCopy> planes, const char *what) {
    hipError_t e = hipSuccess;
    for (const PlaneCopy &c : planes)
        if (e == hipSuccess && c.dst && c.src) e = hipMemcpy(c.dst, c.src, c.bytes, kind);
    return hip_status(e, what);
}

// The accumulator triple sum[3 n] | sum2[3 n] | count[n].
struct AccumPlanes {
    float *sum = nullptr, *sum2 = nullptr;
    int32_t *count = nullptr;
    size_t n = 0;
    size_t offset[3] = {0, 0, 0};   // of the planes in their layout (in), until bind() makes pointers of them
    static AccumPlanes in(PlaneLayout &l, size_t n) {
        AccumPlanes a;
        a.n = n;
        for (int k = 0; k < 3; ++k) a.offset[k] = l.add((k < 2 ? 12 : 4) * n);
        return a;
    }
    void bind(const DeviceBuffer &b) { sum = b.at<float>(offset[0]); sum2 = b.at<float>(offset[1]); count = b.at<int32_t>(offset[2]); }
    int upload(const float *s, const float *s2, const int32_t *c) const {
        return copy_planes(hipMemcpyHostToDevice, {{sum, s, 12 * n}, {sum2, s2, 12 * n}, {count, c, 4 * n}}, "copy of the accumulator planes");
    }
    int download(float *s, float *s2, int32_t *c) const {
        return copy_planes(hipMemcpyDeviceToHost, {{s, sum, 12 * n}, {s2, sum2, 12 * n}, {c, count, 4 * n}}, "copy of the accumulator planes");
    }
};

// A mean image and its count, rgb[3 n] | count[n]: what the filters write and the display, the meter and bloom read.
struct MeanPlanes {
    float *rgb = nullptr;
    int32_t *count = nullptr;
    size_t n = 0;
    size_t offset[2] = {0, 0};
    static MeanPlanes in(PlaneLayout &l, size_t n) {
        MeanPlanes m;
        m.n = n;
        m.offset[0] = l.add(12 * n);
        m.offset[1] = l.add(4 * n);
        return m;
    }
    void bind(const DeviceBuffer &b) { rgb = b.at<float>(offset[0]); count = b.at<int32_t>(offset[1]); }
    int upload(const float *m, const int32_t *c) const { return copy_planes(hipMemcpyHostToDevice, {{rgb, m, 12 * n}, {count, c, 4 * n}}, "copy of a mean image"); }
    int download(float *m, int32_t *c) const { return copy_planes(hipMemcpyDeviceToHost, {{m, rgb, 12 * n}, {c, count, 4 * n}}, "copy of a mean image"); }
};

// The first hits of a view: the centre rays' origins and directions, the hit's position, normal and albedo (3 floats per pixel
// each), the hit's index and its t.  in() lays out all seven; uploaded_in() the four a filter reads, for an entry point whose
// caller brings them (the other three stay NULL).
struct FeaturePlanes {
    float *origins = nullptr, *directions = nullptr, *position = nullptr, *normal = nullptr, *albedo = nullptr, *hit_t = nullptr;
    int32_t *hit = nullptr;
    size_t n = 0;
    bool traced = false;   // origins, directions and hit_t are laid out too
    size_t offset[7] = {0, 0, 0, 0, 0, 0, 0};   // position, normal, albedo, hit; origins, directions, hit_t
    static FeaturePlanes uploaded_in(PlaneLayout &l, size_t n) {
        FeaturePlanes f;
        f.n = n;
        for (int k = 0; k < 4; ++k) f.offset[k] = l.add((k < 3 ? 12 : 4) * n);
        return f;
    }
    static FeaturePlanes in(PlaneLayout &l, size_t n) {
        FeaturePlanes f = uploaded_in(l, n);
        f.traced = true;
        for (int k = 4; k < 7; ++k) f.offset[k] = l.add((k < 6 ? 12 : 4) * n);
        return f;
    }
    void bind(const DeviceBuffer &b) {
        position = b.at<float>(offset[0]); normal = b.at<float>(offset[1]); albedo = b.at<float>(offset[2]); hit = b.at<int32_t>(offset[3]);
        if (traced) origins = b.at<float>(offset[4]), directions = b.at<float>(offset[5]), hit_t = b.at<float>(offset[6]);
    }
    int upload(const float *p, const float *nrm, const float *alb, const int32_t *h) const {
        return copy_planes(hipMemcpyHostToDevice, {{position, p, 12 * n}, {normal, nrm, 12 * n}, {albedo, alb, 12 * n}, {hit, h, 4 * n}},
                           "copy of the feature planes");
    }
    int download(const FeaturePlanes &host) const {   // the same planes in host memory, NULL where the caller wants none
        return copy_planes(hipMemcpyDeviceToHost, {{host.hit, hit, 4 * n}, {host.hit_t, hit_t, 4 * n}, {host.position, position, 12 * n},
                                                   {host.normal, normal, 12 * n}, {host.albedo, albedo, 12 * n}}, "copy of the feature planes");
    }
};

// What the denoiser works in: records A0, A1, B, C (16 bytes per pixel each) and the mean image it writes.
struct DenoisePlanes {
    void *rec_a0 = nullptr, *rec_a1 = nullptr, *rec_b = nullptr, *rec_c = nullptr;
    MeanPlanes out;
    size_t offset[4] = {0, 0, 0, 0};
    static DenoisePlanes in(PlaneLayout &l, size_t n) {
        DenoisePlanes w;
        for (size_t &o : w.offset) o = l.add(16 * n);
        w.out = MeanPlanes::in(l, n);
        return w;
    }
    void bind(const DeviceBuffer &b) {
        rec_a0 = b.at<void>(offset[0]); rec_a1 = b.at<void>(offset[1]); rec_b = b.at<void>(offset[2]); rec_c = b.at<void>(offset[3]);
        out.bind(b);
    }
};

// What the upsampler works in, per pixel of the LOW image: records A, B, C (16 bytes each) and, where the caller's low image
// is accumulators still (own_mean), the plane of their mean.
struct UpsamplePlanes {
    void *rec_a = nullptr, *rec_b = nullptr, *rec_c = nullptr;
    float *mean_lo = nullptr;
    size_t n_lo = 0;
    bool own_mean = false;
    size_t offset[4] = {0, 0, 0, 0};
    static UpsamplePlanes in(PlaneLayout &l, size_t n_lo, bool own_mean) {
        UpsamplePlanes w;
        w.n_lo = n_lo;
        w.own_mean = own_mean;
        for (int k = 0; k < (own_mean ? 4 : 3); ++k) w.offset[k] = l.add((k < 3 ? 16 : 12) * n_lo);
        return w;
    }
    void bind(const DeviceBuffer &b) {
        rec_a = b.at<void>(offset[0]); rec_b = b.at<void>(offset[1]); rec_c = b.at<void>(offset[2]);
        if (own_mean) mean_lo = b.at<float>(offset[3]);
    }
};

// What bloom works in: the plane of bloomed means it writes and the pyramid, `records` records of 16 bytes -- what
// pt::bloom_pyramid_records gives for the image and the levels; the caller's to ask, this header knows no kernel's.
struct BloomPlanes {
    float *out_rgb = nullptr;
    void *pyramid = nullptr;
    size_t n = 0;
    size_t offset[2] = {0, 0};
    static BloomPlanes in(PlaneLayout &l, size_t n, size_t records) {
        BloomPlanes w;
        w.n = n; w.offset[0] = l.add(12 * n); w.offset[1] = l.add(16 * records);
        return w;
    }
    void bind(const DeviceBuffer &b) { out_rgb = b.at<float>(offset[0]); pyramid = b.at<void>(offset[1]); }
};

// What local exposure works in: the plane of locally exposed means it writes and the two planes of the base (a float per pixel each).
struct LocalPlanes {
    float *out_rgb = nullptr, *base[2] = {nullptr, nullptr};
    size_t n = 0;
    size_t offset[3] = {0, 0, 0};
    static LocalPlanes in(PlaneLayout &l, size_t n) {
        LocalPlanes w;
        w.n = n;
        for (int k = 0; k < 3; ++k) w.offset[k] = l.add((k < 1 ? 12 : 4) * n);
        return w;
    }
    void bind(const DeviceBuffer &b) { out_rgb = b.at<float>(offset[0]); base[0] = b.at<float>(offset[1]); base[1] = b.at<float>(offset[2]); }
};

// What sharpening works in: the plane of compressed luminance (a float per pixel) and, where the image it is given is not a plane of
// its caller's own (own_mean), the plane of sharpened means it writes.
struct SharpenPlanes {
    float *luma = nullptr, *out_rgb = nullptr;
    size_t n = 0;
    bool own_mean = false;
    size_t offset[2] = {0, 0};
    static SharpenPlanes in(PlaneLayout &l, size_t n, bool own_mean) {
        SharpenPlanes w;
        w.n = n; w.own_mean = own_mean;
        w.offset[0] = l.add(4 * n);
        if (own_mean) w.offset[1] = l.add(12 * n);
        return w;
    }
    void bind(const DeviceBuffer &b) {
        luma = b.at<float>(offset[0]);
        if (own_mean) out_rgb = b.at<float>(offset[1]);
    }
};

}  // namespace ptc
