// Owners of what the host layer holds on a device: one hipMalloc, one event, one stream -- and the one spelling of "one
// allocation cut into 256-byte aligned planes".  Host only; nothing here is part of the ABI.
// An owner frees in its destructor, on whatever device is current: the handle that holds it (pt_scene, pt_session, pt_frame,
// pt_temporal) makes its own device current first -- in its destructor's body, which runs before the members go.  An empty
// owner (default constructed, moved from, reset) makes no HIP call, so a scene without a device never touches the runtime.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdint>
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
// How every alloc / create ends: the new handle counted, or the owner left empty and the error reported.
template <class H>
int created(hipError_t e, H &handle, const char *what) {
    if (e == hipSuccess) count_live(1);
    else handle = nullptr;
    return e == hipSuccess ? static_cast<int>(PT_OK) : hip_fail(e, what);
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
        const hipError_t e = hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        return e == hipSuccess ? static_cast<int>(PT_OK) : hip_fail(e, what);
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

// The accumulator triple sum[3 n] | sum2[3 n] | count[n]: a view, it owns nothing.
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
    // Plain synchronous copies: the runtime's fast path for pageable memory.  A NULL host pointer skips its plane.
    int upload(const float *s, const float *s2, const int32_t *c) const { return copy(sum, s, sum2, s2, count, c, hipMemcpyHostToDevice); }
    int download(float *s, float *s2, int32_t *c) const { return copy(s, sum, s2, sum2, c, count, hipMemcpyDeviceToHost); }

private:
    int copy(void *d0, const void *s0, void *d1, const void *s1, void *d2, const void *s2, hipMemcpyKind kind) const {
        hipError_t e = d0 && s0 ? hipMemcpy(d0, s0, 12 * n, kind) : hipSuccess;
        if (e == hipSuccess && d1 && s1) e = hipMemcpy(d1, s1, 12 * n, kind);
        if (e == hipSuccess && d2 && s2) e = hipMemcpy(d2, s2, 4 * n, kind);
        return e == hipSuccess ? static_cast<int>(PT_OK) : hip_fail(e, "copy of the accumulator planes");
    }
};

}  // namespace ptc
