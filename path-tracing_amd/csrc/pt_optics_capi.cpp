// Host side of the lens optics stage (include/pt_hip.h: pt_optics_host): the parameter check every entry point with the stage
// shares, and the kernel alone on a host image.  The arithmetic is pt_optics.hip's; there is no host copy of it (the suite restates
// the header in numpy).
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstring>

using ptc::fail;
using ptc::guarded;
using ptc::hip_fail;

int ptc::optics_params_check(const pt_optics_params *o, OpticsSetup &out) {
    if (!o) return fail(PT_ERR_INVALID_ARGUMENT, "optics: null params");
    auto within = [](float v, float lo, float hi) { return std::isfinite(v) && v >= lo && v <= hi; };
    if (!within(o->k1, -4.0f, 4.0f) || !within(o->k2, -4.0f, 4.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "optics: k1 and k2 must be finite and lie in -4 .. 4");
    if (!within(o->ca, -0.25f, 0.25f)) return fail(PT_ERR_INVALID_ARGUMENT, "optics: ca must be finite and lie in -0.25 .. 0.25");
    if (!within(o->vignette, 0.0f, 64.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "optics: vignette must be finite and lie in 0 .. 64");
    OpticsSetup s;
    s.on = o->k1 != 0.0f || o->k2 != 0.0f || o->ca != 0.0f || o->vignette != 0.0f;
    s.k1 = o->k1; s.k2 = o->k2; s.vignette = o->vignette;
    s.mag[0] = 1.0f - o->ca; s.mag[1] = 1.0f; s.mag[2] = 1.0f + o->ca;
    out = s;
    return PT_OK;
}

namespace {

// [a, a + na) and [b, b + nb) share a byte.
bool overlap(const void *a, size_t na, const void *b, size_t nb) {
    const char *pa = static_cast<const char *>(a), *pb = static_cast<const char *>(b);
    return pa < pb + nb && pb < pa + na;
}

int optics_host_impl(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, const pt_optics_params *p,
                     float *out_rgb, int32_t *out_count, float *kernel_ms) {
    if (width <= 0 || height <= 0 || !mean_rgb || !count || !out_rgb || !out_count) return fail(PT_ERR_INVALID_ARGUMENT, "optics: null buffer or empty image");
    int rc = ptc::check_image_size(width, height, "optics: ");
    if (rc != PT_OK) return rc;
    const size_t n = static_cast<size_t>(width) * height;
    if (overlap(out_rgb, 12 * n, mean_rgb, 12 * n) || overlap(out_rgb, 12 * n, count, 4 * n) || overlap(out_count, 4 * n, count, 4 * n) ||
        overlap(out_count, 4 * n, mean_rgb, 12 * n) || overlap(out_rgb, 12 * n, out_count, 4 * n))
        return fail(PT_ERR_INVALID_ARGUMENT, "optics: the stage is a gather: an output buffer must not overlap an input or the other output");
    ptc::OpticsSetup setup;
    if ((rc = ptc::optics_params_check(p, setup)) != PT_OK) return rc;
    if (kernel_ms) *kernel_ms = 0.0f;
    if ((rc = ptc::use_device(device, "optics")) != PT_OK) return rc;
    if (!setup.on) {
        std::memcpy(out_rgb, mean_rgb, 12 * n);
        std::memcpy(out_count, count, 4 * n);
        return PT_OK;
    }
    ptc::PlaneLayout l;
    ptc::MeanPlanes in = ptc::MeanPlanes::in(l, n), out = ptc::MeanPlanes::in(l, n);
    ptc::DeviceBuffer d;
    if ((rc = d.alloc(l, "pt_optics_host")) != PT_OK) return rc;
    in.bind(d); out.bind(d);
    if ((rc = in.upload(mean_rgb, count)) != PT_OK) return rc;
    const auto a = ptc::optics_args(setup, {in.rgb, in.count, false, width, height}, out);
    float ms = 0.0f;
    if ((rc = ptc::timed(nullptr, "pt_optics_host", &ms, [&]() -> int { PT_HIP_TRY(pt::launch_optics(a, nullptr)); return PT_OK; })) != PT_OK) return rc;
    if ((rc = out.download(out_rgb, out_count)) != PT_OK) return rc;
    if (kernel_ms) *kernel_ms = ms;
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_optics_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, const pt_optics_params *o,
                   float *out_rgb, int32_t *out_count, float *kernel_ms) {
    return guarded([&] { return optics_host_impl(device, width, height, mean_rgb, count, o, out_rgb, out_count, kernel_ms); });
}

}  // extern "C"
