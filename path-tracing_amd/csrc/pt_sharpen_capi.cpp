// Host side of sharpening (include/pt_hip.h: pt_sharpen_host): the parameter check every entry point with the stage shares, and the
// kernels alone on a host image.  The arithmetic is pt_sharpen.hip's; there is no host copy of it (the suite restates the header in
// numpy).
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstring>

using ptc::fail;
using ptc::guarded;
using ptc::hip_fail;

int ptc::sharpen_params_check(const pt_sharpen_params *p, SharpenSetup &out) {
    if (!p) return fail(PT_ERR_INVALID_ARGUMENT, "sharpen: null params");
    if (!std::isfinite(p->strength) || p->strength < 0.0f || p->strength > 1.0f)
        return fail(PT_ERR_INVALID_ARGUMENT, "sharpen: strength must be finite and lie in 0 .. 1 (0 = the stage is not run)");
    if (!std::isfinite(p->limit) || p->limit < 0.0f || p->limit > pt::kSharpenMaxLimit)
        return fail(PT_ERR_INVALID_ARGUMENT, "sharpen: limit must be finite and lie in 0 .. 0.1875 (0 = 0.1875)");
    SharpenSetup s;
    s.on = p->strength > 0.0f;
    s.strength = p->strength;
    s.limit = p->limit > 0.0f ? p->limit : pt::kSharpenMaxLimit;
    out = s;
    return PT_OK;
}

namespace {

int sharpen_host_impl(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure,
                      const pt_sharpen_params *p, float *out_rgb, float *kernel_ms) {
    if (width <= 0 || height <= 0 || !mean_rgb || !count || !out_rgb) return fail(PT_ERR_INVALID_ARGUMENT, "sharpen: null buffer or empty image");
    int rc = ptc::check_image_size(width, height, "sharpen: ");
    if (rc != PT_OK) return rc;
    if (!std::isfinite(exposure) || !(exposure > 0.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "sharpen: exposure must be finite and > 0");
    ptc::SharpenSetup setup;
    if ((rc = ptc::sharpen_params_check(p, setup)) != PT_OK) return rc;
    if (kernel_ms) *kernel_ms = 0.0f;
    if ((rc = ptc::use_device(device, "sharpen")) != PT_OK) return rc;
    const size_t n = static_cast<size_t>(width) * height;
    if (!setup.on) {
        if (out_rgb != mean_rgb) std::memmove(out_rgb, mean_rgb, 12 * n);
        return PT_OK;
    }
    ptc::PlaneLayout l;
    ptc::MeanPlanes in = ptc::MeanPlanes::in(l, n);
    const size_t o_e = l.add(4);
    const bool in_place = out_rgb == mean_rgb;   // the kernels then write the plane they read, as the caller's image is
    ptc::SharpenPlanes work = ptc::SharpenPlanes::in(l, n, !in_place);
    ptc::DeviceBuffer d;
    if ((rc = d.alloc(l, "pt_sharpen_host")) != PT_OK) return rc;
    in.bind(d); work.bind(d);
    if ((rc = in.upload(mean_rgb, count)) != PT_OK) return rc;
    PT_HIP_TRY(hipMemcpy(d.at<void>(o_e), &exposure, 4, hipMemcpyHostToDevice));
    const auto a = ptc::sharpen_args(setup, {in.rgb, in.count, false, width, height}, d.at<float>(o_e), work, in_place ? in.rgb : work.out_rgb);
    float ms = 0.0f;
    if ((rc = ptc::timed(nullptr, "pt_sharpen_host", &ms, [&]() -> int { PT_HIP_TRY(pt::launch_sharpen(a, nullptr)); return PT_OK; })) != PT_OK) return rc;
    PT_HIP_TRY(hipMemcpy(out_rgb, a.out_rgb, 12 * n, hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = ms;
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_sharpen_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure, const pt_sharpen_params *p,
                    float *out_rgb, float *kernel_ms) {
    return guarded([&] { return sharpen_host_impl(device, width, height, mean_rgb, count, exposure, p, out_rgb, kernel_ms); });
}

}  // extern "C"
