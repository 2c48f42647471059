// Host side of local exposure (include/pt_hip.h: pt_local_host): the parameter check every entry point with the stage shares, and
// the kernels alone on a host image.  The arithmetic is pt_local.hip's; there is no host copy of it (the suite restates the header
// in numpy).
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstring>

using ptc::fail;
using ptc::guarded;
using ptc::hip_fail;

static_assert(PT_LOCAL_MAX_LEVELS == pt::kLocalMaxLevels, "the ABI header states the deepest base");

int ptc::local_params_check(const pt_local_params *l, LocalSetup &out) {
    if (!l) return fail(PT_ERR_INVALID_ARGUMENT, "local: null params");
    auto bad = [](float v) { return !std::isfinite(v) || v < 0.0f; };
    if (bad(l->strength) || bad(l->pivot) || bad(l->sigma))
        return fail(PT_ERR_INVALID_ARGUMENT, "local: strength must be finite and not negative, pivot and sigma finite and > 0 (0 = the default)");
    if (l->levels < 0 || l->levels > pt::kLocalMaxLevels) return fail(PT_ERR_INVALID_ARGUMENT, "local: levels must lie in 1 .. 8 (0 = 5)");
    LocalSetup s;
    s.on = l->strength > 0.0f;
    s.strength = l->strength;
    s.pivot = l->pivot > 0.0f ? l->pivot : 0.18f;
    s.levels = l->levels > 0 ? l->levels : 5;
    s.sigma = l->sigma > 0.0f ? l->sigma : 0.5f;
    out = s;
    return PT_OK;
}

namespace {

int local_host_impl(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure, const pt_local_params *p,
                    float *out_rgb, float *kernel_ms) {
    if (width <= 0 || height <= 0 || !mean_rgb || !count || !out_rgb) return fail(PT_ERR_INVALID_ARGUMENT, "local: null buffer or empty image");
    int rc = ptc::check_image_size(width, height, "local: ");
    if (rc != PT_OK) return rc;
    if (!std::isfinite(exposure) || !(exposure > 0.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "local: exposure must be finite and > 0");
    ptc::LocalSetup setup;
    if ((rc = ptc::local_params_check(p, setup)) != PT_OK) return rc;
    if (kernel_ms) *kernel_ms = 0.0f;
    if ((rc = ptc::use_device(device, "local")) != PT_OK) return rc;
    const size_t n = static_cast<size_t>(width) * height;
    if (!setup.on) {
        if (out_rgb != mean_rgb) std::memmove(out_rgb, mean_rgb, 12 * n);
        return PT_OK;
    }
    ptc::PlaneLayout l;
    ptc::MeanPlanes in = ptc::MeanPlanes::in(l, n);
    const size_t o_e = l.add(4);
    ptc::LocalPlanes work = ptc::LocalPlanes::in(l, n);
    ptc::DeviceBuffer d;
    if ((rc = d.alloc(l, "pt_local_host")) != PT_OK) return rc;
    in.bind(d); work.bind(d);
    if ((rc = in.upload(mean_rgb, count)) != PT_OK) return rc;
    PT_HIP_TRY(hipMemcpy(d.at<void>(o_e), &exposure, 4, hipMemcpyHostToDevice));
    const auto a = ptc::local_args(setup, {in.rgb, in.count, false, width, height}, d.at<float>(o_e), work);
    float ms = 0.0f;
    if ((rc = ptc::timed(nullptr, "pt_local_host", &ms, [&]() -> int { PT_HIP_TRY(pt::launch_local(a, nullptr)); return PT_OK; })) != PT_OK) return rc;
    PT_HIP_TRY(hipMemcpy(out_rgb, a.out_rgb, 12 * n, hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = ms;
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_local_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure, const pt_local_params *p,
                  float *out_rgb, float *kernel_ms) {
    return guarded([&] { return local_host_impl(device, width, height, mean_rgb, count, exposure, p, out_rgb, kernel_ms); });
}

}  // extern "C"
