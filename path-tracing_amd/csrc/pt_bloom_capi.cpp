// Host side of bloom (include/pt_hip.h: pt_bloom_host): the parameter check every bloomed entry point shares, and the kernels alone
// on a host image.  The arithmetic is pt_bloom.hip's; there is no host copy of it (the suite restates the header in numpy).
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstring>

using ptc::fail;
using ptc::guarded;
using ptc::hip_fail;

static_assert(PT_BLOOM_MAX_LEVELS == pt::kBloomMaxLevels, "the ABI header states the deepest pyramid");

int ptc::bloom_params_check(const pt_bloom_params *b, BloomSetup &out) {
    if (!b) return fail(PT_ERR_INVALID_ARGUMENT, "bloom: null params");
    auto bad = [](float v) { return !std::isfinite(v) || v < 0.0f; };
    if (bad(b->strength) || bad(b->threshold)) return fail(PT_ERR_INVALID_ARGUMENT, "bloom: strength and threshold must be finite and not negative");
    if (b->levels < 0 || b->levels > pt::kBloomMaxLevels) return fail(PT_ERR_INVALID_ARGUMENT, "bloom: levels must lie in 1 .. 8 (0 = 5)");
    BloomSetup s;
    s.on = b->strength > 0.0f;
    s.threshold = b->threshold > 0.0f ? b->threshold : 1.0f;
    s.levels = b->levels > 0 ? b->levels : 5;
    s.weight = b->strength / static_cast<float>(s.levels);
    out = s;
    return PT_OK;
}

namespace {

int bloom_host_impl(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure, const pt_bloom_params *b,
                    float *out_rgb, float *kernel_ms) {
    if (width <= 0 || height <= 0 || !mean_rgb || !count || !out_rgb) return fail(PT_ERR_INVALID_ARGUMENT, "bloom: null buffer or empty image");
    int rc = ptc::check_image_size(width, height, "bloom: ");
    if (rc != PT_OK) return rc;
    if (!std::isfinite(exposure) || !(exposure > 0.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "bloom: exposure must be finite and > 0");
    ptc::BloomSetup setup;
    if ((rc = ptc::bloom_params_check(b, setup)) != PT_OK) return rc;
    if (kernel_ms) *kernel_ms = 0.0f;
    if ((rc = ptc::use_device(device, "bloom")) != PT_OK) return rc;
    const size_t n = static_cast<size_t>(width) * height;
    if (!setup.on) {
        if (out_rgb != mean_rgb) std::memmove(out_rgb, mean_rgb, 12 * n);
        return PT_OK;
    }
    ptc::PlaneLayout l;
    ptc::MeanPlanes in = ptc::MeanPlanes::in(l, n);
    const size_t o_e = l.add(4);
    ptc::BloomPlanes work = ptc::BloomPlanes::in(l, n, pt::bloom_pyramid_records(width, height, setup.levels));
    ptc::DeviceBuffer d;
    if ((rc = d.alloc(l, "pt_bloom_host")) != PT_OK) return rc;
    in.bind(d); work.bind(d);
    if ((rc = in.upload(mean_rgb, count)) != PT_OK) return rc;
    PT_HIP_TRY(hipMemcpy(d.at<void>(o_e), &exposure, 4, hipMemcpyHostToDevice));
    const auto a = ptc::bloom_args(setup, {in.rgb, in.count, false, width, height}, d.at<float>(o_e), work);
    float ms = 0.0f;
    if ((rc = ptc::timed(nullptr, "pt_bloom_host", &ms, [&]() -> int { PT_HIP_TRY(pt::launch_bloom(a, nullptr)); return PT_OK; })) != PT_OK) return rc;
    PT_HIP_TRY(hipMemcpy(out_rgb, a.out_rgb, 12 * n, hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = ms;
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_bloom_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure, const pt_bloom_params *b,
                  float *out_rgb, float *kernel_ms) {
    return guarded([&] { return bloom_host_impl(device, width, height, mean_rgb, count, exposure, b, out_rgb, kernel_ms); });
}

}  // extern "C"
