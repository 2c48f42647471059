// Host side of display grading (include/pt_hip.h: pt_grade_host, pt_meter_host, pt_exposure_from_histogram): the parameter check
// every graded entry point shares, the host chain's grade step, the rule from histogram to exposure, and the meter kernel alone
// on a host image.  The arithmetic is pt_grade.hpp's, the one copy the kernels use too.
#include "pt_capi_internal.hpp"

#include <cmath>

using ptc::fail;
using ptc::guarded;
using ptc::hip_fail;

static_assert(PT_CURVE_REFERENCE == pt::kCurveReference && PT_CURVE_CLAMP == pt::kCurveClamp && PT_CURVE_REINHARD == pt::kCurveReinhard &&
                  PT_CURVE_ACES == pt::kCurveAces && PT_METER_ENTRIES == pt::kMeterEntries,
              "the ABI header states the curves and the histogram's length");
static_assert(sizeof(pt_grade_info) == sizeof(pt::ExposureOut), "the exposure kernel writes what pt_grade_info reports");

int ptc::grade_params_check(const pt_grade_params *g, GradeSetup &out) {
    if (!g) return fail(PT_ERR_INVALID_ARGUMENT, "grade: null params");
    if (g->curve < 0 || g->curve >= pt::kCurveCount) return fail(PT_ERR_INVALID_ARGUMENT, "grade: unknown curve");
    auto bad = [](float v) { return !std::isfinite(v) || v < 0.0f; };
    if (bad(g->exposure)) return fail(PT_ERR_INVALID_ARGUMENT, "grade: exposure must be finite and not negative (0 = 1)");
    if (g->percentile < 0 || g->percentile > 100) return fail(PT_ERR_INVALID_ARGUMENT, "grade: percentile must lie in 1 .. 100 (0 = 50)");
    if (bad(g->key) || bad(g->e_min) || bad(g->e_max) || bad(g->rate))
        return fail(PT_ERR_INVALID_ARGUMENT, "grade: key, e_min, e_max and rate must be finite and not negative (0 = the default)");
    GradeSetup s;
    s.curve = g->curve;
    s.automatic = g->auto_exposure != 0;
    s.exposure = g->exposure > 0.0f ? g->exposure : 1.0f;
    s.rule.percentile = g->percentile > 0 ? g->percentile : 50;
    s.rule.key = g->key > 0.0f ? g->key : 0.18f;
    s.rule.e_min = g->e_min > 0.0f ? g->e_min : 0.00390625f;
    s.rule.e_max = g->e_max > 0.0f ? g->e_max : 256.0f;
    s.rule.rate = g->rate > 0.0f ? g->rate : 1.0f;
    if (s.rule.e_min > s.rule.e_max) return fail(PT_ERR_INVALID_ARGUMENT, "grade: e_min is above e_max");
    out = s;
    return PT_OK;
}

namespace {

int grade_host_impl(int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure, int32_t curve, float *out_rgb) {
    if (width <= 0 || height <= 0 || !mean_rgb || !count || !out_rgb) return fail(PT_ERR_INVALID_ARGUMENT, "grade: null buffer or empty image");
    if (curve < 0 || curve >= pt::kCurveCount) return fail(PT_ERR_INVALID_ARGUMENT, "grade: unknown curve");
    if (!std::isfinite(exposure) || !(exposure > 0.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "grade: exposure must be finite and > 0");
    const size_t n = static_cast<size_t>(width) * height;
    for (size_t p = 0; p < n; ++p)
        for (int k = 0; k < 3; ++k)
            out_rgb[3 * p + k] = count[p] ? pt::grade_value(curve, mean_rgb[3 * p + k], exposure) : mean_rgb[3 * p + k];
    return PT_OK;
}

int exposure_impl(const uint32_t *hist, const pt_grade_params *params, int32_t has_prev, float e_prev, float *e, float *e_target) {
    if (!hist || !e || !e_target) return fail(PT_ERR_INVALID_ARGUMENT, "exposure: null pointer");
    ptc::GradeSetup s;
    const int rc = ptc::grade_params_check(params, s);
    if (rc != PT_OK) return rc;
    pt::exposure_from_histogram(hist, s.rule, has_prev != 0, e_prev, e, e_target);
    return PT_OK;
}

int meter_host_impl(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, uint32_t *hist, float *kernel_ms) {
    if (width <= 0 || height <= 0 || !mean_rgb || !count || !hist) return fail(PT_ERR_INVALID_ARGUMENT, "meter: null buffer or empty image");
    int rc = ptc::check_image_size(width, height, "meter: ");
    if (rc != PT_OK) return rc;
    if (kernel_ms) *kernel_ms = 0.0f;
    if ((rc = ptc::use_device(device, "meter")) != PT_OK) return rc;
    const size_t n = static_cast<size_t>(width) * height;
    ptc::PlaneLayout l;
    ptc::MeanPlanes in = ptc::MeanPlanes::in(l, n);
    const size_t o_hist = l.add(4 * pt::kMeterEntries);
    ptc::DeviceBuffer d;
    if ((rc = d.alloc(l, "pt_meter_host")) != PT_OK) return rc;
    in.bind(d);
    if ((rc = in.upload(mean_rgb, count)) != PT_OK) return rc;
    PT_HIP_TRY(hipMemset(d.at<void>(o_hist), 0, 4 * pt::kMeterEntries));
    const auto a = ptc::meter_args({in.rgb, in.count, false, width, height}, d.at<uint32_t>(o_hist));
    float ms = 0.0f;
    if ((rc = ptc::timed(nullptr, "pt_meter_host", &ms, [&]() -> int { PT_HIP_TRY(pt::launch_meter(a, nullptr)); return PT_OK; })) != PT_OK) return rc;
    PT_HIP_TRY(hipMemcpy(hist, a.hist, 4 * pt::kMeterEntries, hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = ms;
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_grade_host(int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure, int32_t curve, float *out_rgb) {
    return guarded([&] { return grade_host_impl(width, height, mean_rgb, count, exposure, curve, out_rgb); });
}

int pt_exposure_from_histogram(const uint32_t *hist, const pt_grade_params *params, int32_t has_prev, float e_prev, float *e, float *e_target) {
    return guarded([&] { return exposure_impl(hist, params, has_prev, e_prev, e, e_target); });
}

int pt_meter_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, uint32_t *hist, float *kernel_ms) {
    return guarded([&] { return meter_host_impl(device, width, height, mean_rgb, count, hist, kernel_ms); });
}

}  // extern "C"
