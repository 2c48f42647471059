// Display grading (include/pt_hip.h: pt_grade_*, pt_meter_host, pt_exposure_from_histogram), the one copy of its arithmetic:
// the host chain (pt_grade_host, pt_exposure_from_histogram), the kernels (pt_display_graded.hip, pt_meter.hip) and the host's
// finishing of deferred pixels all call these functions.  Every step is one correctly rounded float operation in the order written
// (* / + -, comparisons) or integer arithmetic, so host and device agree bit for bit; nothing is fused.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PT_GRADE_FN __host__ __device__ inline
#else
#define PT_GRADE_FN inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pt {

// pt_hip.h: PT_CURVE_*
constexpr int kCurveReference = 0, kCurveClamp = 1, kCurveReinhard = 2, kCurveAces = 3, kCurveCount = 4;

// The luminance histogram: quarter-octave bins from 2^-16 to 2^16, and one more for "dark" (not above zero, or NaN).
constexpr int kMeterBins = 128, kMeterDark = 128, kMeterEntries = 129;
constexpr uint32_t kMeterFirstIndex = 444;   // bits(2^-16) >> 21

PT_GRADE_FN uint32_t grade_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u;
    std::memcpy(&u, &f, sizeof u);
    return u;
#endif
}
PT_GRADE_FN float grade_from_bits(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
#endif
}

// g = curve(m * e), one channel.
template <int CURVE>
PT_GRADE_FN float grade_value(float m, float e) {
    const float x = m * e;
    if (CURVE == kCurveClamp) return x > 1.0f ? 1.0f : x;
    if (CURVE == kCurveReinhard) return x / (1.0f + x);
    if (CURVE == kCurveAces) {
        const float a = x * ((2.51f * x) + 0.03f);
        const float b = (x * ((2.43f * x) + 0.59f)) + 0.14f;
        const float g = a / b;
        return g > 1.0f ? 1.0f : g;
    }
    return x;
}
PT_GRADE_FN float grade_value(int curve, float m, float e) {
    switch (curve) {
        case kCurveClamp: return grade_value<kCurveClamp>(m, e);
        case kCurveReinhard: return grade_value<kCurveReinhard>(m, e);
        case kCurveAces: return grade_value<kCurveAces>(m, e);
        default: return grade_value<kCurveReference>(m, e);
    }
}

// The denoiser's lum.
PT_GRADE_FN float meter_luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// The histogram entry of a luminance: kMeterDark unless l > 0; else the exponent and two mantissa bits, from 2^-16 on, clamped.
PT_GRADE_FN int meter_bin(float l) {
    if (!(l > 0.0f)) return kMeterDark;
    const uint32_t idx = grade_bits(l) >> 21;
    if (idx < kMeterFirstIndex) return 0;
    const uint32_t bin = idx - kMeterFirstIndex;
    return bin > static_cast<uint32_t>(kMeterBins - 1) ? kMeterBins - 1 : static_cast<int>(bin);
}
// The lower edge of bin b.
PT_GRADE_FN float meter_edge(int b) { return grade_from_bits((static_cast<uint32_t>(b) + kMeterFirstIndex) << 21); }

// pt_grade_params' metering fields with the defaults filled in (pt_grade_capi.cpp checks them first).
struct ExposureRule {
    int32_t percentile;
    float key, e_min, e_max, rate;
};

// The exposure of a metered present: *target = e*, *e = what the display kernel multiplies by.
PT_GRADE_FN void exposure_from_histogram(const uint32_t *hist, const ExposureRule &r, bool has_prev, float e_prev, float *e, float *target) {
    uint64_t total = 0;
    for (int b = 0; b < kMeterBins; ++b) total += hist[b];
    float t;
    if (total == 0) {
        t = has_prev ? e_prev : 1.0f;
    } else {
        const uint64_t want = static_cast<uint64_t>(r.percentile) * total;
        uint64_t cum = 0;
        int bp = kMeterBins - 1;
        for (int b = 0; b < kMeterBins; ++b) {
            cum += hist[b];
            if (100u * cum >= want) {
                bp = b;
                break;
            }
        }
        t = r.key / meter_edge(bp);
        t = t < r.e_min ? r.e_min : (t > r.e_max ? r.e_max : t);
    }
    *target = t;
    if (!has_prev || r.rate >= 1.0f) *e = t;
    else *e = e_prev + (t - e_prev) * r.rate;
}

}  // namespace pt
