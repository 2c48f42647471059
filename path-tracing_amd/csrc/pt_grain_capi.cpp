// Host side of film grain and dithered quantization (include/pt_hip.h: pt_grain_quantize): the parameter check every entry point with
// the stage shares, one pixel's bytes as the host makes them -- the host chain's and the display path's finish of a deferred pixel --
// and the host chain's last step.  The arithmetic is pt_grain.hpp's, the one copy the kernel uses too; the threshold table is the one
// the kernel is given.  Nothing here touches a device.
#include "pt_capi_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "pt_display_table.hpp"

using ptc::fail;
using ptc::guarded;

int ptc::grain_params_check(const pt_grain_params *p, GrainSetup &out) {
    if (!p) return fail(PT_ERR_INVALID_ARGUMENT, "grain: null params");
    if (!std::isfinite(p->strength) || p->strength < 0.0f || p->strength > 1.0f)
        return fail(PT_ERR_INVALID_ARGUMENT, "grain: strength must be finite and lie in 0 .. 1 (0 = no grain)");
    if (!std::isfinite(p->size) || (p->size != 0.0f && (p->size < 1.0f || p->size > pt::kGrainMaxSize)))
        return fail(PT_ERR_INVALID_ARGUMENT, "grain: size must be finite and lie in 1 .. 8 (0 = 1)");
    if (!std::isfinite(p->dither) || p->dither < 0.0f || p->dither > 1.0f)
        return fail(PT_ERR_INVALID_ARGUMENT, "grain: dither must be finite and lie in 0 .. 1 (0 = no dither)");
    GrainSetup s;
    s.on = p->strength > 0.0f || p->dither > 0.0f;
    s.step.strength = p->strength;
    s.step.size = p->size != 0.0f ? p->size : 1.0f;
    s.step.dither = p->dither;
    s.step.seed = p->seed;
    s.step.frame = p->frame;
    s.step.width = 0;
    out = s;
    return PT_OK;
}

void ptc::grain_pixel_bytes(const pt::GrainStep &s, const DisplayTable &table, float gamma, uint32_t x, uint32_t y, const float *g, uint8_t *rgb) {
    float v[3] = {g[0], g[1], g[2]};
    pt::grain_pixel(s, x, y, v[0], v[1], v[2]);
    uint32_t word[3] = {0u, 0u, 0u};
    if (s.dither != 0.0f) pt::grain_dither_words(s, x, y, word[0], word[1], word[2]);
    const std::vector<float> &T = table.thresholds;
    const float last = T.empty() ? 0.0f : T.back();
    for (int k = 0; k < 3; ++k) {
        bool covered = v[k] >= 0.0f && v[k] < last;
        for (size_t b = 0; covered && b < table.band_lo.size(); ++b) covered = !(v[k] >= table.band_lo[b] && v[k] < table.band_hi[b]);
        if (!covered) {   // negative, NaN, at or above the last threshold, or in a doubt band: the host's own two steps
            rgb[k] = quantize_value(tonemap_value(v[k], gamma));
            continue;
        }
        uint32_t level = static_cast<uint32_t>(std::upper_bound(T.begin(), T.end(), v[k]) - T.begin());   // thresholds <= v; below T.size()
        if (s.dither != 0.0f) level = pt::grain_dither_level(level, level ? T[level - 1] : 0.0f, T[level], v[k], s.dither, word[k]);
        rgb[k] = static_cast<uint8_t>(level & 255u);
    }
}

namespace {

int grain_quantize_impl(int32_t width, int32_t height, const float *graded_rgb, const int32_t *count, float gamma, const pt_grain_params *n,
                        uint8_t *bgr) {
    if (width <= 0 || height <= 0 || !graded_rgb || !count || !bgr) return fail(PT_ERR_INVALID_ARGUMENT, "grain: null buffer or empty image");
    int rc = ptc::check_image_size(width, height, "grain: ");
    if (rc != PT_OK) return rc;
    if (!std::isfinite(gamma) || !(gamma > 0.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "grain: gamma must be finite and > 0");
    ptc::GrainSetup setup;
    if ((rc = ptc::grain_params_check(n, setup)) != PT_OK) return rc;
    const size_t pixels = static_cast<size_t>(width) * height;
    std::memset(bgr, 0, 3 * pixels);
    if (!setup.on) {   // pt_tonemap -> pt_quantize, in their own words
        for (size_t p = 0; p < pixels; ++p)
            for (int k = 0; count[p] && k < 3; ++k) bgr[3 * p + k] = ptc::quantize_value(ptc::tonemap_value(graded_rgb[3 * p + 2 - k], gamma));
        return PT_OK;
    }
    setup.step.width = width;
    const std::shared_ptr<const ptc::DisplayTable> table = ptc::display_table(gamma);
    size_t p = 0;
    for (int32_t y = 0; y < height; ++y)
        for (int32_t x = 0; x < width; ++x, ++p) {
            if (!count[p]) continue;
            uint8_t rgb[3];
            ptc::grain_pixel_bytes(setup.step, *table, gamma, static_cast<uint32_t>(x), static_cast<uint32_t>(y), graded_rgb + 3 * p, rgb);
            bgr[3 * p] = rgb[2]; bgr[3 * p + 1] = rgb[1]; bgr[3 * p + 2] = rgb[0];
        }
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_grain_quantize(int32_t width, int32_t height, const float *graded_rgb, const int32_t *count, float gamma, const pt_grain_params *n,
                      uint8_t *bgr) {
    return guarded([&] { return grain_quantize_impl(width, height, graded_rgb, count, gamma, n, bgr); });
}

}  // extern "C"
