// Host side of scene-linear output (include/pt_hip.h: pt_linear_*): the parameter check every entry point with the stage shares, the
// definition of the bytes (pt_linear_encode) and the two file writers.  The arithmetic is pt_linear.hpp's, the one copy the kernel uses
// too.  Nothing here touches a device: the entry points that launch the kernel are pt_display_capi.cpp's.
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

using ptc::fail;
using ptc::guarded;

int ptc::linear_params_check(const pt_linear_params *p, LinearSetup &out) {
    if (!p) return fail(PT_ERR_INVALID_ARGUMENT, "linear: null params");
    if (p->format != 0 && p->format != PT_LINEAR_PFM && p->format != PT_LINEAR_RGBE)
        return fail(PT_ERR_INVALID_ARGUMENT, "linear: format must be PT_LINEAR_PFM (1) or PT_LINEAR_RGBE (2) (0 = no linear output)");
    if (p->exposed != 0 && p->exposed != 1) return fail(PT_ERR_INVALID_ARGUMENT, "linear: exposed must be 0 or 1");
    LinearSetup s;
    s.on = p->format != 0;
    s.format = p->format;
    s.exposed = p->exposed != 0;
    out = s;
    return PT_OK;
}

int ptc::linear_image_check(int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure, const pt_linear_params *lin,
                            const uint8_t *out, LinearSetup &setup) {
    if (width <= 0 || height <= 0 || !mean_rgb || !count || !out) return fail(PT_ERR_INVALID_ARGUMENT, "linear: null buffer or empty image");
    int rc = check_image_size(width, height, "linear: ");
    if (rc != PT_OK || (rc = linear_params_check(lin, setup)) != PT_OK) return rc;
    if (!setup.on) return fail(PT_ERR_INVALID_ARGUMENT, "linear: format 0 encodes nothing; it must be PT_LINEAR_PFM (1) or PT_LINEAR_RGBE (2)");
    if (setup.exposed && (!std::isfinite(exposure) || !(exposure > 0.0f))) return fail(PT_ERR_INVALID_ARGUMENT, "linear: exposure must be finite and > 0");
    return PT_OK;
}

namespace {

bool valid_size(int32_t width, int32_t height) { return width > 0 && height > 0 && static_cast<long long>(width) * height <= 0x7fffffffLL / 4; }

int linear_encode_impl(int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure, const pt_linear_params *lin,
                       uint8_t *out) {
    ptc::LinearSetup setup;
    const int rc = ptc::linear_image_check(width, height, mean_rgb, count, exposure, lin, out, setup);
    if (rc != PT_OK) return rc;
    const size_t w = static_cast<size_t>(width), h = static_cast<size_t>(height);
    for (size_t y = 0; y < h; ++y)
        for (size_t x = 0; x < w; ++x) {
            const size_t p = y * w + x;
            uint32_t word[3] = {0u, 0u, 0u};   // PFM: the three floats' bits; RGBE: word[0] is the pixel
            if (count[p]) {
                float v[3];
                for (int k = 0; k < 3; ++k) v[k] = pt::linear_value(mean_rgb[3 * p + k], setup.exposed, exposure);
                if (setup.format == PT_LINEAR_RGBE) word[0] = pt::linear_rgbe(v[0], v[1], v[2]);
                else for (int k = 0; k < 3; ++k) word[k] = pt::grade_bits(v[k]);
            }
            const int words = setup.format == PT_LINEAR_RGBE ? 1 : 3;
            uint8_t *at = out + (setup.format == PT_LINEAR_RGBE ? 4 * p : 12 * ((h - 1 - y) * w + x));
            for (int k = 0; k < words; ++k)
                for (int b = 0; b < 4; ++b) at[4 * k + b] = static_cast<uint8_t>(word[k] >> (8 * b));
        }
    return PT_OK;
}

int write_picture(const char *path, int32_t width, int32_t height, const uint8_t *body, int32_t format) {
    if (!path || !body || !valid_size(width, height)) return fail(PT_ERR_INVALID_ARGUMENT, "linear: null argument, or an empty or too large image");
    char header[96];
    const int len = format == PT_LINEAR_PFM ? std::snprintf(header, sizeof header, "PF\n%d %d\n-1.0\n", width, height)
                                            : std::snprintf(header, sizeof header, "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n", height, width);
    FILE *f = std::fopen(path, "wb");
    if (!f) return fail(PT_ERR_IO, std::string("cannot open ") + path + " for writing");
    const size_t bytes = pt_linear_bytes(width, height, format);
    bool ok = std::fwrite(header, 1, static_cast<size_t>(len), f) == static_cast<size_t>(len);
    ok = ok && std::fwrite(body, 1, bytes, f) == bytes;
    ok = (std::fclose(f) == 0) && ok;
    return ok ? static_cast<int>(PT_OK) : fail(PT_ERR_IO, std::string("short write to ") + path);
}

}  // namespace

extern "C" {

size_t pt_linear_bytes(int32_t width, int32_t height, int32_t format) {
    if (!valid_size(width, height) || (format != PT_LINEAR_PFM && format != PT_LINEAR_RGBE)) return 0;
    return (format == PT_LINEAR_PFM ? 12u : 4u) * static_cast<size_t>(width) * static_cast<size_t>(height);
}

int pt_linear_encode(int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure, const pt_linear_params *lin,
                     uint8_t *out) {
    return guarded([&] { return linear_encode_impl(width, height, mean_rgb, count, exposure, lin, out); });
}

int pt_write_pfm(const char *path, int32_t width, int32_t height, const uint8_t *body) {
    return guarded([&] { return write_picture(path, width, height, body, PT_LINEAR_PFM); });
}

int pt_write_hdr(const char *path, int32_t width, int32_t height, const uint8_t *body) {
    return guarded([&] { return write_picture(path, width, height, body, PT_LINEAR_RGBE); });
}

}  // extern "C"
