// Scene-linear output (include/pt_hip.h: pt_linear_*), the one copy of its arithmetic and the launch interface of its kernel
// (pt_linear.hip): the host's definition of the bytes (pt_linear_encode) and the kernel call these functions.  Every step is integer
// arithmetic, a comparison or one correctly rounded float multiply, so host and device agree bit for bit; nothing is fused.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "pt_grade.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pt {

constexpr int kLinearPfm = 1, kLinearRgbe = 2;      // pt_hip.h: PT_LINEAR_PFM, PT_LINEAR_RGBE
constexpr uint32_t kLinearMaxBits = 0x7E800000u;    // 2^126: the largest value a channel is encoded as
constexpr uint32_t kLinearMinExponent = 27u;        // the exponent field of 2^-100: a pixel whose largest channel lies below is zero

// What is encoded of one channel: m, or m * e -- one multiply.
PT_GRADE_FN float linear_value(float m, bool exposed, float e) { return exposed ? m * e : m; }

// c' of pt_hip.h: NaN, -0 and negatives give 0, everything above 2^126 gives 2^126.
PT_GRADE_FN float linear_clip(float c) {
    const float top = grade_from_bits(kLinearMaxBits);
    return c > 0.0f ? (c < top ? c : top) : 0.0f;
}

// The four bytes R, G, B, E of one pixel with samples, as the little-endian dword R | G << 8 | B << 16 | E << 24.
PT_GRADE_FN uint32_t linear_rgbe(float r, float g, float b) {
    r = linear_clip(r); g = linear_clip(g); b = linear_clip(b);
    float v = r > g ? r : g;
    v = v > b ? v : b;
    const uint32_t be = (grade_bits(v) >> 23) & 255u;
    if (be < kLinearMinExponent) return 0u;
    const float scale = grade_from_bits((261u - be) << 23);   // 2^(8 - e), e = be - 126: the largest channel becomes 128 .. 255
    const uint32_t br = static_cast<uint32_t>(static_cast<int>(r * scale)), bg = static_cast<uint32_t>(static_cast<int>(g * scale)),
                   bb = static_cast<uint32_t>(static_cast<int>(b * scale));
    return br | (bg << 8) | (bb << 16) | ((be + 2u) << 24);
}

struct LinearArgs {
    int width, height;
    int divide;                  // 0: rgb holds the means; 1: rgb holds sums, the mean is rgb / float(count)
    int format;                  // kLinearPfm or kLinearRgbe
    int exposed;                 // 1: every channel is multiplied by *exposure first
    const float *rgb;            // 3 floats per pixel, 16-byte aligned
    const int32_t *count;        // 16-byte aligned
    const float *exposure;       // a device scalar written earlier on the stream; read only if exposed
    uint32_t *out;               // 16-byte aligned, written as whole 16-byte groups: room for pt::linear_room(width * height, format) bytes
};
// Bytes the kernel may write for n pixels: the body, rounded up to whole 16-byte groups.
inline size_t linear_room(size_t n, int format) { return ((format == kLinearPfm ? 12 : 4) * n + 15) / 16 * 16; }
// One kernel: every pixel's bytes, none left to the host.
hipError_t launch_linear_encode(const LinearArgs &args, hipStream_t stream);

}  // namespace pt
