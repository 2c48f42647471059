// Film grain and dithered quantization (include/pt_hip.h: pt_grain_*), the one copy of their arithmetic: the host chain's last step
// (pt_grain_quantize), the kernel (pt_display_grain.hip) and the host's finishing of deferred pixels all call these functions.  Every
// step is one correctly rounded float operation in the order written (* / + -, comparisons, floor, int <-> float conversions) or
// integer arithmetic, so host and device agree bit for bit; nothing is fused.  The random words are Philox4x32-10 under the
// integrator's key with fourth counter words of their own (1 and 2; the integrator's segments use 0, its direct-lighting words 3, pt_direct.hpp:
// kDirectStream, environment sampling's 4, pt_envdirect.hpp: kEnvDirectStream, and the roulette's word 5, pt_roulette.hpp:
// kRouletteStream -- a new stream takes the next free word); the generator is spelled here once more because the host
// needs it too.
#pragma once
#include <cstdint>

#include "pt_grade.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pt {

// pt_hip.h: the largest lattice pitch
constexpr float kGrainMaxSize = 8.0f;
constexpr uint32_t kGrainKey1 = 0x50544831u;   // "PTH1", the integrator's second key word (pt_kernels.hpp: kPhiloxKey1)
constexpr uint32_t kGrainDitherStream = 1u, kGrainLatticeStream = 2u;   // the counter's fourth word; the integrator's are 0, 3 (pt_direct.hpp), 4 (pt_envdirect.hpp) and 5 (pt_roulette.hpp)

// What the per-pixel steps need of a pt_grain_params, by value (the kernel's argument and the host's setup), and the image's width:
// a pixel of the flat plane is (p % width, p / width).
struct GrainStep {
    float strength;   // 0: no lattice word is drawn, g' = g
    float size;       // the lattice pitch with the default filled in: 1 .. 8
    float dither;     // 0: no dither word is drawn, every channel is quantized as without the stage
    uint32_t seed, frame;
    int32_t width;
};

// Philox4x32-10 of counter (c0, c1, c2, c3) under key (k0, k1): Random123's rounds, multipliers and key schedule.
PT_GRADE_FN void grain_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t &o0, uint32_t &o1,
                              uint32_t &o2, uint32_t &o3) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = static_cast<uint64_t>(c0) * 0xD2511F53u;
        const uint64_t p1 = static_cast<uint64_t>(c2) * 0xCD9E8D57u;
        const uint32_t h0 = static_cast<uint32_t>(p0 >> 32), l0 = static_cast<uint32_t>(p0);
        const uint32_t h1 = static_cast<uint32_t>(p1 >> 32), l1 = static_cast<uint32_t>(p1);
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o0 = c0; o1 = c1; o2 = c2; o3 = c3;
}

// A word as a triangular variate in (-1, 1): the sum of its halves about its mean.  The integer is exact in a float, the product too.
PT_GRADE_FN float grain_tri(uint32_t w) {
    const int s = (static_cast<int>(w & 0xFFFFu) + static_cast<int>(w >> 16)) - 65535;
    return static_cast<float>(s) * 1.52587890625e-05f;   // 2^-16
}

// The three dither words of pixel (x, y): words 0, 1, 2 of counter (x, y, frame, 1), for r, g, b.
PT_GRADE_FN void grain_dither_words(const GrainStep &s, uint32_t x, uint32_t y, uint32_t &wr, uint32_t &wg, uint32_t &wb) {
    uint32_t unused;
    grain_philox(x, y, s.frame, kGrainDitherStream, s.seed, kGrainKey1, wr, wg, wb, unused);
}

// The value of lattice point (ix, iy): word 0 of counter (ix, iy, frame, 2).
PT_GRADE_FN float grain_lattice(const GrainStep &s, uint32_t ix, uint32_t iy) {
    uint32_t w0, w1, w2, w3;
    grain_philox(ix, iy, s.frame, kGrainLatticeStream, s.seed, kGrainKey1, w0, w1, w2, w3);
    return grain_tri(w0);
}

// The noise of pixel (x, y): bilinear over the four lattice values round (x / size, y / size), in difference form.  SIZED = false is
// size == 1, where tx = ty = 0 and the three other values are multiplied by 0: n = v00 to the bit, and they are not drawn.
template <bool SIZED>
PT_GRADE_FN float grain_noise(const GrainStep &s, uint32_t x, uint32_t y) {
    if (!SIZED) return grain_lattice(s, x, y);
    const float fx = static_cast<float>(x) / s.size, fy = static_cast<float>(y) / s.size;
    const uint32_t ix = static_cast<uint32_t>(fx), iy = static_cast<uint32_t>(fy);   // (not negative: this is the floor)
    const float tx = fx - static_cast<float>(ix), ty = fy - static_cast<float>(iy);
    const float v00 = grain_lattice(s, ix, iy), v10 = grain_lattice(s, ix + 1u, iy);
    const float v01 = grain_lattice(s, ix, iy + 1u), v11 = grain_lattice(s, ix + 1u, iy + 1u);
    const float a = v00 + (tx * (v10 - v00));
    const float b = v01 + (tx * (v11 - v01));
    return a + (ty * (b - a));
}

// One channel under grain: sn = strength * n of its pixel.  A channel outside (0, 1) -- NaN included -- keeps its bits.
PT_GRADE_FN float grain_apply(float g, float sn) {
    if (!(0.0f < g && g < 1.0f)) return g;
    const float w = (g * (1.0f - g)) * 4.0f;
    const float v = g + (sn * w);
    return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
}

// The three channels of pixel (x, y) under grain, in place.
template <bool SIZED>
PT_GRADE_FN void grain_pixel(const GrainStep &s, uint32_t x, uint32_t y, float &r, float &g, float &b) {
    if (s.strength == 0.0f) return;
    const float sn = s.strength * grain_noise<SIZED>(s, x, y);
    r = grain_apply(r, sn);
    g = grain_apply(g, sn);
    b = grain_apply(b, sn);
}
PT_GRADE_FN void grain_pixel(const GrainStep &s, uint32_t x, uint32_t y, float &r, float &g, float &b) {
    if (s.size == 1.0f) grain_pixel<false>(s, x, y, r, g, b);
    else grain_pixel<true>(s, x, y, r, g, b);
}

// The level of a channel the table covers, dithered: k = its level (the number of thresholds <= g), lo = the threshold it reached (0
// for k == 0), hi = the next one.  lo <= g < hi, so 0 <= f <= 1 and f + dither * tri lies in (-1, 2): j is -1, 0 or 1.  A level that
// would be negative or leave k's block of 256 stays k: black cannot go below 0, and byte 255 cannot wrap to 0.
PT_GRADE_FN uint32_t grain_dither_level(uint32_t k, float lo, float hi, float g, float dither, uint32_t word) {
    const float f = (g - lo) / (hi - lo);
    const float t = f + (dither * grain_tri(word));
    const int j = static_cast<int>(__builtin_floorf(t));
    const int k2 = static_cast<int>(k) + j;
    return (k2 < 0 || (k2 >> 8) != (static_cast<int>(k) >> 8)) ? k : static_cast<uint32_t>(k2);
}

}  // namespace pt
