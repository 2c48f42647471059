// Colour grading (include/pt_hip.h: pt_colour_*, pt_lut_*), the one copy of its per-pixel arithmetic: the host stage
// (pt_colour_host), the kernel (pt_display_colour.hip) and the host's finishing of deferred pixels all call these functions.  Every
// step is one correctly rounded float operation in the order written (* + -, comparisons) or integer arithmetic, so host and
// device agree bit for bit; nothing is fused.
#pragma once
#include <cstdint>

#include "pt_grade.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pt {

// pt_hip.h: PT_LUT_MAX_SIZE
constexpr int kLutMinSize = 2, kLutMaxSize = 65;

// One vertex of a 3D LUT as host and device hold it: 16 bytes, so that a vertex is one load.
struct alignas(16) LutVertex {
    float r, g, b, pad;
};

// What the per-pixel step needs of a pt_colour_params, by value (the kernel's argument and the host's setup).
struct ColourStep {
    float m[9];             // M = U S W, row-major
    int apply_matrix;       // 0: M is the identity bit for bit and its three lines are skipped
    int lut_n;              // N, or 0: no LUT
    const LutVertex *lut;   // N^3 vertices, red index fastest (host memory on the host, device memory in the kernel)
};

// m' = M m, three lines.
PT_GRADE_FN void colour_matrix_apply(const float *M, float &r, float &g, float &b) {
    const float nr = ((M[0] * r) + (M[1] * g)) + (M[2] * b);
    const float ng = ((M[3] * r) + (M[4] * g)) + (M[5] * b);
    const float nb = ((M[6] * r) + (M[7] * g)) + (M[8] * b);
    r = nr; g = ng; b = nb;
}

// Cell index and fraction of one channel: always 0 <= i <= n - 2, whatever g is.
PT_GRADE_FN void colour_lut_axis(float g, int n, int &i, float &f) {
    const float x = !(g >= 0.0f) ? 0.0f : (g > 1.0f ? 1.0f : g);
    const float s = x * static_cast<float>(n - 1);
    i = static_cast<int>(s);
    if (i > n - 2) i = n - 2;
    f = s - static_cast<float>(i);
}

// The LUT with tetrahedral interpolation, on (r, g, b) in place.
PT_GRADE_FN void colour_lut_apply(const LutVertex *lut, int n, float &r, float &g, float &b) {
    int ir, ig, ib;
    float fr, fg, fb;
    colour_lut_axis(r, n, ir, fr);
    colour_lut_axis(g, n, ig, fg);
    colour_lut_axis(b, n, ib, fb);
    const int sr = 1, sg = n, sb = n * n;
    // the path's axes in the order of their fractions, f1 >= f2 >= f3 (pt_hip.h states the table; ties have one answer)
    int s1, s2;
    float f1, f2, f3;
    if (fr >= fg) {
        if (fg >= fb) { s1 = sr; s2 = sg; f1 = fr; f2 = fg; f3 = fb; }
        else if (fr >= fb) { s1 = sr; s2 = sb; f1 = fr; f2 = fb; f3 = fg; }
        else { s1 = sb; s2 = sr; f1 = fb; f2 = fr; f3 = fg; }
    } else {
        if (fr >= fb) { s1 = sg; s2 = sr; f1 = fg; f2 = fr; f3 = fb; }
        else if (fg >= fb) { s1 = sg; s2 = sb; f1 = fg; f2 = fb; f3 = fr; }
        else { s1 = sb; s2 = sg; f1 = fb; f2 = fg; f3 = fr; }
    }
    const int at = (ib * n + ig) * n + ir;
    const LutVertex A = lut[at], B = lut[at + s1], C = lut[at + s1 + s2], D = lut[at + sr + sg + sb];
    r = ((A.r + (f1 * (B.r - A.r))) + (f2 * (C.r - B.r))) + (f3 * (D.r - C.r));
    g = ((A.g + (f1 * (B.g - A.g))) + (f2 * (C.g - B.g))) + (f3 * (D.g - C.g));
    b = ((A.b + (f1 * (B.b - A.b))) + (f2 * (C.b - B.b))) + (f3 * (D.b - C.b));
}

// One pixel with samples: matrix -> exposure -> curve -> LUT.  In: the mean; out: what takes g's place.
template <int CURVE>
PT_GRADE_FN void colour_pixel(const ColourStep &c, float e, float &r, float &g, float &b) {
    if (c.apply_matrix) colour_matrix_apply(c.m, r, g, b);
    r = grade_value<CURVE>(r, e);
    g = grade_value<CURVE>(g, e);
    b = grade_value<CURVE>(b, e);
    if (c.lut_n) colour_lut_apply(c.lut, c.lut_n, r, g, b);
}
PT_GRADE_FN void colour_pixel(const ColourStep &c, int curve, float e, float &r, float &g, float &b) {
    switch (curve) {
        case kCurveClamp: colour_pixel<kCurveClamp>(c, e, r, g, b); break;
        case kCurveReinhard: colour_pixel<kCurveReinhard>(c, e, r, g, b); break;
        case kCurveAces: colour_pixel<kCurveAces>(c, e, r, g, b); break;
        default: colour_pixel<kCurveReference>(c, e, r, g, b); break;
    }
}

}  // namespace pt
