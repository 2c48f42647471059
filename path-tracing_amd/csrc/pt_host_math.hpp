// The kernels' arithmetic restated for the host's own evaluations (pt_shading_normal_at, pt_rough_step, pt_direct_term): one spelling
// of each, float and double + - * / sqrt only, so that -ffp-contract=off makes them the kernels' results bit for bit.
#pragma once
#include <cmath>
#include <cstdint>

namespace ptc {

// A random word as the kernels' float in (0, 1): its top 23 bits and a half.
inline float host_unit_float(uint32_t w) { return static_cast<float>(((w >> 9) << 1) | 1u) * 5.9604644775390625e-08f; }

// The kernels' normalize3.
inline void host_normalize3(float &x, float &y, float &z) {
    const float inv = 1.0f / std::sqrt((x * x + y * y) + z * z);
    x = x * inv; y = y * inv; z = z * inv;
}

// The kernels' portable_sincos: double +, -, * only, the same constants in the same order.
inline void host_sincos(float a, float &s_out, float &c_out) {
    static const double t[16] = {
        0.63661977236758138, 1.57079632673412561417e+00, 6.07710050650619224932e-11, 0.5,
        -1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04, 2.75573137070700676789e-06,
        -2.50507602534068634195e-08, 1.58969099521155010221e-10,
        4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05, -2.75573143513906633035e-07,
        2.08757232129817482790e-09, -1.13596475577881948265e-11};
    const double x = static_cast<double>(a);
    const int k = static_cast<int>(x * t[0] + t[3]);
    const double kd = static_cast<double>(k);
    const double r = (x - kd * t[1]) - kd * t[2];
    const double z = r * r;
    const double ps = t[4] + z * (t[5] + z * (t[6] + z * (t[7] + z * (t[8] + z * t[9]))));
    const double sn = r + r * (z * ps);
    const double pc = t[10] + z * (t[11] + z * (t[12] + z * (t[13] + z * (t[14] + z * t[15]))));
    const double cs = (1.0 - t[3] * z) + (z * z) * pc;
    const float sf = static_cast<float>(sn), cf = static_cast<float>(cs);
    switch (static_cast<unsigned>(k) & 3u) {
        case 0: s_out = sf; c_out = cf; break;
        case 1: s_out = cf; c_out = -sf; break;
        case 2: s_out = -sf; c_out = -cf; break;
        default: s_out = -cf; c_out = sf; break;
    }
}

}  // namespace ptc
