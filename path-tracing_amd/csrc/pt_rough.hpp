// Rough specular reflection (include/pt_hip.h: rough specular), the one copy of its arithmetic: the glossy lobe of a material with a
// roughness alpha -- the normal turned to the ray's side, the tangent frame of Duff et al. 2017, a microfacet normal drawn from the GGX
// distribution of visible normals (Heitz 2018), the reflection about it and the Smith term G1 of the new direction.  The rough kernels
// (pt_kernels.hip: integrate_kernel_rough) run it per glossy hit and pt_rough_step on the host.  All float, every operation rounded
// once in the order written, nothing fused; roots and quotients are the correctly rounded ones (the build's flags on the device).
// `sincos` is the caller's portable sincos (double +, -, * only), `normalize` its normalize3: v * (1 / sqrt((x x + y y) + z z)).
#pragma once
#include <cstdint>

#include "pt_grade.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pt {

constexpr float kRoughAxisFloor = 9.094947017729282e-13f;               // 2^-40: below it the stretched view direction counts as the normal itself

// The step for a ray of unit direction d that has hit a surface with unit normal n (the stored N, or Ns under shading normals) and
// roughness alpha in [2^-10, 1], with the segment's uniforms u1 = unit_float(w1), u2 = unit_float(w2): l = the new unit direction,
// g1 = the factor on Ks (0 where l leaves on the far side of n), and h = the microfacet normal in the frame (t1, t2, n).
template <class SinCos, class Normalize>
PT_GRADE_FN void rough_step(float nx, float ny, float nz, float dx, float dy, float dz, float alpha, float u1, float u2, SinCos sincos,
                            Normalize normalize, float &lx, float &ly, float &lz, float &g1, float &hx, float &hy, float &hz) {
    // n onto the side the ray came from (exact)
    const float c = (nx * dx + ny * dy) + nz * dz;
    if (c > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    // the frame (t1, t2, n): Duff et al. 2017
    const float s = __builtin_copysignf(1.0f, nz);
    const float a = -1.0f / (s + nz);
    const float b = (nx * ny) * a;
    const float t1x = 1.0f + ((s * nx) * nx) * a, t1y = s * b, t1z = -(s * nx);
    const float t2x = b, t2y = s + (ny * ny) * a, t2z = -ny;
    // v = -d in that frame
    const float vx = -((t1x * dx + t1y * dy) + t1z * dz);
    const float vy = -((t2x * dx + t2y * dy) + t2z * dz);
    const float vz = __builtin_fabsf(c);
    // stretched
    float ex = alpha * vx, ey = alpha * vy, ez = vz;
    normalize(ex, ey, ez);
    // the frame (T1, T2, e) about it; T1.z = 0
    const float q = ex * ex + ey * ey;
    float T1x = 1.0f, T1y = 0.0f;
    if (q >= kRoughAxisFloor) {
        const float iq = 1.0f / __builtin_sqrtf(q);
        T1x = -(ey * iq); T1y = ex * iq;
    }
    const float T2x = -(ez * T1y), T2y = ez * T1x, T2z = ex * T1y - ey * T1x;
    // a point of the unit disk, its second coordinate warped onto the visible half
    const float r = __builtin_sqrtf(u1);
    float sn, cs;
    sincos((2 * 3.141593f) * u2, sn, cs);
    const float p1 = r * cs;
    float p2 = r * sn;
    const float w = 0.5f * (1.0f + ez);
    const float k1 = 1.0f - p1 * p1;
    p2 = (1.0f - w) * __builtin_sqrtf(k1 > 0.0f ? k1 : 0.0f) + w * p2;
    // projected onto the hemisphere
    const float k2 = (1.0f - p1 * p1) - p2 * p2;
    const float p3 = __builtin_sqrtf(k2 > 0.0f ? k2 : 0.0f);
    const float mx = (p1 * T1x + p2 * T2x) + p3 * ex;
    const float my = (p1 * T1y + p2 * T2y) + p3 * ey;
    const float mz = p2 * T2z + p3 * ez;
    // unstretched: the microfacet normal in (t1, t2, n)
    hx = alpha * mx; hy = alpha * my; hz = mz > 0.0f ? mz : 0.0f;
    normalize(hx, hy, hz);
    // in the scene's frame, and the reflection about it (the mirror's form)
    const float Hx = (hx * t1x + hy * t2x) + hz * nx;
    const float Hy = (hx * t1y + hy * t2y) + hz * ny;
    const float Hz = (hx * t1z + hy * t2z) + hz * nz;
    const float dh = (Hx * dx + Hy * dy) + Hz * dz;
    lx = dx - Hx * dh * 2.0f; ly = dy - Hy * dh * 2.0f; lz = dz - Hz * dh * 2.0f;
    normalize(lx, ly, lz);
    // the separable Smith term of the new direction
    const float nl = (nx * lx + ny * ly) + nz * lz;
    g1 = 0.0f;
    if (nl > 0.0f) {
        const float a2 = alpha * alpha;
        const float g = (2.0f * nl) / (nl + __builtin_sqrtf(a2 + (1.0f - a2) * (nl * nl)));
        g1 = g < 1.0f ? g : 1.0f;
    }
}

}  // namespace pt
