// Direct lighting (include/pt_hip.h: direct lighting), the one copy of its arithmetic: the light table's record, the choice of a light
// by the table's distribution over the areas, the point on it, and the term a diffuse hit adds for that point before visibility.  The
// direct kernels (pt_kernels.hip: integrate_kernel_direct) run it per scattering diffuse hit and pt_direct_term on the host.  All
// float, every operation rounded once in the order written, nothing fused; roots and quotients are the correctly rounded ones (the
// build's flags on the device).  `normalize` is the caller's normalize3: v * (1 / sqrt((x x + y y) + z z)).
#pragma once
#include <cstdint>

#include "pt_grade.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pt {

// The fourth Philox counter word of the direct term's words (l0 .. l3).  Every other call of the integrator has 0 there; the display's
// dither and grain, which run under the same key, have 1 and 2 (pt_grain.hpp).
constexpr uint32_t kDirectStream = 3u;

// One light of the table (RenderArgs::lights; pt_hip.h: pt_light has the same layout): 80 bytes, five 16-byte loads.  Lights are the
// triangles of non-zero area whose material is the single emissive lobe, in the original triangle order.
struct alignas(16) LightRec {
    float v0[3];
    float cdf;       // float(cumulative area up to and including this light / total area); the last light's is 1.0f
    float e1[3];     // v1 - v0, float differences
    int32_t orig;    // the triangle's index in the original order: what the closest-hit search reports for it
    float e2[3];     // v2 - v0
    float pad0;
    float nl[3];     // the stored plane normal
    float pad1;
    float le[3];     // the material's Kd: what the emissive lobe multiplies the throughput by
    float pad2;
};
static_assert(sizeof(LightRec) == 80, "five 16-byte loads");

// The first light i with u < cdf_i (u in (0, 1), the last cdf is 1: there is one), by bisection.
PT_GRADE_FN int32_t direct_pick(const LightRec *lights, int32_t n, float u) {
    int32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (u < lights[mid].cdf) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// The term of light `l` for a diffuse hit whose next origin is O = p + N eps, with stored normal N, shading normal n (Ns, or N),
// throughput T (after the texel step) and albedo Kd; u1, u2 = unit_float(l1), unit_float(l2); area = the table's total area A.
// Returns whether there is a term (r2 > 0 and all three cosines > 0); w = the unit direction of the shadow ray, P = the sampled point.
template <class Normalize>
PT_GRADE_FN bool direct_term(const LightRec &l, float area, float u1, float u2, float ox, float oy, float oz, float Nx, float Ny, float Nz,
                             float nx, float ny, float nz, float tr, float tg, float tb, float kdr, float kdg, float kdb, Normalize normalize,
                             float &px, float &py, float &pz, float &wx, float &wy, float &wz, float &cr, float &cg, float &cb) {
    if (u1 + u2 > 1.0f) { u1 = 1.0f - u1; u2 = 1.0f - u2; }   // (exact: multiples of 2^-24)
    px = (l.v0[0] + l.e1[0] * u1) + l.e2[0] * u2;
    py = (l.v0[1] + l.e1[1] * u1) + l.e2[1] * u2;
    pz = (l.v0[2] + l.e1[2] * u1) + l.e2[2] * u2;
    wx = px - ox; wy = py - oy; wz = pz - oz;
    const float r2 = (wx * wx + wy * wy) + wz * wz;
    normalize(wx, wy, wz);
    const float cn = (Nx * wx + Ny * wy) + Nz * wz;
    const float cs = (nx * wx + ny * wy) + nz * wz;
    const float cl = -((l.nl[0] * wx + l.nl[1] * wy) + l.nl[2] * wz);
    cr = cg = cb = 0.0f;
    if (!(r2 > 0.0f && cn > 0.0f && cs > 0.0f && cl > 0.0f)) return false;
    const float g = (((cs * __builtin_fabsf(wz)) * cl) * area) / (3.141593f * r2);
    cr = ((tr * kdr) * l.le[0]) * g;
    cg = ((tg * kdg) * l.le[1]) * g;
    cb = ((tb * kdb) * l.le[2]) * g;
    return true;
}

}  // namespace pt
