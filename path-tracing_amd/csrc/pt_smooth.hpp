// Smooth shading (include/pt_hip.h: shading normals), the one copy of its arithmetic: the interpolated normal of a hit point, its
// fallback to the stored plane normal, the flip onto the plane's side, and the test that sends a step back to the stored normal.
// The smooth kernels (pt_kernels.hip: integrate_kernel_smooth) run it per hit, the first-hit feature pass (pt_smooth_features.hip)
// per pixel and pt_shading_normal_at on the host.  All float, every operation rounded once, nothing fused.  `normalize` is the
// caller's normalize3: v * (1 / sqrt((x x + y y) + z z)) with a correctly rounded root and reciprocal.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pt_grade.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pt {

// One corner's normal on the device: 16 bytes, one load.  Three per triangle (RenderArgs::smooth_normals), in the ORIGINAL triangle
// order, corners in the order of the vertices.
struct alignas(16) SmoothCorner { float x, y, z, pad; };

// Ns of a hit with barycentrics b1, b2 (pt_texture.hpp: tex_barycentrics_record) on a triangle with corner normals n0, n1, n2 and
// stored plane normal N:  m = (b0 n0 + b1 n1) + b2 n2 per component,  l = (m.x^2 + m.y^2) + m.z^2;  l not finite or not > 0: N;
// else normalize(m);  then onto N's side.  Returns whether Ns is the interpolated one (false: it is N itself).
template <class Normalize>
PT_GRADE_FN bool smooth_normal(float n0x, float n0y, float n0z, float n1x, float n1y, float n1z, float n2x, float n2y, float n2z,
                               float b1, float b2, float Nx, float Ny, float Nz, Normalize normalize, float &sx, float &sy, float &sz) {
    const float b0 = (1.0f - b1) - b2;
    float mx = (b0 * n0x + b1 * n1x) + b2 * n2x;
    float my = (b0 * n0y + b1 * n1y) + b2 * n2y;
    float mz = (b0 * n0z + b1 * n1z) + b2 * n2z;
    const float l = (mx * mx + my * my) + mz * mz;
    const bool usable = l > 0.0f && l < __builtin_inff();   // (a NaN fails both)
    if (usable) {
        normalize(mx, my, mz);
    } else {
        mx = Nx; my = Ny; mz = Nz;
    }
    if ((mx * Nx + my * Ny) + mz * Nz < 0.0f) { mx = -mx; my = -my; mz = -mz; }
    sx = mx; sy = my; sz = mz;
    return usable;
}

// The fallback rule: a step made with Ns whose new unit direction r leaves on the other side of the stored plane from the origin's
// offset oe (+-eps) is made again with N.  True = keep the step.
PT_GRADE_FN bool smooth_keeps(float rx, float ry, float rz, float Nx, float Ny, float Nz, float oe) {
    return ((rx * Nx + ry * Ny) + rz * Nz) * oe > 0.0f;
}

}  // namespace pt
