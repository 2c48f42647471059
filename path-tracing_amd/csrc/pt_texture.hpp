// Albedo textures (include/pt_hip.h: pt_texture), the one copy of their arithmetic: the barycentrics of a hit point, the texture
// coordinates they give, the wrap and the two filters.  The texture kernels (pt_kernels.hip: integrate_kernel_texture) run it per
// textured hit, the first-hit feature pass (pt_denoise.hip) per textured pixel and pt_texture_lookup on the host.  All float, every
// operation rounded once, nothing fused; the divisions are IEEE divisions.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pt_grade.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pt {

constexpr int kTexMaxSide = 8192;                 // the largest width or height of one texture
constexpr uint64_t kTexMaxTexels = 1ull << 28;    // the most texels one list holds (16 bytes each on the device)
constexpr int kTexNearest = 0, kTexBilinear = 1;  // PT_TEXTURE_NEAREST, PT_TEXTURE_BILINEAR

struct alignas(16) TexTexel { float r, g, b, pad; };   // 16 bytes: one load
// One material's entry of the texture table (RenderArgs::tex_recs): w == 0 = not textured.  Its w x h texels start at texel `first`
// of the list's pool, rows top-down (row 0 is the top of the picture, v = 1).
struct alignas(16) TexRec {
    uint32_t first;
    int32_t w, h, filter;
};

// b1, b2 of point p in the plane of triangle (v0, v1, v2): p ~ v0 + b1 (v1 - v0) + b2 (v2 - v0).  den == 0 (a collinear triangle) gives 0, 0.
PT_GRADE_FN void tex_barycentrics(float v0x, float v0y, float v0z, float v1x, float v1y, float v1z, float v2x, float v2y, float v2z,
                                  float px, float py, float pz, float &b1, float &b2) {
    const float e1x = v1x - v0x, e1y = v1y - v0y, e1z = v1z - v0z;
    const float e2x = v2x - v0x, e2y = v2y - v0y, e2z = v2z - v0z;
    const float wx = px - v0x, wy = py - v0y, wz = pz - v0z;
    const float d11 = (e1x * e1x + e1y * e1y) + e1z * e1z;
    const float d12 = (e1x * e2x + e1y * e2y) + e1z * e2z;
    const float d22 = (e2x * e2x + e2y * e2y) + e2z * e2z;
    const float w1 = (wx * e1x + wy * e1y) + wz * e1z;
    const float w2 = (wx * e2x + wy * e2y) + wz * e2z;
    const float den = d11 * d22 - d12 * d12;
    b1 = 0.0f;
    b2 = 0.0f;
    if (den != 0.0f) {   // (a NaN den goes through the divisions and leaves NaN coordinates, which tex_wrap sends to 0)
        b1 = (d22 * w1 - d12 * w2) / den;
        b2 = (d11 * w2 - d12 * w1) / den;
    }
}

// The per-triangle record of the barycentrics (RenderArgs::tex_bary, pt_hip.h states it): b1 = a1 . p + c1, b2 = a2 . p + c2.
// 32 bytes: two 16-byte loads.  Built on the host by tex_bary_record in plain float, nothing fused.
struct alignas(16) TexBary {
    float a1[3], c1;
    float a2[3], c2;
};
inline TexBary tex_bary_record(const float *v0, const float *v1, const float *v2) {
    const float e1x = v1[0] - v0[0], e1y = v1[1] - v0[1], e1z = v1[2] - v0[2];
    const float e2x = v2[0] - v0[0], e2y = v2[1] - v0[1], e2z = v2[2] - v0[2];
    const float d11 = (e1x * e1x + e1y * e1y) + e1z * e1z;
    const float d12 = (e1x * e2x + e1y * e2y) + e1z * e2z;
    const float d22 = (e2x * e2x + e2y * e2y) + e2z * e2z;
    const float den = d11 * d22 - d12 * d12;
    TexBary r = {{0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 0.0f}, 0.0f};
    if (den != 0.0f) {   // (den == 0, a collinear triangle: the zero record, b1 = b2 = 0)
        r.a1[0] = (e1x * d22 - e2x * d12) / den; r.a1[1] = (e1y * d22 - e2y * d12) / den; r.a1[2] = (e1z * d22 - e2z * d12) / den;
        r.a2[0] = (e2x * d11 - e1x * d12) / den; r.a2[1] = (e2y * d11 - e1y * d12) / den; r.a2[2] = (e2z * d11 - e1z * d12) / den;
        r.c1 = -((r.a1[0] * v0[0] + r.a1[1] * v0[1]) + r.a1[2] * v0[2]);
        r.c2 = -((r.a2[0] * v0[0] + r.a2[1] * v0[1]) + r.a2[2] * v0[2]);
    }
    return r;
}
// b1, b2 of point p from the record: ((a.x * p.x + a.y * p.y) + a.z * p.z) + c
PT_GRADE_FN void tex_barycentrics_record(float a1x, float a1y, float a1z, float c1, float a2x, float a2y, float a2z, float c2,
                                         float px, float py, float pz, float &b1, float &b2) {
    b1 = ((a1x * px + a1y * py) + a1z * pz) + c1;
    b2 = ((a2x * px + a2y * py) + a2z * pz) + c2;
}

// (u, v) at barycentrics b1, b2 from the triangle's three corners' coordinates uv = u0, v0, u1, v1, u2, v2.
PT_GRADE_FN void tex_interpolate(const float uv0, const float vv0, const float uv1, const float vv1, const float uv2, const float vv2,
                                 float b1, float b2, float &u, float &v) {
    const float b0 = (1.0f - b1) - b2;
    u = (b0 * uv0 + b1 * uv1) + b2 * uv2;
    v = (b0 * vv0 + b1 * vv1) + b2 * vv2;
}

// Repeat wrap: the fraction u - floor(u) where that lies in [0, 1), else 0 (NaN, +-inf, and the few negative u whose fraction rounds to 1).
PT_GRADE_FN float tex_wrap(float u) {
    const float f = u - __builtin_floorf(u);
    return (f >= 0.0f && f < 1.0f) ? f : 0.0f;
}

// The (up to) four texels of a lookup, as indices into the texture's w x h texels (rows top-down), and the two weights.
struct TexTaps {
    int32_t i00, i10, i01, i11;   // (x0, y0), (x1, y0), (x0, y1), (x1, y1), y counted upwards; nearest: all four the same texel
    float tx, ty;
};

// along one axis of n texels, fraction f in [0, 1): nearest = the texel f falls into; bilinear = the two texels whose centres
// (i + 0.5) / n enclose f, the one below wrapping to n - 1 and the one above to 0, and the weight of the upper one
PT_GRADE_FN void tex_axis(float f, int n, int filter, int &i0, int &i1, float &t) {
    const float x = f * static_cast<float>(n);   // in [0, n]
    if (filter == kTexNearest) {
        const int i = static_cast<int>(x);
        i0 = i1 = i < n - 1 ? i : n - 1;
        t = 0.0f;
    } else {
        const float c = x - 0.5f;                // in [-0.5, n - 0.5]
        const float fl = __builtin_floorf(c);    // -1 .. n - 1
        t = c - fl;
        const int i = static_cast<int>(fl);
        i0 = i < 0 ? n - 1 : i;
        i1 = i + 1 > n - 1 ? 0 : i + 1;
    }
}

PT_GRADE_FN TexTaps tex_taps(int w, int h, int filter, float u, float v) {
    int x0, x1, y0, y1;
    TexTaps k;
    tex_axis(tex_wrap(u), w, filter, x0, x1, k.tx);
    tex_axis(tex_wrap(v), h, filter, y0, y1, k.ty);
    const int32_t r0 = (h - 1 - y0) * w, r1 = (h - 1 - y1) * w;   // v points up, the rows run down
    k.i00 = r0 + x0; k.i10 = r0 + x1;
    k.i01 = r1 + x0; k.i11 = r1 + x1;
    return k;
}

PT_GRADE_FN float tex_lerp(float a, float b, float t) { return a + (b - a) * t; }

// The texel the texture holds at (u, v).  `texels`: anything indexable that yields a TexTexel.
template <class Texels>
PT_GRADE_FN void tex_lookup(const Texels texels, int w, int h, int filter, float u, float v, float &r, float &g, float &b) {
    const TexTaps k = tex_taps(w, h, filter, u, v);
    const TexTexel t00 = texels[k.i00];
    if (filter == kTexNearest) {
        r = t00.r; g = t00.g; b = t00.b;
        return;
    }
    const TexTexel t10 = texels[k.i10], t01 = texels[k.i01], t11 = texels[k.i11];
    r = tex_lerp(tex_lerp(t00.r, t10.r, k.tx), tex_lerp(t01.r, t11.r, k.tx), k.ty);
    g = tex_lerp(tex_lerp(t00.g, t10.g, k.tx), tex_lerp(t01.g, t11.g, k.tx), k.ty);
    b = tex_lerp(tex_lerp(t00.b, t10.b, k.tx), tex_lerp(t01.b, t11.b, k.tx), k.ty);
}

// The texel of a hit: point p on triangle `tri` (its vertices v0, v1, v2 and, per corner, coordinates uv[0 .. 5]) of a material whose
// entry is `m` (m.w != 0).
template <class Texels>
PT_GRADE_FN void tex_at_hit(const TexRec m, const Texels pool, const float *uv, float v0x, float v0y, float v0z, float v1x, float v1y, float v1z,
                            float v2x, float v2y, float v2z, float px, float py, float pz, float &r, float &g, float &b) {
    float b1, b2, u, v;
    tex_barycentrics(v0x, v0y, v0z, v1x, v1y, v1z, v2x, v2y, v2z, px, py, pz, b1, b2);
    tex_interpolate(uv[0], uv[1], uv[2], uv[3], uv[4], uv[5], b1, b2, u, v);
    tex_lookup(pool + m.first, m.w, m.h, m.filter, u, v, r, g, b);
}

// The same from the triangle's record `rec` (RenderArgs::tex_bary) instead of its vertices: the form the kernels run.
template <class Texels>
PT_GRADE_FN void tex_at_hit_record(const TexRec m, const Texels pool, const float *uv, const TexBary *rec, float px, float py, float pz,
                                   float &r, float &g, float &b) {
    const TexBary t = *rec;   // (two 16-byte loads)
    float b1, b2, u, v;
    tex_barycentrics_record(t.a1[0], t.a1[1], t.a1[2], t.c1, t.a2[0], t.a2[1], t.a2[2], t.c2, px, py, pz, b1, b2);
    tex_interpolate(uv[0], uv[1], uv[2], uv[3], uv[4], uv[5], b1, b2, u, v);
    tex_lookup(pool + m.first, m.w, m.h, m.filter, u, v, r, g, b);
}

}  // namespace pt
