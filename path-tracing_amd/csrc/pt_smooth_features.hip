// The first-hit feature pass of a handle with shading normals (include/pt_hip.h: shading normals, "THE FIRST-HIT FEATURE PASS"): the twin
// of pt_texture_features.hip's feature_gather_texture_kernel, which writes normal = Ns of the first hit -- pt_smooth.hpp's interpolation,
// the one the smooth kernels run, after the flip and before any fallback -- and everything else, the textured albedo included, as that
// kernel does.  One correctly rounded float operation per step, nothing fused.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_smooth_features.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {

__global__ __launch_bounds__(256) void feature_gather_smooth_kernel(const ExactRec *__restrict__ exact, const MatRec *__restrict__ mats,
                                                                    const TexRec *__restrict__ tex_recs, const float *__restrict__ tex_uv,
                                                                    const TexTexel *__restrict__ tex_texels, const TexBary *__restrict__ tex_bary,
                                                                    const SmoothCorner *__restrict__ smooth_normals, const float *__restrict__ origins,
                                                                    const float *__restrict__ directions, const int32_t *__restrict__ hit_index,
                                                                    const float *__restrict__ hit_t, int n, float *__restrict__ position,
                                                                    float *__restrict__ normal, float *__restrict__ albedo) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const size_t o = 3 * static_cast<size_t>(p);
    const int32_t i = hit_index[p];
    float P[3] = {0.0f, 0.0f, 0.0f}, N[3] = {0.0f, 0.0f, 0.0f}, A[3] = {0.0f, 0.0f, 0.0f};
    if (i >= 0) {
        const float t = hit_t[p];
        const ExactRec &e = exact[i];   // (the table in the original triangle order: e.orig == i)
        const MatRec &m = mats[e.material];
        for (int k = 0; k < 3; ++k) {
            P[k] = origins[o + k] + directions[o + k] * t;
            A[k] = m.kd[k];
        }
        const TexBary r = tex_bary[i];
        float b1, b2;
        tex_barycentrics_record(r.a1[0], r.a1[1], r.a1[2], r.c1, r.a2[0], r.a2[1], r.a2[2], r.c2, P[0], P[1], P[2], b1, b2);
        const SmoothCorner c0 = smooth_normals[3 * static_cast<size_t>(i)], c1 = smooth_normals[3 * static_cast<size_t>(i) + 1],
                           c2 = smooth_normals[3 * static_cast<size_t>(i) + 2];
        smooth_normal(c0.x, c0.y, c0.z, c1.x, c1.y, c1.z, c2.x, c2.y, c2.z, b1, b2, e.plane[0], e.plane[1], e.plane[2],
                      [](float &x, float &y, float &z) {
                          const float inv = 1.0f / __builtin_sqrtf((x * x + y * y) + z * z);   // (correctly rounded: the build's flags)
                          x = x * inv; y = y * inv; z = z * inv;
                      },
                      N[0], N[1], N[2]);
        const TexRec tm = tex_recs[e.material];
        if (tm.w != 0) {
            const float *uv = tex_uv + 6 * static_cast<size_t>(i);
            float u, v, xr, xg, xb;
            tex_interpolate(uv[0], uv[1], uv[2], uv[3], uv[4], uv[5], b1, b2, u, v);
            tex_lookup(tex_texels + tm.first, tm.w, tm.h, tm.filter, u, v, xr, xg, xb);
            A[0] *= xr; A[1] *= xg; A[2] *= xb;
        }
    }
    for (int k = 0; k < 3; ++k) {
        position[o + k] = P[k];
        normal[o + k] = N[k];
        albedo[o + k] = A[k];
    }
}

}  // namespace

hipError_t launch_feature_gather_smooth(const ExactRec *d_exact, const MatRec *d_mats, const void *d_tex_recs, const float *d_tex_uv,
                                        const void *d_tex_texels, const void *d_tex_bary, const void *d_smooth_normals, const float *d_origins,
                                        const float *d_directions, const int32_t *d_hit_index, const float *d_hit_t, int n, float *d_position,
                                        float *d_normal, float *d_albedo, hipStream_t stream) {
    hipLaunchKernelGGL(feature_gather_smooth_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_exact, d_mats,
                       static_cast<const TexRec *>(d_tex_recs), d_tex_uv, static_cast<const TexTexel *>(d_tex_texels),
                       static_cast<const TexBary *>(d_tex_bary), static_cast<const SmoothCorner *>(d_smooth_normals), d_origins, d_directions,
                       d_hit_index, d_hit_t, n, d_position, d_normal, d_albedo);
    return hipGetLastError();
}

}  // namespace pt
