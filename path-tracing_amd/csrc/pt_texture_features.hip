// The first-hit feature pass of a handle with a texture list (include/pt_hip.h: pt_texture, "THE FIRST-HIT FEATURE PASS"): the twin of
// pt_denoise.hip's feature_gather_kernel, which writes albedo = Kd x texel for a hit on a textured material -- the lookup of
// pt_texture.hpp, the one the texture kernels run -- and everything else as that kernel does.  One correctly rounded float operation
// per step, nothing fused.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_texture_features.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {

__global__ __launch_bounds__(256) void feature_gather_texture_kernel(const ExactRec *__restrict__ exact, const MatRec *__restrict__ mats,
                                                                     const TexRec *__restrict__ tex_recs, const float *__restrict__ tex_uv,
                                                                     const TexTexel *__restrict__ tex_texels, const TexBary *__restrict__ tex_bary, const float *__restrict__ origins,
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
            N[k] = e.plane[k];
            A[k] = m.kd[k];
        }
        const TexRec tm = tex_recs[e.material];
        if (tm.w != 0) {
            float xr, xg, xb;
            tex_at_hit_record(tm, tex_texels, tex_uv + 6 * static_cast<size_t>(i), tex_bary + i, P[0], P[1], P[2], xr, xg, xb);
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

hipError_t launch_feature_gather_textured(const ExactRec *d_exact, const MatRec *d_mats, const void *d_tex_recs, const float *d_tex_uv,
                                          const void *d_tex_texels, const void *d_tex_bary, const float *d_origins, const float *d_directions, const int32_t *d_hit_index,
                                          const float *d_hit_t, int n, float *d_position, float *d_normal, float *d_albedo, hipStream_t stream) {
    hipLaunchKernelGGL(feature_gather_texture_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_exact, d_mats,
                       static_cast<const TexRec *>(d_tex_recs), d_tex_uv, static_cast<const TexTexel *>(d_tex_texels), static_cast<const TexBary *>(d_tex_bary), d_origins, d_directions,
                       d_hit_index, d_hit_t, n, d_position, d_normal, d_albedo);
    return hipGetLastError();
}

}  // namespace pt
