// Launch interface of the first-hit feature gather of a handle with shading normals (pt_smooth_features.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "pt_scene.hpp"
#include "pt_smooth.hpp"
#include "pt_texture.hpp"

namespace pt {

// pt_texture_features.hpp's launch_feature_gather_textured for a handle with shading normals: normal = Ns of the first hit (after the
// flip, before any fallback; d_smooth_normals: RenderArgs::smooth_normals), albedo = Kd x texel where the material is textured (an
// all-zero table without a list), everything else the same.
hipError_t launch_feature_gather_smooth(const ExactRec *d_exact, const MatRec *d_mats, const void *d_tex_recs, const float *d_tex_uv,
                                        const void *d_tex_texels, const void *d_tex_bary, const void *d_smooth_normals, const float *d_origins,
                                        const float *d_directions, const int32_t *d_hit_index, const float *d_hit_t, int n, float *d_position,
                                        float *d_normal, float *d_albedo, hipStream_t stream);

}  // namespace pt
