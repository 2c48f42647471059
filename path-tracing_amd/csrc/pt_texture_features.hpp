// Launch interface of the textured first-hit feature gather (pt_texture_features.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "pt_scene.hpp"
#include "pt_texture.hpp"

namespace pt {

// pt_denoise.hpp's launch_feature_gather for a handle with a texture list: albedo = Kd x texel where the first hit's material is
// textured (d_tex_recs, d_tex_uv, d_tex_texels, d_tex_bary: RenderArgs::tex_recs, tex_uv, tex_texels, tex_bary), everything else the same.
hipError_t launch_feature_gather_textured(const ExactRec *d_exact, const MatRec *d_mats, const void *d_tex_recs, const float *d_tex_uv,
                                          const void *d_tex_texels, const void *d_tex_bary, const float *d_origins, const float *d_directions, const int32_t *d_hit_index,
                                          const float *d_hit_t, int n, float *d_position, float *d_normal, float *d_albedo, hipStream_t stream);

}  // namespace pt
