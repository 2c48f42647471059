// Launch interface of the first-hit feature kernels and of the feature-guided denoiser (pt_denoise.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "pt_scene.hpp"

namespace pt {

// Constants of the denoiser's arithmetic, as include/pt_hip.h states them (pt_denoise_host).
constexpr int kDenoiseMaxLevels = 8;
constexpr float kDenoiseSigmaLuminance = 4.0f;
constexpr float kDenoiseSigmaPlane = 0.1f;
constexpr int kDenoiseNormalPowerLog2 = 7;
constexpr int kDenoiseMaxNormalPowerLog2 = 16;
constexpr float kDenoiseAlbedoFloor = 0.01f;
constexpr float kDenoiseTiny = 1e-6f;
constexpr float kDenoiseFillMinWeight = 1e-4f;
constexpr int kDenoiseSpatialBelow = 4;

struct FeatureCamera {
    float v[12];   // origin, right, up, forward (pt_camera)
};

// Rays through the centres of the pixels of rows [row_begin, row_begin + rows): origins / directions, 3 floats per pixel.
hipError_t launch_feature_rays(const FeatureCamera &cam, int width, int height, int row_begin, int rows, float *d_origins,
                               float *d_directions, hipStream_t stream);
// position = origin + direction * t, the hit triangle's stored plane normal, Kd of its material; zeros on a miss.
hipError_t launch_feature_gather(const ExactRec *d_exact, const MatRec *d_mats, const float *d_origins, const float *d_directions,
                                 const int32_t *d_hit_index, const float *d_hit_t, int n, float *d_position, float *d_normal,
                                 float *d_albedo, hipStream_t stream);

struct DenoiseArgs {
    int width, height, levels;
    float sigma_luminance, sigma_plane;
    int normal_power_log2, demodulate;
    const float *sum, *sum2;          // device planes, 3 floats per pixel
    const int32_t *count;
    const float *position, *normal, *albedo;
    const int32_t *hit_index;
    void *rec_a0, *rec_a1, *rec_b, *rec_c;   // 16 bytes per pixel each, 16-byte aligned
    float *mean_rgb;
    int32_t *count_out;
};
// The whole chain on one stream, no host synchronisation in between: prepare, variance estimate, `levels` a-trous passes, finish.
hipError_t launch_denoise(const DenoiseArgs &args, hipStream_t stream);

}  // namespace pt
