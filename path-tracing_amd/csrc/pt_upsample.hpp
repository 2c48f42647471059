// Launch interface of the feature-guided upsampler (pt_upsample.hip; include/pt_hip.h: pt_upsample_host).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace pt {

// Constants of the upsampler's arithmetic, as include/pt_hip.h states them; the feature weight's defaults are the denoiser's.
constexpr int kUpsampleMinScale = 2;
constexpr int kUpsampleMaxScale = 4;
constexpr float kUpsampleMinWeight = 1e-4f;

struct UpsampleArgs {
    int width, height, scale;            // the OUTPUT size; the low image is (width / scale) x (height / scale)
    float sigma_plane;
    int normal_power_log2, demodulate;
    const float *mean_lo;                // device planes of the low image: 3 floats per pixel, and the count
    const int32_t *count_lo;
    const float *position, *normal, *albedo;   // device planes of the output image, 3 floats per pixel
    const int32_t *hit_index;
    void *rec_a, *rec_b, *rec_c;         // 16 bytes per LOW pixel each, 16-byte aligned
    float *mean_rgb;
    int32_t *count_out;
};
// The chain on one stream: the low-resolution prepare, then the full-resolution reconstruction.
hipError_t launch_upsample(const UpsampleArgs &args, hipStream_t stream);
// mean = sum / float(count) where count != 0, sum elsewhere: the unfiltered mean (pt_denoise_host with levels = 0) of planes that
// lie on the device.
hipError_t launch_upsample_mean(const float *d_sum, const int32_t *d_count, int n_px, float *d_mean, hipStream_t stream);

}  // namespace pt
