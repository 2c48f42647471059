// Launch interface of the local exposure kernels (pt_local.hip; include/pt_hip.h: pt_local_host, pt_display_present_local).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace pt {

constexpr int kLocalMaxLevels = 8;   // pt_hip.h: PT_LOCAL_MAX_LEVELS

struct LocalArgs {
    int width, height;       // of the image: W x H
    int levels;              // L, 1 .. kLocalMaxLevels
    int divide;              // 0: rgb holds the means; 1: rgb holds sums, the mean is rgb / float(count)
    const float *rgb;        // 3 floats per pixel
    const int32_t *count;    // a pixel with count == 0 is never a tap and keeps its value
    const float *exposure;   // device scalar e
    float strength;          // c > 0
    float pivot;
    float sigma;
    float *base[2];          // two planes of W x H floats: b_k is written to base[k & 1]
    float *out_rgb;          // 3 floats per pixel: m * g (may be rgb: a lane reads and writes its own pixel only)
};
// L + 2 kernels on `stream`: the luminance plane, L levels, the gain.
hipError_t launch_local(const LocalArgs &args, hipStream_t stream);

}  // namespace pt
