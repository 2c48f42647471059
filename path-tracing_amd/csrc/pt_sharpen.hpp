// Launch interface of the sharpening kernels (pt_sharpen.hip; include/pt_hip.h: pt_sharpen_host, pt_display_present_sharpen).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace pt {

constexpr float kSharpenMaxLimit = 0.1875f;   // pt_hip.h: the largest (and the default) limit; 1 - 4 limit = 0.25 > 0

struct SharpenArgs {
    int width, height;       // of the image: W x H
    int divide;              // 0: rgb holds the means; 1: rgb holds sums, the mean is rgb / float(count)
    const float *rgb;        // 3 floats per pixel
    const int32_t *count;    // a pixel with count == 0 is never a tap and keeps its value
    const float *exposure;   // device scalar e
    float strength;          // in (0, 1]
    float limit;             // in (0, kSharpenMaxLimit]
    float *luma;             // a plane of W x H floats: y, or a negative value for a pixel that is never a tap
    float *out_rgb;          // 3 floats per pixel: m * g (may be rgb: the taps come from luma, and a lane reads and writes its own pixel only)
};
// 2 kernels on `stream`: the plane of compressed luminance, the gain.
hipError_t launch_sharpen(const SharpenArgs &args, hipStream_t stream);

}  // namespace pt
