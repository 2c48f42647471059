// Launch interface of the lens optics kernel (pt_optics.hip; include/pt_hip.h: pt_optics_host, pt_display_present_optics).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace pt {

struct OpticsArgs {
    int width, height;       // of the image: W x H, read and written
    int divide;              // 0: rgb holds the means; 1: rgb holds sums, a tap's mean is rgb / float(count)
    const float *rgb;        // 3 floats per pixel
    const int32_t *count;    // a pixel with count == 0 is never a tap
    float k1, k2;            // f = 1 + r2 (k1 + k2 r2)
    float mag[3];            // per channel: 1 - ca, 1, 1 + ca, rounded once on the host
    float vignette;
    float *out_rgb;          // 3 floats per pixel; a gather: NOT rgb
    int32_t *out_count;      // 1, or 0 where a channel found no tap; NOT count
};
// One kernel on `stream`.  hipErrorInvalidValue, and nothing launched, for an empty image or an output plane that is an input.
hipError_t launch_optics(const OpticsArgs &args, hipStream_t stream);

}  // namespace pt
