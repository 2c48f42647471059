// Launch interface of the display kernel (pt_display.hip; include/pt_hip.h: pt_display_*): linear means to image bytes.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "pt_colour.hpp"
#include "pt_grain.hpp"

namespace pt {

// Thresholds the kernel searches: the host's table (pt_display_table), padded with +inf to this length.
constexpr int kDisplayTableSize = 4096;

// One entry of the list of pixels the kernel leaves to the host: 16 bytes.
struct DisplayDeferred {
    int32_t pixel;
    float mean[3];   // r, g, b: what the host tone-maps and quantizes
};

struct DisplayArgs {
    int n;                       // pixels of the flat plane
    int divide;                  // 0: rgb holds the means; 1: rgb holds sums, the mean is rgb / float(count)
    const float *rgb;            // 3 floats per pixel, 16-byte aligned
    const int32_t *count;        // 16-byte aligned; a pixel with count == 0 gets three zero bytes
    const float *table;          // kDisplayTableSize thresholds, non-decreasing, +inf behind the last one in use; 16-byte aligned
    float last;                  // the last threshold in use: a mean at or above it is deferred
    int n_bands;                 // doubt bands [band_lo[i], band_hi[i]): a mean inside one is deferred
    const float *band_lo, *band_hi;
    uint32_t *bgr;               // 3 bytes per pixel (B, G, R), written as dwords: room for (n + 3) / 4 * 12 bytes
    DisplayDeferred *deferred;   // room for n entries, 16-byte aligned
    uint32_t *n_deferred;        // zero before the launch
};
// One kernel: per channel the number of thresholds <= the mean, & 255; deferred pixels go to the list with zero bytes.
hipError_t launch_display(const DisplayArgs &args, hipStream_t stream);
// The same with grading (pt_display_graded.hip): per channel g = curve(mean * *exposure) is what is looked up and what decides
// whether a pixel is deferred; a deferred entry still carries the ungraded mean.  `curve` is a PT_CURVE_* (pt_grade.hpp), `exposure`
// a device scalar written earlier on `stream`.
hipError_t launch_display_graded(const DisplayArgs &args, int curve, const float *exposure, hipStream_t stream);
// The same with colour grading (pt_display_colour.hip): per pixel matrix -> exposure -> curve -> LUT (pt_colour.hpp) makes the g;
// a deferred entry carries the mean before the matrix.  `colour.lut` is device memory, valid until the kernel has finished.
hipError_t launch_display_colour(const DisplayArgs &args, int curve, const float *exposure, const ColourStep &colour, hipStream_t stream);
// The same with film grain and dither (pt_display_grain.hip): g takes the pixel's grain behind the LUT (pt_grain.hpp), and the level of
// a channel the table covers is dithered between the thresholds round it.  `grain.width` is the image's, `grain.size` is in 1 .. 8.
hipError_t launch_display_grain(const DisplayArgs &args, int curve, const float *exposure, const ColourStep &colour, const GrainStep &grain,
                                hipStream_t stream);

}  // namespace pt
