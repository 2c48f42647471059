// Launch interface of the metering kernels (pt_meter.hip; include/pt_hip.h: pt_meter_host, pt_display_present_graded).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "pt_grade.hpp"

namespace pt {

struct MeterArgs {
    int n;                  // pixels of the flat plane
    int divide;             // 0: rgb holds the means; 1: rgb holds sums, the mean is rgb / float(count)
    const float *rgb;       // 3 floats per pixel, 16-byte aligned
    const int32_t *count;   // 16-byte aligned; a pixel with count == 0 is not metered
    uint32_t *hist;         // kMeterEntries counts, zero before the launch
};
// hist[meter_bin(lum(mean))] += 1 for every pixel with samples: exact, whatever the order.
hipError_t launch_meter(const MeterArgs &args, hipStream_t stream);

// What exposure_kernel leaves for the display kernel (the first word) and for the host.
struct ExposureOut {
    float exposure;     // e
    float target;       // e*
    uint32_t metered;   // pixels in bins 0 .. 127
    uint32_t dark;      // hist[kMeterDark]
};
// One wave: *out = exposure_from_histogram(hist, rule, has_prev, e_prev) of pt_grade.hpp, behind the meter on the same stream.
hipError_t launch_exposure(const uint32_t *hist, const ExposureRule &rule, bool has_prev, float e_prev, ExposureOut *out, hipStream_t stream);

}  // namespace pt
