// What the display kernels share besides their statements (pt_display_body.inc): the launch shape and the table search.
// Device code; included by pt_display.hip, pt_display_graded.hip and pt_display_colour.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_display.hpp"

namespace pt {

namespace {

constexpr int kDisplayBlock = 256;
constexpr int kDisplayMaxBlocks = 2048;

// Number of thresholds <= m, for m below the last threshold in use (so the answer is below kDisplayTableSize).
__device__ __forceinline__ uint32_t display_level(const float *T, float m) {
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t step = kDisplayTableSize / 2; step; step >>= 1)
        if (T[pos + step - 1] <= m) pos += step;
    return pos;
}

}  // namespace

}  // namespace pt
