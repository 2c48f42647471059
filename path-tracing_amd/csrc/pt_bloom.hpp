// Launch interface of the bloom kernels (pt_bloom.hip; include/pt_hip.h: pt_bloom_host, pt_display_present_bloom).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace pt {

constexpr int kBloomMaxLevels = 8;   // pt_hip.h: PT_BLOOM_MAX_LEVELS

// The size of pyramid level k >= 1 from level k - 1's.
inline int bloom_half(int v) { return (v + 1) >> 1; }
// 16-byte records of levels 1 .. levels of a width x height image, back to back: what BloomArgs::pyramid holds.
inline size_t bloom_pyramid_records(int width, int height, int levels) {
    size_t records = 0;
    for (int k = 1; k <= levels; ++k) {
        width = bloom_half(width); height = bloom_half(height);
        records += static_cast<size_t>(width) * height;
    }
    return records;
}

struct BloomArgs {
    int width, height;       // of the image: W x H
    int levels;              // L, 1 .. kBloomMaxLevels
    int divide;              // 0: rgb holds the means; 1: rgb holds sums, the mean is rgb / float(count)
    const float *rgb;        // 3 floats per pixel
    const int32_t *count;    // a pixel with count == 0 adds nothing and keeps its value
    const float *exposure;   // device scalar e: the bright pass starts at T / e
    float threshold;         // T
    float weight;            // S / (float)L, divided on the host
    void *pyramid;           // bloom_pyramid_records(width, height, levels) records of 16 bytes, 16-byte aligned
    float *out_rgb;          // 3 floats per pixel: m + A * weight (not rgb)
};
// 2 L kernels on `stream`: L down (the first with the bright pass), L up (the last with the output).
hipError_t launch_bloom(const BloomArgs &args, hipStream_t stream);

}  // namespace pt
