// Launch interface of the temporal accumulation stage (pt_temporal.hip; include/pt_hip.h: pt_temporal_push_host).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace pt {

// Constants of the stage's arithmetic, as include/pt_hip.h states them.
constexpr float kTemporalMaxFrames = 32.0f;
constexpr float kTemporalSigmaPlane = 0.1f;
constexpr float kTemporalMinNormalDot = 0.9f;
constexpr float kTemporalMinWeight = 1e-3f;

enum TemporalMode : int {
    kTemporalFirstFrame = 0,   // no history: the merge copies
    kTemporalStatic = 1,       // the camera did not move: the only tap is the pixel itself
    kTemporalReproject = 2,
};

// The history of one frame: four 16-byte records per pixel, each plane 16-byte aligned.
struct TemporalRecords {
    void *sum_n;      // Hs.xyz, Hn
    void *sum2_age;   // Hs2.xyz, HL
    void *normal;     // N'.xyz, hit flag (1 = a triangle, 0 = a miss)
    void *position;   // P'.xyz, 0
};

struct TemporalArgs {
    int width, height, mode;
    float max_frames, sigma_plane, min_normal_dot;
    float cam[12];           // the current camera: origin, right, up, forward (pt_camera)
    float prev_origin[3];    // of the history's camera
    float prev_inverse[9];   // rows i0, i1, i2 of the inverse of [right' up' forward']
    const float *sum, *sum2;   // the frame's accumulators, device planes
    const int32_t *count;
    const float *position, *normal;   // the frame's feature planes
    const int32_t *hit_index;
    TemporalRecords prev, next;       // read / written; never the same planes
    float *sum_out, *sum2_out;
    int32_t *count_out;
    float *history_frames;
};
// One kernel: reproject, test, interpolate, cap, merge, write the new history and the output planes.
hipError_t launch_temporal_merge(const TemporalArgs &args, hipStream_t stream);

}  // namespace pt
