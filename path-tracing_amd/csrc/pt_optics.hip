// Lens optics (include/pt_hip.h: pt_optics_host, pt_display_present_optics): radial distortion, lateral chromatic aberration and
// cos^4 vignetting as one resample of the linear mean, ahead of the meter.  The header states every operation; this file keeps
// their order, and nothing is fused.
//
// optics_kernel: one lane per output pixel, a 256-thread workgroup per 32 x 8 tile.  A lane computes the pixel's r2 and f once,
// then per channel a source position of its own and four taps there: twelve 4-byte reads and up to twelve count reads, none of
// them shared with another channel in general (with ca = 0 the three positions coincide and the compiler's loads do too).  The
// taps of neighbouring lanes are neighbours in the source unless |f| is large, so a wave's reads of one tap fall in a few
// cache lines; there is no LDS tile.
//
// A source position is clamped to the image before it becomes an index, and x1, y1 are clamped again; lanes outside the image
// leave before they read.  The kernel writes its own pixel of out_rgb and out_count only, and these are not the input planes
// (launch_optics refuses that): every other lane reads them.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_optics.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {

constexpr int kOpticsBlock = 256;
constexpr int kTileW = 32, kTileH = 8;   // a workgroup's tile of the plane it writes
static_assert(kTileW * kTileH == kOpticsBlock, "one lane per pixel of the tile");

// !(s >= 0) ? 0 : (s > hi ? hi : s): a NaN goes to 0.
__device__ __forceinline__ float clamp_position(float s, float hi) { return !(s >= 0.0f) ? 0.0f : (s > hi ? hi : s); }

// The weighted mean of the taps kept, about the first of them.
struct TapSum {
    float ref = 0.0f, sw = 0.0f, sd = 0.0f;
    bool any = false;
};

template <bool DIVIDE>
__device__ __forceinline__ void tap(const OpticsArgs &a, int ch, int x, int y, float w, TapSum &s) {
    if (w == 0.0f) return;
    const size_t p = static_cast<size_t>(y) * a.width + x;
    const int32_t c = a.count[p];
    if (c == 0) return;
    float m = a.rgb[3 * p + ch];
    if (DIVIDE) m = m / static_cast<float>(c);
    if (!s.any) {
        s.any = true; s.ref = m; s.sw = w;
    } else {
        s.sw = s.sw + w;
        s.sd = s.sd + (w * (m - s.ref));
    }
}

// Channel ch resampled at the position scale s maps (px, py) to: false if no tap was kept.
template <bool DIVIDE>
__device__ __forceinline__ bool resample(const OpticsArgs &a, int ch, float cx, float cy, float px, float py, float s, float &val) {
    const float sx = clamp_position(cx + (px * s), static_cast<float>(a.width - 1));
    const float sy = clamp_position(cy + (py * s), static_cast<float>(a.height - 1));
    const int x0 = static_cast<int>(sx), y0 = static_cast<int>(sy);
    const float fx = sx - static_cast<float>(x0), fy = sy - static_cast<float>(y0);
    const int x1 = x0 + 1 > a.width - 1 ? a.width - 1 : x0 + 1, y1 = y0 + 1 > a.height - 1 ? a.height - 1 : y0 + 1;
    const float wx0 = 1.0f - fx, wy0 = 1.0f - fy;
    TapSum t;
    tap<DIVIDE>(a, ch, x0, y0, wx0 * wy0, t);
    tap<DIVIDE>(a, ch, x1, y0, fx * wy0, t);
    tap<DIVIDE>(a, ch, x0, y1, wx0 * fy, t);
    tap<DIVIDE>(a, ch, x1, y1, fx * fy, t);
    if (!t.any) return false;
    val = t.ref + (t.sd / t.sw);
    return true;
}

template <bool DIVIDE>
__global__ __launch_bounds__(kOpticsBlock) void optics_kernel(OpticsArgs a, uint32_t tiles_x) {
    const int x = static_cast<int>(blockIdx.x % tiles_x) * kTileW + static_cast<int>(threadIdx.x) % kTileW;
    const int y = static_cast<int>(blockIdx.x / tiles_x) * kTileH + static_cast<int>(threadIdx.x) / kTileW;
    if (x >= a.width || y >= a.height) return;
    const float cx = 0.5f * static_cast<float>(a.width - 1), cy = 0.5f * static_cast<float>(a.height - 1);
    const float px = static_cast<float>(x) - cx, py = static_cast<float>(y) - cy;
    const float hh = 0.5f * static_cast<float>(a.height);
    const float u = px / hh, v = py / hh;
    const float r2 = (u * u) + (v * v);
    const float f = 1.0f + (r2 * (a.k1 + (a.k2 * r2)));
    float val[3];
    bool full = true;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) full = resample<DIVIDE>(a, ch, cx, cy, px, py, f * a.mag[ch], val[ch]) && full;
    const float q = 1.0f + (a.vignette * r2);
    const float gain = 1.0f / (q * q);
    const size_t p = static_cast<size_t>(y) * a.width + x;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) a.out_rgb[3 * p + ch] = full ? val[ch] * gain : 0.0f;
    a.out_count[p] = full ? 1 : 0;
}

}  // namespace

hipError_t launch_optics(const OpticsArgs &a, hipStream_t stream) {
    if (a.width <= 0 || a.height <= 0 || !a.rgb || !a.count || !a.out_rgb || !a.out_count) return hipErrorInvalidValue;
    if (a.out_rgb == a.rgb || a.out_count == a.count) return hipErrorInvalidValue;
    // One grid dimension: the largest image, 2^29 pixels, has at most 2^26 tiles, whatever its shape.
    const uint32_t tiles_x = static_cast<uint32_t>((a.width + kTileW - 1) / kTileW);
    const dim3 grid(tiles_x * static_cast<uint32_t>((a.height + kTileH - 1) / kTileH));
    if (a.divide) hipLaunchKernelGGL((optics_kernel<true>), grid, dim3(kOpticsBlock), 0, stream, a, tiles_x);
    else hipLaunchKernelGGL((optics_kernel<false>), grid, dim3(kOpticsBlock), 0, stream, a, tiles_x);
    return hipGetLastError();
}

}  // namespace pt
