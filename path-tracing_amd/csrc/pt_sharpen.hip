// Sharpening (include/pt_hip.h: pt_sharpen_host, pt_display_present_sharpen): a gain per pixel from a contrast-adaptive sharpen of
// the range-compressed luminance, on the linear mean the display kernel is about to read.  The header states every operation; this
// file keeps their order, and nothing is fused.
//
// sharpen_luma_kernel: y = a / (1 + a) of the exposed luminance a, one float per pixel, or -1 for a pixel that is never a tap (no
// samples, or an a outside 0 .. 65536).  A tap is one 4-byte load and its validity one comparison.
//
// sharpen_apply_kernel: the pixel's y and the four of its ring from that plane, y', the gain l1 / l0, and m * g as a plane of means
// for the display kernel.  The taps come from the plane of y and never from the means, so the kernel may write the image it reads.
// The ring's four loads of neighbouring lanes overlap in the cache; nothing is staged in LDS.
//
// A 256-thread workgroup has a 32 x 8 tile, one lane per pixel.  Every coordinate is tested or clamped before it is used as an index,
// lanes outside the image included; only lanes inside write.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_grade.hpp"
#include "pt_sharpen.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {

constexpr int kSharpenBlock = 256;
constexpr int kTileW = 32, kTileH = 8;
static_assert(kTileW * kTileH == kSharpenBlock, "one lane per pixel of the tile");
constexpr float kInvalid = -1.0f;          // any value < 0 marks a pixel that is never a tap (a valid y is >= 0, or -0)
constexpr float kMaxExposed = 65536.0f;    // the largest a that is compressed
constexpr float kY1 = static_cast<float>(65536.0 / 65537.0);

__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }
// The header's min and max: one comparison each.
__device__ __forceinline__ float min2(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float max2(float a, float b) { return b > a ? b : a; }

// The pixel's linear mean, as the display kernels divide.
template <bool DIVIDE>
__device__ __forceinline__ void pixel_mean(const float *rgb, size_t p, int32_t c, float &r, float &g, float &b) {
    r = rgb[3 * p]; g = rgb[3 * p + 1]; b = rgb[3 * p + 2];
    if (DIVIDE) {
        const float n = static_cast<float>(c);
        r = r / n; g = g / n; b = b / n;
    }
}

struct Tile {
    int x, y;        // the lane's pixel
    bool inside;
    size_t p;        // its index, of the clamped coordinates: always inside the image
};
__device__ __forceinline__ Tile lane_pixel(int w, int h, uint32_t tiles_x) {
    Tile t;
    t.x = static_cast<int>(blockIdx.x % tiles_x) * kTileW + static_cast<int>(threadIdx.x) % kTileW;
    t.y = static_cast<int>(blockIdx.x / tiles_x) * kTileH + static_cast<int>(threadIdx.x) / kTileW;
    t.inside = t.x < w && t.y < h;
    t.p = static_cast<size_t>(clampi(t.y, h)) * w + clampi(t.x, w);
    return t;
}

struct KernelArgs {
    int w, h;
    uint32_t tiles_x;        // tiles in a row; a workgroup's tile is blockIdx.x, row by row
    const float *rgb;
    const int32_t *count;
    const float *exposure;
    float strength, limit;
    float *luma;
    float *out_rgb;
};

template <bool DIVIDE>
__global__ __launch_bounds__(kSharpenBlock) void sharpen_luma_kernel(KernelArgs a) {
    const Tile t = lane_pixel(a.w, a.h, a.tiles_x);
    if (!t.inside) return;
    const int32_t c = a.count[t.p];
    float y = kInvalid;
    if (c != 0) {
        float r, g, b;
        pixel_mean<DIVIDE>(a.rgb, t.p, c, r, g, b);
        const float l = meter_luminance(r, g, b);
        const float al = l * *a.exposure;
        if ((al >= 0.0f) && (al <= kMaxExposed)) y = al / (1.0f + al);   // (a NaN fails both)
    }
    a.luma[t.p] = y;
}

// One ring value: outside the image, or invalid, it is the centre's.
__device__ __forceinline__ float ring(const float *luma, int w, int h, int x, int y, float c) {
    const bool in_image = x >= 0 && x < w && y >= 0 && y < h;
    const float v = luma[static_cast<size_t>(clampi(y, h)) * w + clampi(x, w)];
    return (in_image && !(v < 0.0f)) ? v : c;
}

template <bool DIVIDE>
__global__ __launch_bounds__(kSharpenBlock) void sharpen_apply_kernel(KernelArgs a) {
    const Tile t = lane_pixel(a.w, a.h, a.tiles_x);
    if (!t.inside) return;
    const int32_t n = a.count[t.p];
    float r, g, b;
    if (n != 0) {
        pixel_mean<DIVIDE>(a.rgb, t.p, n, r, g, b);
        const float c = a.luma[t.p];
        if (!(c < 0.0f)) {
            const float vb = ring(a.luma, a.w, a.h, t.x, t.y - 1, c), vd = ring(a.luma, a.w, a.h, t.x - 1, t.y, c);
            const float vf = ring(a.luma, a.w, a.h, t.x + 1, t.y, c), vh = ring(a.luma, a.w, a.h, t.x, t.y + 1, c);
            const float mn = min2(min2(vb, vd), min2(vf, vh)), mx = max2(max2(vb, vd), max2(vf, vh));
            const float hmin = mx > 0.0f ? mn / (4.0f * mx) : 0.0f;
            const float hmax = (1.0f - mx) / ((4.0f * mn) - 4.0f);
            float lobe = max2(-hmin, hmax);
            lobe = min2(lobe, 0.0f);
            lobe = max2(lobe, -a.limit);
            lobe = lobe * a.strength;
            const float den = 1.0f + (4.0f * lobe);
            const float sd = (((vb - c) + (vd - c)) + (vf - c)) + (vh - c);
            float y1 = c + ((lobe * sd) / den);
            y1 = !(y1 >= 0.0f) ? 0.0f : (y1 > kY1 ? kY1 : y1);
            const float l0 = c / (1.0f - c);
            const float l1 = y1 / (1.0f - y1);
            const float gain = l0 > 0.0f ? l1 / l0 : 1.0f;
            r = r * gain; g = g * gain; b = b * gain;
        }
    } else {   // (no samples: never looked at by the display kernel; the plane keeps the input's value)
        r = a.rgb[3 * t.p]; g = a.rgb[3 * t.p + 1]; b = a.rgb[3 * t.p + 2];
    }
    a.out_rgb[3 * t.p] = r; a.out_rgb[3 * t.p + 1] = g; a.out_rgb[3 * t.p + 2] = b;
}

}  // namespace

hipError_t launch_sharpen(const SharpenArgs &s, hipStream_t stream) {
    if (s.width <= 0 || s.height <= 0 || !(s.strength > 0.0f) || !(s.strength <= 1.0f) || !(s.limit > 0.0f) || !(s.limit <= kSharpenMaxLimit))
        return hipErrorInvalidValue;
    KernelArgs a;
    a.w = s.width; a.h = s.height; a.rgb = s.rgb; a.count = s.count; a.exposure = s.exposure;
    a.strength = s.strength; a.limit = s.limit; a.luma = s.luma; a.out_rgb = s.out_rgb;
    // One grid dimension: a plane of the largest image has fewer than 2^24 tiles, whatever its shape.
    a.tiles_x = static_cast<uint32_t>((s.width + kTileW - 1) / kTileW);
    const dim3 grid(a.tiles_x * static_cast<uint32_t>((s.height + kTileH - 1) / kTileH));
    if (s.divide) {
        hipLaunchKernelGGL((sharpen_luma_kernel<true>), grid, dim3(kSharpenBlock), 0, stream, a);
        hipLaunchKernelGGL((sharpen_apply_kernel<true>), grid, dim3(kSharpenBlock), 0, stream, a);
    } else {
        hipLaunchKernelGGL((sharpen_luma_kernel<false>), grid, dim3(kSharpenBlock), 0, stream, a);
        hipLaunchKernelGGL((sharpen_apply_kernel<false>), grid, dim3(kSharpenBlock), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace pt
