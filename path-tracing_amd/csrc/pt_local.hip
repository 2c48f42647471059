// Local exposure (include/pt_hip.h: pt_local_host, pt_display_present_local): a gain per pixel from an edge-aware base of the
// luminance, on the linear mean the display kernel is about to read.  The header states every operation; this file keeps their
// order, and nothing is fused.
//
// local_luma_kernel: b_0, one float per pixel -- the meter's luminance of the mean, or -1 for a pixel that is never a tap (no
// samples, or a luminance outside 0 .. 2^64).  Every later plane keeps that mark, so a tap is one 4-byte load and its validity one
// comparison.
//
// local_atrous_kernel: a 256-thread workgroup makes a 32 x 8 tile of b_{k+1} from the 25 taps of b_k at spacing 2^k.  At spacing
// 1 and 2 the tile's taps lie in a 36 x 12 and a 40 x 16 region that its lanes share, staged through LDS with -1 where the
// region leaves the image, so that "outside" and "invalid" are the same comparison; a wave reads two rows of 32 consecutive floats
// per tap, and no two lanes of a 32-lane half meet on a bank.  From spacing 4 on the taps of neighbouring lanes are 4 and more
// floats apart and no longer shared within the tile: they come from global memory, as the denoiser's levels do.
// -DPT_LOCAL_NO_LDS builds every level in that form (make local-variant, tools/local_study.py).
//
// local_apply_kernel: g from b_L and the device scalar e, and m * g as a plane of means for the display kernel.
//
// Every coordinate is tested or clamped before it is used as an index, lanes outside the image included; only lanes inside write.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_grade.hpp"
#include "pt_local.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {

constexpr int kLocalBlock = 256;
constexpr int kTileW = 32, kTileH = 8;   // a workgroup's tile of the plane it writes
static_assert(kTileW * kTileH == kLocalBlock, "one lane per pixel of the tile");
constexpr float kInvalid = -1.0f;        // any negative value marks a pixel that is never a tap
constexpr float kMaxLuminance = 18446744073709551616.0f;   // 2^64

__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// The pixel's linear mean, as the display kernels divide.
template <bool DIVIDE>
__device__ __forceinline__ void pixel_mean(const float *rgb, size_t p, int32_t c, float &r, float &g, float &b) {
    r = rgb[3 * p]; g = rgb[3 * p + 1]; b = rgb[3 * p + 2];
    if (DIVIDE) {
        const float n = static_cast<float>(c);
        r = r / n; g = g / n; b = b / n;
    }
}

struct LumaArgs {
    int n;
    const float *rgb;
    const int32_t *count;
    float *base;             // b_0
};

template <bool DIVIDE>
__global__ __launch_bounds__(kLocalBlock) void local_luma_kernel(LumaArgs a) {
    const int p = static_cast<int>(blockIdx.x) * kLocalBlock + static_cast<int>(threadIdx.x);
    if (p >= a.n) return;
    const int32_t c = a.count[p];
    float l = kInvalid;
    if (c != 0) {
        float r, g, b;
        pixel_mean<DIVIDE>(a.rgb, static_cast<size_t>(p), c, r, g, b);
        l = meter_luminance(r, g, b);
        if (!(l >= 0.0f) || !(l <= kMaxLuminance)) l = kInvalid;   // (a NaN fails both)
    }
    a.base[p] = l;
}

// The 5 x 5 B3 spline: (1 4 6 4 1)/16 x (1 4 6 4 1)/16, every product exact.
__device__ __forceinline__ float spline1(int j) { return j == 0 ? 0.375f : ((j == 1 || j == -1) ? 0.25f : 0.0625f); }

// One tap into the two sums: bq < 0 (invalid, or outside the image) adds nothing.
__device__ __forceinline__ void tap(float bp, float bq, float spline, float sigma, float &sw, float &sd) {
    const float d = bq - bp;
    const float mn = bq < bp ? bq : bp;
    const float s = (sigma * mn) + 1e-30f;
    const float r = d / s;
    const float wr = 1.0f / (1.0f + (r * r));
    const float w = spline * wr;
    if (!(bq < 0.0f)) {
        sw = sw + w;
        sd = sd + (w * d);
    }
}

struct AtrousArgs {
    int w, h;
    int step;                // 2^k: the spacing of the taps
    uint32_t tiles_x;        // tiles in a row; a workgroup's tile is blockIdx.x, row by row
    float sigma;
    const float *in;         // b_k
    float *out;              // b_{k+1}
};

// STAGE = 1, 2: spacing STAGE, the taps from an LDS tile.  STAGE = 0: spacing a.step, the taps from global memory.
template <int STAGE>
__global__ __launch_bounds__(kLocalBlock) void local_atrous_kernel(AtrousArgs a) {
    const int x0 = static_cast<int>(blockIdx.x % a.tiles_x) * kTileW, y0 = static_cast<int>(blockIdx.x / a.tiles_x) * kTileH;
    const int tx = static_cast<int>(threadIdx.x) % kTileW, ty = static_cast<int>(threadIdx.x) / kTileW;
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < a.w && y < a.h;
    float sw = 0.0f, sd = 0.0f, bp;
    if constexpr (STAGE != 0) {
        constexpr int kHalo = 2 * STAGE, kW = kTileW + 2 * kHalo, kH = kTileH + 2 * kHalo;
        __shared__ float T[kW * kH];
        for (int i = static_cast<int>(threadIdx.x); i < kW * kH; i += kLocalBlock) {
            const int gx = x0 - kHalo + i % kW, gy = y0 - kHalo + i / kW;
            const bool in_image = gx >= 0 && gx < a.w && gy >= 0 && gy < a.h;
            const float v = a.in[static_cast<size_t>(clampi(gy, a.h)) * a.w + clampi(gx, a.w)];
            T[i] = in_image ? v : kInvalid;
        }
        __syncthreads();
        const float *t = T + (ty + kHalo) * kW + (tx + kHalo);
        bp = t[0];
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx)
                tap(bp, t[dy * STAGE * kW + dx * STAGE], spline1(dy) * spline1(dx), a.sigma, sw, sd);
    } else {
        const int cx = clampi(x, a.w), cy = clampi(y, a.h);
        bp = a.in[static_cast<size_t>(cy) * a.w + cx];
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
            const int qy = cy + dy * a.step;
            const bool row_in = qy >= 0 && qy < a.h;
            const size_t line = static_cast<size_t>(clampi(qy, a.h)) * a.w;
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int qx = cx + dx * a.step;
                const bool in_image = row_in && qx >= 0 && qx < a.w;
                const float v = a.in[line + clampi(qx, a.w)];
                tap(bp, in_image ? v : kInvalid, spline1(dy) * spline1(dx), a.sigma, sw, sd);
            }
        }
    }
    if (!inside) return;
    // (an invalid pixel keeps its mark; a valid one has its own tap in sw, 0.140625 at least)
    a.out[static_cast<size_t>(y) * a.w + x] = bp < 0.0f ? bp : bp + (sd / sw);
}

struct ApplyArgs {
    int n;
    const float *rgb;
    const int32_t *count;
    const float *base;       // b_L
    const float *exposure;
    float strength, pivot;
    float *out_rgb;
};

template <bool DIVIDE>
__global__ __launch_bounds__(kLocalBlock) void local_apply_kernel(ApplyArgs a) {
    const int i = static_cast<int>(blockIdx.x) * kLocalBlock + static_cast<int>(threadIdx.x);
    if (i >= a.n) return;
    const size_t p = static_cast<size_t>(i);
    const int32_t c = a.count[p];
    float r, g, b;
    if (c != 0) {
        pixel_mean<DIVIDE>(a.rgb, p, c, r, g, b);
        const float base = a.base[p];
        if (!(base < 0.0f)) {
            const float e = *a.exposure;
            const float al = base * e;
            const float gain = (1.0f + a.strength) / (1.0f + ((a.strength * al) / a.pivot));
            r = r * gain; g = g * gain; b = b * gain;
        }
    } else {   // (no samples: never looked at by the display kernel; the plane keeps the input's value)
        r = a.rgb[3 * p]; g = a.rgb[3 * p + 1]; b = a.rgb[3 * p + 2];
    }
    a.out_rgb[3 * p] = r; a.out_rgb[3 * p + 1] = g; a.out_rgb[3 * p + 2] = b;
}

dim3 pixels(int n) { return dim3(static_cast<uint32_t>((n + kLocalBlock - 1) / kLocalBlock)); }

}  // namespace

hipError_t launch_local(const LocalArgs &l, hipStream_t stream) {
    if (l.width <= 0 || l.height <= 0 || l.levels < 1 || l.levels > kLocalMaxLevels) return hipErrorInvalidValue;
    const int n = l.width * l.height;
    LumaArgs la;
    la.n = n; la.rgb = l.rgb; la.count = l.count; la.base = l.base[0];
    if (l.divide) hipLaunchKernelGGL((local_luma_kernel<true>), pixels(n), dim3(kLocalBlock), 0, stream, la);
    else hipLaunchKernelGGL((local_luma_kernel<false>), pixels(n), dim3(kLocalBlock), 0, stream, la);
    // One grid dimension: a plane of the largest image has fewer than 2^24 tiles, whatever its shape.
    AtrousArgs a;
    a.w = l.width; a.h = l.height; a.sigma = l.sigma;
    a.tiles_x = static_cast<uint32_t>((l.width + kTileW - 1) / kTileW);
    const dim3 grid(a.tiles_x * static_cast<uint32_t>((l.height + kTileH - 1) / kTileH));
    for (int k = 0; k < l.levels; ++k) {
        a.step = 1 << k; a.in = l.base[k & 1]; a.out = l.base[(k + 1) & 1];
#if !defined(PT_LOCAL_NO_LDS)
        if (k == 0) hipLaunchKernelGGL((local_atrous_kernel<1>), grid, dim3(kLocalBlock), 0, stream, a);
        else if (k == 1) hipLaunchKernelGGL((local_atrous_kernel<2>), grid, dim3(kLocalBlock), 0, stream, a);
        else
#endif
            hipLaunchKernelGGL((local_atrous_kernel<0>), grid, dim3(kLocalBlock), 0, stream, a);
    }
    ApplyArgs p;
    p.n = n; p.rgb = l.rgb; p.count = l.count; p.base = l.base[l.levels & 1]; p.exposure = l.exposure;
    p.strength = l.strength; p.pivot = l.pivot; p.out_rgb = l.out_rgb;
    if (l.divide) hipLaunchKernelGGL((local_apply_kernel<true>), pixels(n), dim3(kLocalBlock), 0, stream, p);
    else hipLaunchKernelGGL((local_apply_kernel<false>), pixels(n), dim3(kLocalBlock), 0, stream, p);
    return hipGetLastError();
}

}  // namespace pt
