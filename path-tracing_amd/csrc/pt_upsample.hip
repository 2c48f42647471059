// Feature-guided upsampling of a frame traced at reduced resolution (include/pt_hip.h: pt_upsample_host).  The header states the
// arithmetic; everything here is one correctly rounded float operation per step in that order, nothing fused (the Makefile builds
// with -ffp-contract=off and IEEE divide), so tests/upsample_restatement.py reproduces the results bit for bit in numpy.
//
// What a tap reads is packed into three 16-byte records per LOW pixel, as the denoiser packs its own:
//   A  c.xyz (the low mean divided by the guide's albedo) + data flag (1 = count_lo > 0)
//   B  the guide's normal.xyz + hit flag (1 = a triangle, 0 = a miss)
//   C  the guide's position.xyz + 0
// so a tap is three 16-byte loads.  A workgroup is 32 x 8 output pixels; its taps cover at most (31 / s + 3) x (7 / s + 3) low
// pixels -- 5 KB of records at s = 2, which 256 lanes read 12 288 times: the footprint lives in the L1 / L2 and the kernel reads it
// from global memory (the variant that stages it in LDS first is kept behind -DPT_UPSAMPLE_LDS for the A/B: profiles/upsample_1080p.txt).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_denoise.hpp"
#include "pt_feature_weight.hpp"
#include "pt_upsample.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {

__global__ __launch_bounds__(256) void upsample_mean_kernel(const float *__restrict__ sum, const int32_t *__restrict__ count, int n_px,
                                                            float *__restrict__ mean) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_px) return;
    const size_t p = static_cast<size_t>(i);
    const int32_t cnt = count[p];
    const float n = static_cast<float>(cnt);
    for (int k = 0; k < 3; ++k) {
        const float s = sum[3 * p + k];
        mean[3 * p + k] = cnt != 0 ? s / n : s;
    }
}

// the demodulation divisor of a pixel: its albedo, floored, if it is a hit and the stage demodulates
__device__ __forceinline__ float divisor(float albedo, bool demodulate_hit) {
    return demodulate_hit ? (albedo > kDenoiseAlbedoFloor ? albedo : kDenoiseAlbedoFloor) : 1.0f;
}

// Step 1, per low pixel Q: its guide g(Q) = (s X + s / 2, s Y + s / 2) of the output image, c = m / a, the guide's features.
__global__ __launch_bounds__(256) void upsample_prepare_kernel(UpsampleArgs a, int w, int n_lo) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_lo) return;
    const int X = i % w, Y = i / w;
    const size_t q = static_cast<size_t>(i);
    const size_t g = static_cast<size_t>(a.scale * Y + a.scale / 2) * a.width + (a.scale * X + a.scale / 2);
    const bool hit = a.hit_index[g] >= 0;
    const bool dm = a.demodulate && hit;
    const float c0 = a.mean_lo[3 * q] / divisor(a.albedo[3 * g], dm);
    const float c1 = a.mean_lo[3 * q + 1] / divisor(a.albedo[3 * g + 1], dm);
    const float c2 = a.mean_lo[3 * q + 2] / divisor(a.albedo[3 * g + 2], dm);
    static_cast<float4 *>(a.rec_a)[q] = make_float4(c0, c1, c2, a.count_lo[q] > 0 ? 1.0f : 0.0f);
    static_cast<float4 *>(a.rec_b)[q] = make_float4(a.normal[3 * g], a.normal[3 * g + 1], a.normal[3 * g + 2], hit ? 1.0f : 0.0f);
    static_cast<float4 *>(a.rec_c)[q] = make_float4(a.position[3 * g], a.position[3 * g + 1], a.position[3 * g + 2], 0.0f);
}

#ifdef PT_UPSAMPLE_LDS
constexpr bool kStageInLds = true;
#else
constexpr bool kStageInLds = false;
#endif

// Steps 2 - 5, per output pixel: four taps of the low grid, the heaviest used one the base.  S = the scale, a compile-time constant
// (the divisions by s and 2 s are by constants).
template <int S>
__global__ __launch_bounds__(256) void upsample_kernel(UpsampleArgs a, int w, int h) {
    constexpr int kFootW = 31 / S + 3, kFootH = 7 / S + 3;   // taps of 32 x 8 pixels: 18 x 6, 13 x 5, 10 x 4 low pixels
    __shared__ float4 lds[kStageInLds ? 3 * kFootW * kFootH : 1];
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    const float4 *A = static_cast<const float4 *>(a.rec_a), *B = static_cast<const float4 *>(a.rec_b), *Cc = static_cast<const float4 *>(a.rec_c);
    // the tile's first tap: floor((2 x + 1 - S) / (2 S)) of the tile's first pixel, in integers (a negative numerator is above -2 S)
    const int nx0 = 64 * static_cast<int>(blockIdx.x) + 1 - S, ny0 = 16 * static_cast<int>(blockIdx.y) + 1 - S;
    const int fx0 = nx0 >= 0 ? nx0 / (2 * S) : -1, fy0 = ny0 >= 0 ? ny0 / (2 * S) : -1;
    if (kStageInLds) {
        for (int t = threadIdx.x; t < kFootW * kFootH; t += 256) {
            const int X = fx0 + t % kFootW, Y = fy0 + t / kFootW;
            const bool inside = X >= 0 && X < w && Y >= 0 && Y < h;
            const size_t q = inside ? static_cast<size_t>(Y) * w + X : 0;
            float4 ra = A[q];
            if (!inside) ra.w = 0.0f;          // a tap outside the low image is one without data
            lds[3 * t] = ra;
            lds[3 * t + 1] = B[q];
            lds[3 * t + 2] = Cc[q];
        }
        __syncthreads();
    }
    if (x >= a.width || y >= a.height) return;
    const size_t p = static_cast<size_t>(y) * a.width + x;
    const bool hit = a.hit_index[p] >= 0;
    const float4 bp = make_float4(a.normal[3 * p], a.normal[3 * p + 1], a.normal[3 * p + 2], hit ? 1.0f : 0.0f);
    const float4 cp = make_float4(a.position[3 * p], a.position[3 * p + 1], a.position[3 * p + 2], 0.0f);
    const float fx = static_cast<float>(2 * x + 1 - S) / static_cast<float>(2 * S);
    const float fy = static_cast<float>(2 * y + 1 - S) / static_cast<float>(2 * S);
    const float x0f = __builtin_floorf(fx), y0f = __builtin_floorf(fy);
    const float tx = fx - x0f, ty = fy - y0f;
    const int X0 = static_cast<int>(x0f), Y0 = static_cast<int>(y0f);
    float om[4];
    float4 cq[4];
    bool used[4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int t = 2 * j + i, X = X0 + i, Y = Y0 + j;
            used[t] = false;
            om[t] = 0.0f;
            cq[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (X < 0 || X >= w || Y < 0 || Y >= h) continue;
            float4 aq, bq, gq;
            if (kStageInLds) {
                const int l = 3 * ((Y - fy0) * kFootW + (X - fx0));
                aq = lds[l]; bq = lds[l + 1]; gq = lds[l + 2];
            } else {
                const size_t q = static_cast<size_t>(Y) * w + X;
                aq = A[q]; bq = B[q]; gq = Cc[q];
            }
            if (aq.w == 0.0f || bq.w != bp.w) continue;
            const float tent = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
            om[t] = hit ? feature_weight(tent, bp, cp, bq, gq, a.sigma_plane, a.normal_power_log2) : tent;
            cq[t] = aq;
            used[t] = true;
        }
    }
    bool any = false;
    float best = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (used[t] && (!any || om[t] > best)) {
            any = true;
            best = om[t];
            b0 = cq[t].x; b1 = cq[t].y; b2 = cq[t].z;
        }
    float wt = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (used[t]) {
            wt = wt + om[t];
            s0 = s0 + om[t] * (cq[t].x - b0);
            s1 = s1 + om[t] * (cq[t].y - b1);
            s2 = s2 + om[t] * (cq[t].z - b2);
        }
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
    int32_t n = 0;
    if (wt > kUpsampleMinWeight) {
        const bool dm = a.demodulate && hit;
        o0 = divisor(a.albedo[3 * p], dm) * (b0 + s0 / wt);
        o1 = divisor(a.albedo[3 * p + 1], dm) * (b1 + s1 / wt);
        o2 = divisor(a.albedo[3 * p + 2], dm) * (b2 + s2 / wt);
        o0 = o0 > 0.0f ? o0 : 0.0f;
        o1 = o1 > 0.0f ? o1 : 0.0f;
        o2 = o2 > 0.0f ? o2 : 0.0f;
        n = 1;
    } else {
        const size_t r = static_cast<size_t>(y / S) * w + x / S;   // the low pixel that contains p
        if (a.count_lo[r] > 0) {
            o0 = a.mean_lo[3 * r]; o1 = a.mean_lo[3 * r + 1]; o2 = a.mean_lo[3 * r + 2];
            n = 1;
        }
    }
    a.mean_rgb[3 * p] = o0; a.mean_rgb[3 * p + 1] = o1; a.mean_rgb[3 * p + 2] = o2;
    a.count_out[p] = n;
}

template <int S>
void launch_scale(const UpsampleArgs &a, int w, int h, hipStream_t stream) {
    const dim3 tiles((a.width + 31) / 32, (a.height + 7) / 8);
    hipLaunchKernelGGL(upsample_kernel<S>, tiles, dim3(256), 0, stream, a, w, h);
}

}  // namespace

hipError_t launch_upsample(const UpsampleArgs &a, hipStream_t stream) {
    if (a.scale < kUpsampleMinScale || a.scale > kUpsampleMaxScale || a.width % a.scale || a.height % a.scale) return hipErrorInvalidValue;
    const int w = a.width / a.scale, h = a.height / a.scale, n_lo = w * h;
    hipLaunchKernelGGL(upsample_prepare_kernel, dim3((n_lo + 255) / 256), dim3(256), 0, stream, a, w, n_lo);
    if (a.scale == 2) launch_scale<2>(a, w, h, stream);
    else if (a.scale == 3) launch_scale<3>(a, w, h, stream);
    else launch_scale<4>(a, w, h, stream);
    return hipGetLastError();
}

hipError_t launch_upsample_mean(const float *d_sum, const int32_t *d_count, int n_px, float *d_mean, hipStream_t stream) {
    hipLaunchKernelGGL(upsample_mean_kernel, dim3((n_px + 255) / 256), dim3(256), 0, stream, d_sum, d_count, n_px, d_mean);
    return hipGetLastError();
}

}  // namespace pt
