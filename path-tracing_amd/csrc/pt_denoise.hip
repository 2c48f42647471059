// First-hit feature buffers and the feature-guided denoiser (include/pt_hip.h: pt_render_features_host, pt_denoise_host).
// The header states the arithmetic; everything here is one correctly rounded float operation per step in that order, nothing
// fused (the Makefile builds with -ffp-contract=off and IEEE divide / sqrt), so tests/denoise_restatement.py reproduces the
// results bit for bit in numpy.
//
// The denoiser is an edge-avoiding a-trous wavelet filter.  What a tap reads is packed into three 16-byte records per pixel:
//   A  colour.xyz (the demodulated mean) + variance of its luminance (< 0: the pixel holds no data)     ping-pong, two planes
//   B  normal.xyz + hit flag (1 = a triangle, 0 = a miss)                                               read-only
//   C  position.xyz + 0                                                                                 read-only
// so a tap is three 16-byte loads.  A workgroup is 32 x 8 pixels: a wave covers two row segments of 32 pixels, 512 contiguous
// bytes per record and row.  All levels read global memory: from spacing 4 on the taps of a workgroup share nothing, and the
// footprint of levels 0 and 1 lives in the L2.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_denoise.hpp"
#include "pt_feature_weight.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {

__device__ __forceinline__ float luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__global__ __launch_bounds__(256) void feature_rays_kernel(FeatureCamera cam, int width, int height, int row_begin, int n,
                                                           float *__restrict__ origins, float *__restrict__ directions) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int y = row_begin + p / width, x = p % width;
    const float u = static_cast<float>(static_cast<double>(x) / width - 0.5);
    const float v = static_cast<float>(-static_cast<double>(y) / height + 0.5);
    const float *c = cam.v;
    float dx = (u * c[3] + v * c[6]) + c[9];
    float dy = (u * c[4] + v * c[7]) + c[10];
    float dz = (u * c[5] + v * c[8]) + c[11];
    const float inv = 1.0f / __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
    const size_t o = 3 * static_cast<size_t>(p);
    origins[o] = c[0]; origins[o + 1] = c[1]; origins[o + 2] = c[2];
    directions[o] = dx * inv; directions[o + 1] = dy * inv; directions[o + 2] = dz * inv;
}

__global__ __launch_bounds__(256) void feature_gather_kernel(const ExactRec *__restrict__ exact, const MatRec *__restrict__ mats,
                                                             const float *__restrict__ origins, const float *__restrict__ directions,
                                                             const int32_t *__restrict__ hit_index, const float *__restrict__ hit_t, int n,
                                                             float *__restrict__ position, float *__restrict__ normal,
                                                             float *__restrict__ albedo) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const size_t o = 3 * static_cast<size_t>(p);
    const int32_t i = hit_index[p];
    float P[3] = {0.0f, 0.0f, 0.0f}, N[3] = {0.0f, 0.0f, 0.0f}, A[3] = {0.0f, 0.0f, 0.0f};
    if (i >= 0) {
        const float t = hit_t[p];
        const ExactRec &e = exact[i];
        const MatRec &m = mats[e.material];
        for (int k = 0; k < 3; ++k) {
            P[k] = origins[o + k] + directions[o + k] * t;
            N[k] = e.plane[k];
            A[k] = m.kd[k];
        }
    }
    for (int k = 0; k < 3; ++k) {
        position[o + k] = P[k];
        normal[o + k] = N[k];
        albedo[o + k] = A[k];
    }
}

struct PixelIn {
    float mean[3], a[3], c0[3], var;
    bool sampled;
};

// mean = sum / n, the demodulation divisor a, c0 = mean / a and the variance of the mean on luminance (prepare and finish)
__device__ __forceinline__ PixelIn pixel_in(const float *__restrict__ sum, const float *__restrict__ sum2, const int32_t *__restrict__ count,
                                            const float *__restrict__ albedo, const int32_t *__restrict__ hit_index, size_t p,
                                            int demodulate, bool want_var) {
    PixelIn r;
    const int32_t cnt = count[p];
    r.sampled = cnt > 0;
    const bool hit = hit_index[p] >= 0;
    const float n = static_cast<float>(r.sampled ? cnt : 1);
    float v3[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 3; ++k) {
        const float s = sum[3 * p + k];
        r.mean[k] = r.sampled ? s / n : s;
        const float al = albedo[3 * p + k];
        r.a[k] = (demodulate && hit) ? (al > kDenoiseAlbedoFloor ? al : kDenoiseAlbedoFloor) : 1.0f;
        r.c0[k] = r.sampled ? r.mean[k] / r.a[k] : 0.0f;
        if (want_var) {
            const float d = sum2[3 * p + k] / n - r.mean[k] * r.mean[k];
            v3[k] = ((d > 0.0f ? d : 0.0f) / n) / (r.a[k] * r.a[k]);
        }
    }
    r.var = r.sampled ? luma(v3[0], v3[1], v3[2]) : -1.0f;
    return r;
}

__global__ __launch_bounds__(256) void denoise_prepare_kernel(DenoiseArgs a, int n_px) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_px) return;
    const size_t p = static_cast<size_t>(i);
    const PixelIn px = pixel_in(a.sum, a.sum2, a.count, a.albedo, a.hit_index, p, a.demodulate, true);
    static_cast<float4 *>(a.rec_a0)[p] = make_float4(px.c0[0], px.c0[1], px.c0[2], px.var);
    static_cast<float4 *>(a.rec_b)[p] =
        make_float4(a.normal[3 * p], a.normal[3 * p + 1], a.normal[3 * p + 2], a.hit_index[p] >= 0 ? 1.0f : 0.0f);
    static_cast<float4 *>(a.rec_c)[p] = make_float4(a.position[3 * p], a.position[3 * p + 1], a.position[3 * p + 2], 0.0f);
}

// The variance a pixel with samples enters the filter with: the 3 x 3 binomial mean of the sample variance, and for pixels with
// fewer than kDenoiseSpatialBelow samples at least the feature-weighted spatial variance of the luminance in its 7 x 7 window.
__global__ __launch_bounds__(256) void denoise_variance_kernel(DenoiseArgs a) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= a.width || y >= a.height) return;
    const float4 *A = static_cast<const float4 *>(a.rec_a0), *B = static_cast<const float4 *>(a.rec_b), *Cc = static_cast<const float4 *>(a.rec_c);
    const size_t p = static_cast<size_t>(y) * a.width + x;
    const float4 ap = A[p];
    float4 out = ap;
    if (ap.w >= 0.0f) {
        const float4 bp = B[p], cp = Cc[p];
        float g_acc = 0.0f, g_w = 0.0f, m_w = 0.0f, m1 = 0.0f, m2 = 0.0f;
        for (int dy = -3; dy <= 3; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= a.height) continue;
            for (int dx = -3; dx <= 3; ++dx) {
                const int xx = x + dx;
                if (xx < 0 || xx >= a.width) continue;
                const size_t q = static_cast<size_t>(yy) * a.width + xx;
                const float4 aq = A[q], bq = B[q];
                if (!(aq.w >= 0.0f) || bq.w != bp.w) continue;
                if (dy >= -1 && dy <= 1 && dx >= -1 && dx <= 1) {
                    const float w = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
                    g_acc = g_acc + w * aq.w;
                    g_w = g_w + w;
                }
                float w = 1.0f;
                if (bp.w != 0.0f) w = feature_weight(1.0f, bp, cp, bq, Cc[q], a.sigma_plane, a.normal_power_log2);
                const float lq = luma(aq.x, aq.y, aq.z);
                m_w = m_w + w;
                m1 = m1 + w * lq;
                m2 = m2 + w * (lq * lq);
            }
        }
        const float mu = m1 / m_w;
        float sp = m2 / m_w - mu * mu;
        sp = sp > 0.0f ? sp : 0.0f;
        const float g = g_acc / g_w;
        out.w = a.count[p] >= kDenoiseSpatialBelow ? g : (g > sp ? g : sp);
    }
    static_cast<float4 *>(a.rec_a1)[p] = out;
}

// One level: the 5 x 5 B3-spline kernel with tap spacing `step`, rows outer, columns inner, the centre first.
__global__ __launch_bounds__(256) void denoise_atrous_kernel(const float4 *__restrict__ A, const float4 *__restrict__ B,
                                                             const float4 *__restrict__ Cc, float4 *__restrict__ out, int width, int height,
                                                             int step, float sigma_luminance, float sigma_plane, int k) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= width || y >= height) return;
    const size_t p = static_cast<size_t>(y) * width + x;
    const float4 ap = A[p], bp = B[p], cp = Cc[p];
    const bool have = ap.w >= 0.0f, hit = bp.w != 0.0f;
    const float lp = luma(ap.x, ap.y, ap.z);
    const float den = sigma_luminance * __builtin_sqrtf(have ? ap.w : 0.0f) + kDenoiseTiny;
    const float wc = 0.375f * 0.375f;
    float sw = have ? wc : 0.0f, sv = have ? (wc * wc) * ap.w : 0.0f;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    const float spline[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + dy * step;
        if (yy < 0 || yy >= height) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const int xx = x + dx * step;
            if (xx < 0 || xx >= width) continue;
            const size_t q = static_cast<size_t>(yy) * width + xx;
            const float4 aq = A[q], bq = B[q];
            if (!(aq.w >= 0.0f) || bq.w != bp.w) continue;
            float w = spline[dy + 2] * spline[dx + 2];
            if (hit) w = feature_weight(w, bp, cp, bq, Cc[q], sigma_plane, k);
            if (have) {
                const float t = (lp - luma(aq.x, aq.y, aq.z)) / den;
                w = w * (1.0f / (1.0f + t * t));
            }
            sw = sw + w;
            s0 = s0 + w * (aq.x - ap.x);
            s1 = s1 + w * (aq.y - ap.y);
            s2 = s2 + w * (aq.z - ap.z);
            sv = sv + (w * w) * aq.w;
        }
    }
    float4 r = ap;
    if (sw > kDenoiseFillMinWeight) {
        r.x = ap.x + s0 / sw;
        r.y = ap.y + s1 / sw;
        r.z = ap.z + s2 / sw;
        r.w = sv / (sw * sw);
    }
    out[p] = r;
}

__global__ __launch_bounds__(256) void denoise_finish_kernel(DenoiseArgs a, const float4 *__restrict__ A, int n_px) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_px) return;
    const size_t p = static_cast<size_t>(i);
    const PixelIn px = pixel_in(a.sum, a.sum2, a.count, a.albedo, a.hit_index, p, a.demodulate, false);
    const float4 ap = A[p];
    const float col[3] = {ap.x, ap.y, ap.z};
    const bool filled = ap.w >= 0.0f;
    for (int k = 0; k < 3; ++k) {
        float o = px.mean[k];
        if (filled) {
            o = px.sampled ? px.mean[k] + px.a[k] * (col[k] - px.c0[k]) : px.a[k] * col[k];
            o = o > 0.0f ? o : 0.0f;
        }
        a.mean_rgb[3 * p + k] = o;
    }
    a.count_out[p] = px.sampled ? a.count[p] : (filled ? 1 : 0);
}

}  // namespace

hipError_t launch_feature_rays(const FeatureCamera &cam, int width, int height, int row_begin, int rows, float *d_origins,
                               float *d_directions, hipStream_t stream) {
    const int n = rows * width;
    hipLaunchKernelGGL(feature_rays_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, cam, width, height, row_begin, n, d_origins, d_directions);
    return hipGetLastError();
}

hipError_t launch_feature_gather(const ExactRec *d_exact, const MatRec *d_mats, const float *d_origins, const float *d_directions,
                                 const int32_t *d_hit_index, const float *d_hit_t, int n, float *d_position, float *d_normal,
                                 float *d_albedo, hipStream_t stream) {
    hipLaunchKernelGGL(feature_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_exact, d_mats, d_origins, d_directions,
                       d_hit_index, d_hit_t, n, d_position, d_normal, d_albedo);
    return hipGetLastError();
}

hipError_t launch_denoise(const DenoiseArgs &a, hipStream_t stream) {
    const int n_px = a.width * a.height;
    const dim3 flat((n_px + 255) / 256), tiles((a.width + 31) / 32, (a.height + 7) / 8);
    hipLaunchKernelGGL(denoise_prepare_kernel, flat, dim3(256), 0, stream, a, n_px);
    hipLaunchKernelGGL(denoise_variance_kernel, tiles, dim3(256), 0, stream, a);
    float4 *cur = static_cast<float4 *>(a.rec_a1), *other = static_cast<float4 *>(a.rec_a0);
    for (int level = 0; level < a.levels; ++level) {
        hipLaunchKernelGGL(denoise_atrous_kernel, tiles, dim3(256), 0, stream, cur, static_cast<const float4 *>(a.rec_b),
                           static_cast<const float4 *>(a.rec_c), other, a.width, a.height, 1 << level, a.sigma_luminance, a.sigma_plane,
                           a.normal_power_log2);
        float4 *t = cur; cur = other; other = t;
    }
    hipLaunchKernelGGL(denoise_finish_kernel, flat, dim3(256), 0, stream, a, cur, n_px);
    return hipGetLastError();
}

}  // namespace pt
