// Bloom (include/pt_hip.h: pt_bloom_host, pt_display_present_bloom): the light above a threshold, spread over its neighbourhood by
// a (1 3 3 1)/8 pyramid down and a (1 3)/4 pyramid up, added to the linear mean the display kernel is about to read.  The header
// states every operation; this file keeps their order, and nothing is fused.
//
// A pyramid level is a plane of 16-byte records (r, g, b, 0), so a tap is one 16-byte load.  Level 0, the bright pass B of the
// image, is never stored: the first down kernel makes it from the means (or sums) and counts as it reads them.
//
// bloom_down_kernel: a 256-thread workgroup makes a 32 x 8 tile of level k from the 66 x 18 region of level k - 1 under it.  The
// horizontal pass is taken at the 32 decimated columns only, for the region's 18 rows, straight from global memory into an LDS
// tile of 32 x 18 records (9 KB); a lane's four taps are neighbours, and half of them are its neighbour lane's too, so they come
// from the cache.  The vertical pass reads four records of one column from LDS.  A wave covers two rows of 32 records; the
// records are written whole and read as their three floats, accesses that are served in groups of 8 lanes on consecutive
// records, 32 consecutive words: no two lanes of a group meet on a bank, so the rows need no padding.
//
// bloom_up_kernel: a workgroup makes a 32 x 8 tile of level k: the 6 coarse rows it touches are upsampled horizontally to its 32
// columns into LDS (3 KB), two taps each from global memory, then vertically from LDS, two taps each.  For k >= 1 the result is
// added to D_k in place (a lane reads and writes its own record only); for k = 0 it is the glare A, and the kernel writes
// m + A * weight as a plane of means for the display kernel.
//
// Every coordinate is clamped into its plane before it is used as an index, lanes outside the image included; only lanes inside
// write.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "pt_bloom.hpp"
#include "pt_grade.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {

constexpr int kBloomBlock = 256;
constexpr int kTileW = 32, kTileH = 8;             // a workgroup's tile of the level it writes
constexpr int kDownRows = 2 * kTileH + 2;          // rows of the level above under a down tile: 2 Y0 - 1 .. 2 Y0 + 16
constexpr int kUpRows = kTileH / 2 + 2;            // coarse rows under an up tile: y0 / 2 - 1 .. y0 / 2 + 4
static_assert(kTileW * kTileH == kBloomBlock, "one lane per record of the tile");

__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, 0.0f); }
__device__ __forceinline__ float4 mul4(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, 0.0f); }

// ((p0 + p1) * 0.375) + ((pm + p2) * 0.125)
__device__ __forceinline__ float4 down_taps(float4 pm, float4 p0, float4 p1, float4 p2) {
    return add4(mul4(add4(p0, p1), 0.375f), mul4(add4(pm, p2), 0.125f));
}
// (near * 0.75) + (far * 0.25)
__device__ __forceinline__ float4 up_taps(float4 near, float4 far) { return add4(mul4(near, 0.75f), mul4(far, 0.25f)); }

// The pixel's linear mean, as the display kernels divide.
template <bool DIVIDE>
__device__ __forceinline__ void pixel_mean(const float *rgb, size_t p, int32_t c, float &r, float &g, float &b) {
    r = rgb[3 * p]; g = rgb[3 * p + 1]; b = rgb[3 * p + 2];
    if (DIVIDE) {
        const float n = static_cast<float>(c);
        r = r / n; g = g / n; b = b / n;
    }
}

// B of pixel p: the part of the mean above the luminance t.
template <bool DIVIDE>
__device__ __forceinline__ float4 bright_pass(const float *rgb, const int32_t *count, size_t p, float t) {
    const int32_t c = count[p];
    if (c == 0) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float r, g, b;
    pixel_mean<DIVIDE>(rgb, p, c, r, g, b);
    const float l = meter_luminance(r, g, b);
    if (!(l > t) || !(l <= FLT_MAX)) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float s = (l - t) / l;
    return make_float4(r * s, g * s, b * s, 0.0f);
}

struct DownArgs {
    int in_w, in_h, out_w, out_h;
    uint32_t tiles_x;        // tiles in a row of the level written; a workgroup's tile is blockIdx.x, row by row
    const float4 *in;        // level k - 1 (k >= 2)
    const float *rgb;        // FIRST: the image, in_w x in_h
    const int32_t *count;
    const float *exposure;
    float threshold;
    float4 *out;             // level k
};

template <bool FIRST, bool DIVIDE>
__global__ __launch_bounds__(kBloomBlock) void bloom_down_kernel(DownArgs a) {
    __shared__ float4 G[kDownRows * kTileW];
    const int X0 = static_cast<int>(blockIdx.x % a.tiles_x) * kTileW, Y0 = static_cast<int>(blockIdx.x / a.tiles_x) * kTileH;
    float t = 0.0f;
    if (FIRST) t = a.threshold / *a.exposure;
    for (int i = threadIdx.x; i < kDownRows * kTileW; i += kBloomBlock) {
        const int row = i / kTileW, col = i % kTileW;
        const int y = clampi(2 * Y0 - 1 + row, a.in_h), x = 2 * (X0 + col);
        const size_t line = static_cast<size_t>(y) * a.in_w;
        float4 p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t at = line + clampi(x - 1 + j, a.in_w);
            p[j] = FIRST ? bright_pass<DIVIDE>(a.rgb, a.count, at, t) : a.in[at];
        }
        G[i] = down_taps(p[0], p[1], p[2], p[3]);
    }
    __syncthreads();
    const int tx = threadIdx.x % kTileW, ty = threadIdx.x / kTileW;
    const int X = X0 + tx, Y = Y0 + ty;
    const float4 *g = G + (2 * ty) * kTileW + tx;   // rows 2 Y - 1 .. 2 Y + 2 of the level above
    const float4 d = down_taps(g[0], g[kTileW], g[2 * kTileW], g[3 * kTileW]);
    if (X < a.out_w && Y < a.out_h) a.out[static_cast<size_t>(Y) * a.out_w + X] = d;
}

struct UpArgs {
    int w, h, coarse_w, coarse_h;
    uint32_t tiles_x;
    const float4 *coarse;    // U_{k+1}
    float4 *level;           // !LAST: D_k in, U_k out
    const float *rgb;        // LAST: the image, its counts, the weight and the output plane
    const int32_t *count;
    float weight;
    float *out_rgb;
};

template <bool LAST, bool DIVIDE>
__global__ __launch_bounds__(kBloomBlock) void bloom_up_kernel(UpArgs a) {
    __shared__ float4 G[kUpRows * kTileW];
    const int x0 = static_cast<int>(blockIdx.x % a.tiles_x) * kTileW, y0 = static_cast<int>(blockIdx.x / a.tiles_x) * kTileH;
    for (int i = threadIdx.x; i < kUpRows * kTileW; i += kBloomBlock) {
        const int row = i / kTileW, x = x0 + i % kTileW;
        const int Yc = clampi(y0 / 2 - 1 + row, a.coarse_h);
        const int X = x >> 1;
        const size_t line = static_cast<size_t>(Yc) * a.coarse_w;
        const float4 near = a.coarse[line + clampi(X, a.coarse_w)];
        const float4 far = a.coarse[line + clampi((x & 1) ? X + 1 : X - 1, a.coarse_w)];
        G[i] = up_taps(near, far);
    }
    __syncthreads();
    const int tx = threadIdx.x % kTileW, ty = threadIdx.x / kTileW;
    const int x = x0 + tx, y = y0 + ty;
    const int row = (ty >> 1) + 1;                  // of coarse row y >> 1 in G
    const float4 v = up_taps(G[row * kTileW + tx], G[((ty & 1) ? row + 1 : row - 1) * kTileW + tx]);
    if (x >= a.w || y >= a.h) return;
    const size_t p = static_cast<size_t>(y) * a.w + x;
    if (!LAST) {
        a.level[p] = add4(a.level[p], v);
        return;
    }
    const int32_t c = a.count[p];
    float r, g, b;
    if (c != 0) {
        pixel_mean<DIVIDE>(a.rgb, p, c, r, g, b);
        r = r + (v.x * a.weight); g = g + (v.y * a.weight); b = b + (v.z * a.weight);
    } else {   // (no samples: never looked at by the display kernel; the plane keeps the input's value)
        r = a.rgb[3 * p]; g = a.rgb[3 * p + 1]; b = a.rgb[3 * p + 2];
    }
    a.out_rgb[3 * p] = r; a.out_rgb[3 * p + 1] = g; a.out_rgb[3 * p + 2] = b;
}

// One grid dimension: a plane of the largest image has fewer than 2^24 tiles, whatever its shape.
uint32_t tiles_across(int w) { return static_cast<uint32_t>((w + kTileW - 1) / kTileW); }
dim3 tiles(int w, int h) { return dim3(tiles_across(w) * static_cast<uint32_t>((h + kTileH - 1) / kTileH)); }

}  // namespace

hipError_t launch_bloom(const BloomArgs &b, hipStream_t stream) {
    if (b.width <= 0 || b.height <= 0 || b.levels < 1 || b.levels > kBloomMaxLevels) return hipErrorInvalidValue;
    int w[kBloomMaxLevels + 1], h[kBloomMaxLevels + 1];
    float4 *level[kBloomMaxLevels + 1];
    w[0] = b.width; h[0] = b.height; level[0] = nullptr;
    float4 *next = static_cast<float4 *>(b.pyramid);
    for (int k = 1; k <= b.levels; ++k) {
        w[k] = bloom_half(w[k - 1]); h[k] = bloom_half(h[k - 1]);
        level[k] = next;
        next += static_cast<size_t>(w[k]) * h[k];
    }
    for (int k = 1; k <= b.levels; ++k) {
        DownArgs a;
        a.in_w = w[k - 1]; a.in_h = h[k - 1]; a.out_w = w[k]; a.out_h = h[k];
        a.in = level[k - 1]; a.rgb = b.rgb; a.count = b.count; a.exposure = b.exposure; a.threshold = b.threshold;
        a.out = level[k]; a.tiles_x = tiles_across(w[k]);
        const dim3 grid = tiles(w[k], h[k]);
        if (k > 1)
            hipLaunchKernelGGL((bloom_down_kernel<false, false>), grid, dim3(kBloomBlock), 0, stream, a);
        else if (b.divide)
            hipLaunchKernelGGL((bloom_down_kernel<true, true>), grid, dim3(kBloomBlock), 0, stream, a);
        else
            hipLaunchKernelGGL((bloom_down_kernel<true, false>), grid, dim3(kBloomBlock), 0, stream, a);
    }
    for (int k = b.levels - 1; k >= 0; --k) {
        UpArgs a;
        a.w = w[k]; a.h = h[k]; a.coarse_w = w[k + 1]; a.coarse_h = h[k + 1];
        a.coarse = level[k + 1]; a.level = level[k];
        a.rgb = b.rgb; a.count = b.count; a.weight = b.weight; a.out_rgb = b.out_rgb; a.tiles_x = tiles_across(w[k]);
        const dim3 grid = tiles(w[k], h[k]);
        if (k > 0)
            hipLaunchKernelGGL((bloom_up_kernel<false, false>), grid, dim3(kBloomBlock), 0, stream, a);
        else if (b.divide)
            hipLaunchKernelGGL((bloom_up_kernel<true, true>), grid, dim3(kBloomBlock), 0, stream, a);
        else
            hipLaunchKernelGGL((bloom_up_kernel<true, false>), grid, dim3(kBloomBlock), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace pt
