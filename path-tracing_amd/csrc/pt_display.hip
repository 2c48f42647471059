// Linear means to image bytes on the device (include/pt_hip.h: pt_display_*).  The host writes, per channel of a pixel with
// samples, b = (uint8_t)(int)(std::pow(m, gamma) * 255.0f).  std::pow is not an operation the device reproduces bit for bit,
// and it does not have to: for gamma > 0 the integer L(m) = (int)(std::pow(m, gamma) * 255.0f) is a non-decreasing step
// function of m >= 0, so L(m) is the number of thresholds T_k <= m, T_k being the smallest float with L >= k -- and the host
// tabulates the T_k from its own std::pow (pt_display_capi.cpp).  The device only compares: a 12-step binary search in a copy
// of the table in LDS, then & 255 (levels above 255 wrap as the host's conversion to unsigned char does).
//
// What the table does not cover is left to the host: a channel that is negative or NaN, one at or above the last threshold,
// one inside a doubt band (a range around a threshold where the host's pow was found not to be monotone).  Such a pixel is
// appended to a list with its three means -- one atomic per wave and pixel slot -- and its bytes are written as 0; the host
// finishes it with the same function it would have used anyway.  So the bytes are the host chain's for every input.
//
// A lane handles four consecutive pixels of the flat plane: 48 bytes of means (three 16-byte loads), 16 of counts, and 12
// bytes of output as three dwords -- no byte stores.  The last group of a plane whose pixel count is no multiple of four
// loads pixel by pixel with a bounds check; the output buffer is padded to whole groups, so it stores its dwords all the same.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_display.hpp"

#pragma clang fp contract(off)

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

template <bool DIVIDE>
__global__ __launch_bounds__(kDisplayBlock) void display_kernel(DisplayArgs a) {
    __shared__ __attribute__((aligned(16))) float T[kDisplayTableSize];
    for (int i = threadIdx.x; i < kDisplayTableSize / 4; i += kDisplayBlock)
        reinterpret_cast<float4 *>(T)[i] = reinterpret_cast<const float4 *>(a.table)[i];
    __syncthreads();
    const int n_groups = (a.n + 3) / 4;
    for (int g = blockIdx.x * kDisplayBlock + threadIdx.x; g < n_groups; g += gridDim.x * kDisplayBlock) {
        const int p0 = 4 * g;
        float m[12];
        int32_t c[4];
        if (p0 + 4 <= a.n) {
            const float4 *src = reinterpret_cast<const float4 *>(a.rgb + 3 * static_cast<size_t>(p0));
            const float4 v0 = src[0], v1 = src[1], v2 = src[2];
            const int4 cc = *reinterpret_cast<const int4 *>(a.count + p0);
            m[0] = v0.x; m[1] = v0.y; m[2] = v0.z; m[3] = v0.w; m[4] = v1.x; m[5] = v1.y; m[6] = v1.z; m[7] = v1.w;
            m[8] = v2.x; m[9] = v2.y; m[10] = v2.z; m[11] = v2.w;
            c[0] = cc.x; c[1] = cc.y; c[2] = cc.z; c[3] = cc.w;
        } else {   // the tail of the plane: one to three pixels
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int p = p0 + j;
                const bool inside = p < a.n;
                c[j] = inside ? a.count[p] : 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) m[3 * j + k] = inside ? a.rgb[3 * static_cast<size_t>(p) + k] : 0.0f;
            }
        }
        if (DIVIDE) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float n = static_cast<float>(c[j]);
#pragma unroll
                for (int k = 0; k < 3; ++k) m[3 * j + k] = m[3 * j + k] / n;   // (count == 0: never looked at)
            }
        }
        bool out_of_table[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) out_of_table[i] = !(m[i] >= 0.0f) || m[i] >= a.last;
        for (int b = 0; b < a.n_bands; ++b) {
            const float lo = a.band_lo[b], hi = a.band_hi[b];
#pragma unroll
            for (int i = 0; i < 12; ++i) out_of_table[i] |= m[i] >= lo && m[i] < hi;
        }
        bool defer[4];
        uint32_t px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool samples = c[j] != 0;
            defer[j] = samples && (out_of_table[3 * j] || out_of_table[3 * j + 1] || out_of_table[3 * j + 2]);
            const uint32_t r = display_level(T, m[3 * j]) & 255u, gr = display_level(T, m[3 * j + 1]) & 255u,
                           bl = display_level(T, m[3 * j + 2]) & 255u;
            px[j] = samples && !defer[j] ? (bl | (gr << 8) | (r << 16)) : 0u;
        }
        // B G R B | G R B G | R B G R
        uint3 w;
        w.x = px[0] | (px[1] << 24);
        w.y = (px[1] >> 8) | (px[2] << 16);
        w.z = (px[2] >> 16) | (px[3] << 8);
        *reinterpret_cast<uint3 *>(a.bgr + 3 * static_cast<size_t>(g)) = w;

        if (__ballot(defer[0] || defer[1] || defer[2] || defer[3])) {   // rare: the whole wave skips it otherwise
            const uint32_t lane = __lane_id();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned long long mask = __ballot(defer[j]);
                if (!mask) continue;
                const int leader = __ffsll(mask) - 1;
                uint32_t base = 0;
                if (static_cast<int>(lane) == leader) base = atomicAdd(a.n_deferred, static_cast<uint32_t>(__popcll(mask)));
                base = __shfl(base, leader);
                if (defer[j]) {   // every pixel is appended at most once, so the list never outgrows its n entries
                    const uint32_t at = base + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
                    reinterpret_cast<float4 *>(a.deferred)[at] = make_float4(__int_as_float(p0 + j), m[3 * j], m[3 * j + 1], m[3 * j + 2]);
                }
            }
        }
    }
}

}  // namespace

hipError_t launch_display(const DisplayArgs &a, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    const int n_groups = (a.n + 3) / 4;
    const int blocks = (n_groups + kDisplayBlock - 1) / kDisplayBlock;
    const dim3 grid(blocks < kDisplayMaxBlocks ? blocks : kDisplayMaxBlocks);
    if (a.divide)
        hipLaunchKernelGGL(display_kernel<true>, grid, dim3(kDisplayBlock), 0, stream, a);
    else
        hipLaunchKernelGGL(display_kernel<false>, grid, dim3(kDisplayBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pt
