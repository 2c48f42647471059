// Scene-linear output on the device (include/pt_hip.h: pt_linear_*): the image the display kernel would read -- sums or means and their
// counts -- to the body of a PFM or of a flat Radiance picture.  The arithmetic is pt_linear.hpp's, the copy the host's definition
// (pt_linear_encode) uses; every pixel is finished here: there is no table, no deferred list and nothing the host redoes.
//
// Both kernels stream: what matters is the shape of their accesses, and both write nothing but whole 16-byte groups of the output,
// whose buffer is padded to them (pt::linear_room).
//
// RGBE.  A lane handles four consecutive pixels of the flat plane, as the display kernel does: 48 bytes of means (three 16-byte loads),
// 16 of counts, and its four pixels' dwords as one 16-byte store.  The last group of a plane whose pixel count is no multiple of four
// loads pixel by pixel with a bounds check and stores all the same.
//
// PFM.  The body is the plane of means with its rows in reverse order, so a lane is given four consecutive FLOATS OF THE OUTPUT -- a
// 16-byte group, aligned whatever the width is -- and finds where each comes from: one division gives the first one's row and column,
// the others follow along the row and wrap at its end into the next output row, which is the input row above.  Where a row is a whole
// number of groups (width % 4 == 0) a group never leaves its row and its source is 16-byte aligned too: one 16-byte load, and two
// counts, since four consecutive floats belong to two pixels.  Otherwise the four floats are loaded one by one (the lanes of a wave
// still read one contiguous stretch per row) with the count of each one's pixel.  Neither form has a loop whose length depends on the
// lane: the group that reaches beyond the plane's end is the same four steps with a bounds check.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_linear.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {

constexpr int kLinearBlock = 256;
constexpr int kLinearMaxBlocks = 2048;

// One channel of a pixel with samples: the mean (the display kernel's own division), then the exposure.
template <bool DIVIDE, bool EXPOSED>
__device__ __forceinline__ float linear_channel(float x, int32_t count, float e) {
    if (DIVIDE) x = x / static_cast<float>(count);   // (count == 0: never looked at)
    return linear_value(x, EXPOSED, e);
}

template <bool DIVIDE, bool EXPOSED>
__global__ __launch_bounds__(kLinearBlock) void linear_rgbe_kernel(LinearArgs a) {
    const float e = EXPOSED ? *a.exposure : 1.0f;
    const int n = a.width * a.height;
    const int n_groups = (n + 3) / 4;
    for (int g = blockIdx.x * kLinearBlock + threadIdx.x; g < n_groups; g += gridDim.x * kLinearBlock) {
        const int p0 = 4 * g;
        float m[12];
        int32_t c[4];
        if (p0 + 4 <= n) {
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
                const bool inside = p < n;
                c[j] = inside ? a.count[p] : 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) m[3 * j + k] = inside ? a.rgb[3 * static_cast<size_t>(p) + k] : 0.0f;
            }
        }
        uint32_t px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t word = linear_rgbe(linear_channel<DIVIDE, EXPOSED>(m[3 * j], c[j], e), linear_channel<DIVIDE, EXPOSED>(m[3 * j + 1], c[j], e),
                                              linear_channel<DIVIDE, EXPOSED>(m[3 * j + 2], c[j], e));
            px[j] = c[j] != 0 ? word : 0u;
        }
        *reinterpret_cast<uint4 *>(a.out + 4 * static_cast<size_t>(g)) = make_uint4(px[0], px[1], px[2], px[3]);
    }
}

// ROWS4: width % 4 == 0.
template <bool DIVIDE, bool EXPOSED, bool ROWS4>
__global__ __launch_bounds__(kLinearBlock) void linear_pfm_kernel(LinearArgs a) {
    const float e = EXPOSED ? *a.exposure : 1.0f;
    const int row = 3 * a.width;          // floats of a row
    const int total = row * a.height;     // floats of the plane (pt_hip.h's largest image: below 2^31)
    const int n_groups = (total + 3) / 4;
    for (int g = blockIdx.x * kLinearBlock + threadIdx.x; g < n_groups; g += gridDim.x * kLinearBlock) {
        const int o0 = 4 * g;             // the group's first float in the output
        int y_out = o0 / row, col = o0 - y_out * row;
        float x[4];
        int32_t c[4];
        if (ROWS4) {   // o0 + 4 <= total, the four floats lie in one row, and the row above starts on a 16-byte boundary as this one does
            const int i0 = (a.height - 1 - y_out) * row + col;
            const float4 v = *reinterpret_cast<const float4 *>(a.rgb + i0);
            const int pa = i0 / 3, first = 3 - (i0 - 3 * pa);   // floats i0 .. i0 + first - 1 are pixel pa's, the others pixel pa + 1's
            const int32_t ca = a.count[pa], cb = a.count[pa + 1];   // (i0 + 3 < total: pixel pa + 1 exists)
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = k < first ? ca : cb;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool inside = o0 + k < total;   // (beyond the end y_out may be the height: float 0 is read in its place, without a branch)
                const int i = inside ? (a.height - 1 - y_out) * row + col : 0;
                const int32_t ci = a.count[i / 3];
                x[k] = a.rgb[i];
                c[k] = inside ? ci : 0;
                if (++col == row) { col = 0; ++y_out; }
            }
        }
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // (computed for every float, then chosen: no branch round the division, and the load stays one)
            const uint32_t bits = __float_as_uint(linear_channel<DIVIDE, EXPOSED>(x[k], c[k], e));
            w[k] = c[k] != 0 ? bits : 0u;
        }
        *reinterpret_cast<uint4 *>(a.out + 4 * static_cast<size_t>(g)) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

template <bool DIVIDE, bool EXPOSED>
void launch(const LinearArgs &a, hipStream_t stream) {
    const int words = a.format == kLinearPfm ? 3 * a.width * a.height : a.width * a.height;   // dwords of the body
    const int n_groups = (words + 3) / 4;
    const int blocks = (n_groups + kLinearBlock - 1) / kLinearBlock;
    const dim3 grid(blocks < kLinearMaxBlocks ? blocks : kLinearMaxBlocks);
    if (a.format == kLinearRgbe)
        hipLaunchKernelGGL((linear_rgbe_kernel<DIVIDE, EXPOSED>), grid, dim3(kLinearBlock), 0, stream, a);
    else if (a.width % 4 == 0)
        hipLaunchKernelGGL((linear_pfm_kernel<DIVIDE, EXPOSED, true>), grid, dim3(kLinearBlock), 0, stream, a);
    else
        hipLaunchKernelGGL((linear_pfm_kernel<DIVIDE, EXPOSED, false>), grid, dim3(kLinearBlock), 0, stream, a);
}

}  // namespace

hipError_t launch_linear_encode(const LinearArgs &a, hipStream_t stream) {
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    if (a.format != kLinearPfm && a.format != kLinearRgbe) return hipErrorInvalidValue;
    if (a.divide)
        a.exposed ? launch<true, true>(a, stream) : launch<true, false>(a, stream);
    else
        a.exposed ? launch<false, true>(a, stream) : launch<false, false>(a, stream);
    return hipGetLastError();
}

}  // namespace pt
