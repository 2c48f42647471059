// Metering for the automatic exposure (include/pt_hip.h: pt_meter_host, pt_display_present_graded): a luminance histogram of the
// linear mean the display kernel is about to read, and the exposure it gives.
//
// meter_kernel reads as the display kernel does -- a lane takes four consecutive pixels of the flat plane, 48 bytes of means as
// three 16-byte loads and 16 of counts, the tail group pixel by pixel with a bounds check -- and counts with integer atomics
// only, so the histogram is exact and the same from run to run.  A workgroup keeps ONE COPY OF THE HISTOGRAM PER WAVE in LDS
// (4 x 129 words = 2 KB, no limit on the occupancy): waves never meet on an address, and an odd stride of 129 words puts the four
// copies of a bin into four banks for the flush.  Within a wave, lanes that hit one bin are serialised by the LDS atomic unit; the
// worst case, a flat image, is taken out beforehand: if every metered lane of the wave has the same bin, one lane adds the
// lane count.  After the loop 129 lanes add the non-zero sums of the four copies to the global histogram, one atomic each.
//
// exposure_kernel is one wave whose first lane runs pt_grade.hpp's exposure_from_histogram: 128 additions, one division.  It
// exists so that the chain meter -> exposure -> display needs no round trip to the host.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_meter.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {

constexpr int kMeterBlock = 256;
constexpr int kMeterWaves = kMeterBlock / 64;
constexpr int kMeterMaxBlocks = 2048;

// One pixel slot of the wave: `valid` lanes count their `bin` in the wave's copy `h`.
__device__ __forceinline__ void meter_count(uint32_t *h, bool valid, int bin) {
    const unsigned long long active = __ballot(valid);
    if (!active) return;
    const int leader = __ffsll(active) - 1;
    const int first = __shfl(bin, leader);
    if (__ballot(valid && bin == first) == active) {   // one bin for the whole wave (a flat region): one add
        if (static_cast<int>(__lane_id()) == leader) atomicAdd(&h[first], static_cast<uint32_t>(__popcll(active)));
    } else if (valid) {
        atomicAdd(&h[bin], 1u);
    }
}

template <bool DIVIDE>
__global__ __launch_bounds__(kMeterBlock) void meter_kernel(MeterArgs a) {
    __shared__ uint32_t H[kMeterWaves * kMeterEntries];
    for (int i = threadIdx.x; i < kMeterWaves * kMeterEntries; i += kMeterBlock) H[i] = 0u;
    __syncthreads();
    uint32_t *h = H + (threadIdx.x / 64) * kMeterEntries;
    const int n_groups = (a.n + 3) / 4;
    for (int g = blockIdx.x * kMeterBlock + threadIdx.x; g < n_groups; g += gridDim.x * kMeterBlock) {
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
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float r = m[3 * j], gr = m[3 * j + 1], b = m[3 * j + 2];
            if (DIVIDE) {
                const float n = static_cast<float>(c[j]);
                r = r / n; gr = gr / n; b = b / n;   // (count == 0: not metered)
            }
            meter_count(h, c[j] != 0, meter_bin(meter_luminance(r, gr, b)));
        }
    }
    __syncthreads();
    if (threadIdx.x < kMeterEntries) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < kMeterWaves; ++w) sum += H[w * kMeterEntries + threadIdx.x];
        if (sum) atomicAdd(&a.hist[threadIdx.x], sum);
    }
}

__global__ __launch_bounds__(64) void exposure_kernel(const uint32_t *hist, ExposureRule rule, int has_prev, float e_prev, ExposureOut *out) {
    if (threadIdx.x != 0) return;
    ExposureOut o;
    exposure_from_histogram(hist, rule, has_prev != 0, e_prev, &o.exposure, &o.target);
    uint32_t metered = 0;
    for (int b = 0; b < kMeterBins; ++b) metered += hist[b];
    o.metered = metered;
    o.dark = hist[kMeterDark];
    *out = o;
}

}  // namespace

hipError_t launch_meter(const MeterArgs &a, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    const int n_groups = (a.n + 3) / 4;
    const int blocks = (n_groups + kMeterBlock - 1) / kMeterBlock;
    const dim3 grid(blocks < kMeterMaxBlocks ? blocks : kMeterMaxBlocks);
    if (a.divide)
        hipLaunchKernelGGL(meter_kernel<true>, grid, dim3(kMeterBlock), 0, stream, a);
    else
        hipLaunchKernelGGL(meter_kernel<false>, grid, dim3(kMeterBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_exposure(const uint32_t *hist, const ExposureRule &rule, bool has_prev, float e_prev, ExposureOut *out, hipStream_t stream) {
    hipLaunchKernelGGL(exposure_kernel, dim3(1), dim3(64), 0, stream, hist, rule, has_prev ? 1 : 0, e_prev, out);
    return hipGetLastError();
}

}  // namespace pt
