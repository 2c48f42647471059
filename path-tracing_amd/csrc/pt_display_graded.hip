// The graded display kernel (include/pt_hip.h: pt_display_present_graded): pt_display.hip's kernel with one step more -- every
// channel of a pixel becomes g = curve(m * e) before the table is searched, e read from a device scalar (a manual exposure is
// written there by the host layer, an automatic one by pt_meter.hip's exposure_kernel earlier on the same stream).  The statements
// are pt_display_body.inc, the arithmetic pt_grade.hpp; the curve is a compile-time constant, so a kernel holds one curve's code.
// The threshold table is the ungraded one: g goes through it as a mean would.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_display.hpp"
#include "pt_display_kernel.hpp"
#include "pt_grade.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {

#define PT_DISPLAY_GRADED
template <bool DIVIDE, int CURVE>
__global__ __launch_bounds__(kDisplayBlock) void display_kernel(DisplayArgs a, const float *exposure) {
#include "pt_display_body.inc"
}
#undef PT_DISPLAY_GRADED

template <int CURVE>
void launch_curve(const DisplayArgs &a, const float *exposure, dim3 grid, hipStream_t stream) {
    if (a.divide)
        hipLaunchKernelGGL((display_kernel<true, CURVE>), grid, dim3(kDisplayBlock), 0, stream, a, exposure);
    else
        hipLaunchKernelGGL((display_kernel<false, CURVE>), grid, dim3(kDisplayBlock), 0, stream, a, exposure);
}

}  // namespace

hipError_t launch_display_graded(const DisplayArgs &a, int curve, const float *exposure, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    const int n_groups = (a.n + 3) / 4;
    const int blocks = (n_groups + kDisplayBlock - 1) / kDisplayBlock;
    const dim3 grid(blocks < kDisplayMaxBlocks ? blocks : kDisplayMaxBlocks);
    switch (curve) {
        case kCurveReference: launch_curve<kCurveReference>(a, exposure, grid, stream); break;
        case kCurveClamp: launch_curve<kCurveClamp>(a, exposure, grid, stream); break;
        case kCurveReinhard: launch_curve<kCurveReinhard>(a, exposure, grid, stream); break;
        case kCurveAces: launch_curve<kCurveAces>(a, exposure, grid, stream); break;
        default: return hipErrorInvalidValue;   // (the host layer has refused an unknown curve long before)
    }
    return hipGetLastError();
}

}  // namespace pt
