// The colour display kernel (include/pt_hip.h: pt_display_present_colour): pt_display_graded.hip's kernel with two steps more --
// before the exposure a 3 x 3 matrix on the pixel's mean (passed by value; skipped when it is the identity bit for bit), behind
// the curve a 3D LUT with tetrahedral interpolation (16-byte vertices in device memory, four plain loads per pixel: the LUT is
// 4.4 MB at most and stays in L2 / Infinity Cache, the kernel's stream is the 16 bytes per pixel it reads).  The statements are
// pt_display_body.inc, the arithmetic pt_grade.hpp and pt_colour.hpp; curve and "with a LUT" are compile-time constants.  A LUT
// index is clamped into the table whatever the value (NaN and negatives go to cell 0), so no load leaves the table.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_colour.hpp"
#include "pt_display.hpp"
#include "pt_display_kernel.hpp"
#include "pt_grade.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {

#define PT_DISPLAY_GRADED
#define PT_DISPLAY_COLOUR
template <bool DIVIDE, int CURVE, bool LUT>
__global__ __launch_bounds__(kDisplayBlock) void display_colour_kernel(DisplayArgs a, const float *exposure, ColourStep colour) {
#include "pt_display_body.inc"
}
#undef PT_DISPLAY_COLOUR
#undef PT_DISPLAY_GRADED

template <int CURVE, bool LUT>
void launch_divide(const DisplayArgs &a, const float *exposure, const ColourStep &c, dim3 grid, hipStream_t stream) {
    if (a.divide)
        hipLaunchKernelGGL((display_colour_kernel<true, CURVE, LUT>), grid, dim3(kDisplayBlock), 0, stream, a, exposure, c);
    else
        hipLaunchKernelGGL((display_colour_kernel<false, CURVE, LUT>), grid, dim3(kDisplayBlock), 0, stream, a, exposure, c);
}

template <int CURVE>
void launch_curve(const DisplayArgs &a, const float *exposure, const ColourStep &c, dim3 grid, hipStream_t stream) {
    if (c.lut_n) launch_divide<CURVE, true>(a, exposure, c, grid, stream);
    else launch_divide<CURVE, false>(a, exposure, c, grid, stream);
}

}  // namespace

hipError_t launch_display_colour(const DisplayArgs &a, int curve, const float *exposure, const ColourStep &c, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    if (c.lut_n && (c.lut_n < kLutMinSize || c.lut_n > kLutMaxSize || !c.lut)) return hipErrorInvalidValue;
    const int n_groups = (a.n + 3) / 4;
    const int blocks = (n_groups + kDisplayBlock - 1) / kDisplayBlock;
    const dim3 grid(blocks < kDisplayMaxBlocks ? blocks : kDisplayMaxBlocks);
    switch (curve) {
        case kCurveReference: launch_curve<kCurveReference>(a, exposure, c, grid, stream); break;
        case kCurveClamp: launch_curve<kCurveClamp>(a, exposure, c, grid, stream); break;
        case kCurveReinhard: launch_curve<kCurveReinhard>(a, exposure, c, grid, stream); break;
        case kCurveAces: launch_curve<kCurveAces>(a, exposure, c, grid, stream); break;
        default: return hipErrorInvalidValue;   // (the host layer has refused an unknown curve long before)
    }
    return hipGetLastError();
}

}  // namespace pt
