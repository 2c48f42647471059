// The grain display kernel (include/pt_hip.h: pt_display_present_grain): pt_display_colour.hip's kernel with two steps more -- behind
// the LUT the pixel's film grain on g (one lattice word of Philox per pixel at pitch 1, four otherwise), and in the table search a
// triangular dither of the level between the two thresholds round g, out of the LDS table the kernel holds anyway (one more Philox
// call per pixel).  The statements are pt_display_body.inc, the arithmetic pt_grade.hpp, pt_colour.hpp and pt_grain.hpp; curve,
// "with a LUT" and "pitch other than 1" are compile-time constants.  The kernel reads and writes what the colour kernel does: the
// stage costs arithmetic, no memory traffic.  A table index is a level below kDisplayTableSize whatever the value, so no LDS read
// leaves the table.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_colour.hpp"
#include "pt_display.hpp"
#include "pt_display_kernel.hpp"
#include "pt_grade.hpp"
#include "pt_grain.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {

#define PT_DISPLAY_GRADED
#define PT_DISPLAY_COLOUR
#define PT_DISPLAY_GRAIN
template <bool DIVIDE, int CURVE, bool LUT, bool SIZED>
__global__ __launch_bounds__(kDisplayBlock) void display_grain_kernel(DisplayArgs a, const float *exposure, ColourStep colour, GrainStep grain) {
#include "pt_display_body.inc"
}
#undef PT_DISPLAY_GRAIN
#undef PT_DISPLAY_COLOUR
#undef PT_DISPLAY_GRADED

template <int CURVE, bool LUT, bool SIZED>
void launch_divide(const DisplayArgs &a, const float *exposure, const ColourStep &c, const GrainStep &g, dim3 grid, hipStream_t stream) {
    if (a.divide)
        hipLaunchKernelGGL((display_grain_kernel<true, CURVE, LUT, SIZED>), grid, dim3(kDisplayBlock), 0, stream, a, exposure, c, g);
    else
        hipLaunchKernelGGL((display_grain_kernel<false, CURVE, LUT, SIZED>), grid, dim3(kDisplayBlock), 0, stream, a, exposure, c, g);
}

template <int CURVE>
void launch_curve(const DisplayArgs &a, const float *exposure, const ColourStep &c, const GrainStep &g, dim3 grid, hipStream_t stream) {
    const bool sized = g.size != 1.0f;
    if (c.lut_n) {
        if (sized) launch_divide<CURVE, true, true>(a, exposure, c, g, grid, stream);
        else launch_divide<CURVE, true, false>(a, exposure, c, g, grid, stream);
    } else {
        if (sized) launch_divide<CURVE, false, true>(a, exposure, c, g, grid, stream);
        else launch_divide<CURVE, false, false>(a, exposure, c, g, grid, stream);
    }
}

}  // namespace

hipError_t launch_display_grain(const DisplayArgs &a, int curve, const float *exposure, const ColourStep &c, const GrainStep &g, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    if (c.lut_n && (c.lut_n < kLutMinSize || c.lut_n > kLutMaxSize || !c.lut)) return hipErrorInvalidValue;
    if (g.width <= 0 || !(g.size >= 1.0f && g.size <= kGrainMaxSize)) return hipErrorInvalidValue;   // (the host layer fills both in)
    const int n_groups = (a.n + 3) / 4;
    const int blocks = (n_groups + kDisplayBlock - 1) / kDisplayBlock;
    const dim3 grid(blocks < kDisplayMaxBlocks ? blocks : kDisplayMaxBlocks);
    switch (curve) {
        case kCurveReference: launch_curve<kCurveReference>(a, exposure, c, g, grid, stream); break;
        case kCurveClamp: launch_curve<kCurveClamp>(a, exposure, c, g, grid, stream); break;
        case kCurveReinhard: launch_curve<kCurveReinhard>(a, exposure, c, g, grid, stream); break;
        case kCurveAces: launch_curve<kCurveAces>(a, exposure, c, g, grid, stream); break;
        default: return hipErrorInvalidValue;   // (the host layer has refused an unknown curve long before)
    }
    return hipGetLastError();
}

}  // namespace pt
