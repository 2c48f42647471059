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
//
// The kernel's statements are pt_display_body.inc and its helpers pt_display_kernel.hpp: the graded kernel of
// pt_display_graded.hip (display grading: exposure and a tone curve applied to the mean before the table is searched) is made of
// the same text with one step more.  This file's kernel is the ungraded one, and it is compiled from the tokens it always had:
// the include below is plain text between its braces, and the compiler's report for this file (make asm) equals the one from
// before the statements moved, line for line.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_display.hpp"
#include "pt_display_kernel.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {






template <bool DIVIDE>
__global__ __launch_bounds__(kDisplayBlock) void display_kernel(DisplayArgs a) {
#include "pt_display_body.inc"
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
