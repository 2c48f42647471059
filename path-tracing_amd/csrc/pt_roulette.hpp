// Russian roulette (include/pt_hip.h: Russian roulette), the one copy of its arithmetic: the step that ends a path with a probability
// that follows its throughput and divides the survivors by that probability.  The roulette kernels (pt_kernels.hip:
// integrate_kernel_roulette) run it at the end of every scattering step from depth + 1 >= start on, and pt_roulette_step on the host.
// All float, every operation rounded once in the order written, nothing fused; the quotients are the correctly rounded ones (the
// build's flags on the device).
#pragma once
#include <cstdint>

#include "pt_grade.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pt {

// The fourth Philox counter word of the roulette's word.  Every other call of the integrator's paths has 0 there, the direct term's 3
// (pt_direct.hpp), environment sampling's 4 (pt_envdirect.hpp); the display's dither and grain, which run under the same key, have 1
// and 2 (pt_grain.hpp).
constexpr uint32_t kRouletteStream = 5u;

// What a handle may be given: start >= 1, floor in [2^-10, 1].  The default floor is a choice.
constexpr float kRouletteMinFloor = 0.0009765625f, kRouletteDefaultFloor = 0.0625f;
PT_GRADE_FN bool roulette_params_ok(int32_t start, float floor) { return start >= 1 && floor >= kRouletteMinFloor && floor <= 1.0f; }

// The step on throughput T after the lobe's factor.  `unit` is called at most once, and only where its value decides: it returns
// unit_float(w0) of philox(pixel, pass, depth, kRouletteStream), depth as before the increment.
//   m = max(|tr|, |tg|, |tb|), a NaN propagating; !(m < 1): the path survives unchanged.  Else p = m < floor ? floor : m, and the path
//   survives with T / p (three divisions) if unit < p and ends with T = 0 otherwise.
// Returns whether the path survives.
template <class Unit>
PT_GRADE_FN bool roulette_step(float floor, Unit unit, float &tr, float &tg, float &tb) {
    const float ar = __builtin_fabsf(tr), ag = __builtin_fabsf(tg), ab = __builtin_fabsf(tb);
    if (!(ar < 1.0f && ag < 1.0f && ab < 1.0f)) return true;   // !(m < 1), m the NaN-propagating maximum
    float m = ar;
    if (ag > m) m = ag;
    if (ab > m) m = ab;
    const float p = m < floor ? floor : m;
    if (unit() < p) {
        tr = tr / p; tg = tg / p; tb = tb / p;
        return true;
    }
    tr = tg = tb = 0.0f;
    return false;
}

}  // namespace pt
