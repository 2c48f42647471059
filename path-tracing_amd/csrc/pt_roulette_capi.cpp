// Host side of Russian roulette (include/pt_hip.h: Russian roulette): the two parameters on a scene and on a frame, their getters, and
// the host's own evaluation of the step.  There is no table: the parameters live in the handle's SurfaceTables and travel in the kernel
// arguments.  A setter checks everything before it touches a handle, so a failed call leaves every handle as it was.
#include "pt_capi_internal.hpp"

#include <cmath>

#include "pt_host_math.hpp"

using ptc::fail;
using ptc::guarded;

namespace {

int refuse(const std::string &why) { return fail(PT_ERR_INVALID_ARGUMENT, "Russian roulette: " + why); }

// One handle or every device's copy of a frame's scene.
int set_impl(pt_scene *const *scenes, size_t n_scenes, int32_t start, float floor) {
    return ptc::set_on_copies(
        scenes, n_scenes,
        [&] {
            if (start == 0) return static_cast<int>(PT_OK);
            if (start < 0) return refuse("start is negative (0 clears, 1 is the first scattering step)");
            if (!std::isfinite(floor) || !pt::roulette_params_ok(start, floor)) return refuse("the floor must lie in [2^-10, 1]");
            for (size_t i = 0; i < n_scenes; ++i)
                if (!scenes[i]->surface.direct && !scenes[i]->surface.envdirect)
                    return refuse("the scene handle has neither direct lighting nor environment sampling on: roulette needs their per-path accounting");
            return static_cast<int>(PT_OK);
        },
        [](size_t) { return static_cast<int>(PT_OK); },
        [&](size_t i) {
            scenes[i]->surface.rr_start = start;
            scenes[i]->surface.rr_floor = start > 0 ? floor : 0.0f;
        });
}

int get_impl(const pt_scene *scene, int32_t *start, float *floor) {
    if (!scene || !start) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    *start = scene->surface.rr_start;
    if (floor) *floor = scene->surface.rr_floor;
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_scene_set_roulette(pt_scene *scene, int32_t start, float floor) {
    return guarded([&] { return set_impl(&scene, 1, start, floor); });
}

int pt_scene_get_roulette(const pt_scene *scene, int32_t *start, float *floor) {
    return guarded([&] { return get_impl(scene, start, floor); });
}

int pt_frame_set_roulette(pt_frame *frame, int32_t start, float floor) {
    return ptc::on_frame(frame, [&](pt_scene *const *sc, size_t n_sc) { return set_impl(sc, n_sc, start, floor); });
}

int pt_frame_get_roulette(pt_frame *frame, int32_t *start, float *floor) {
    return ptc::on_frame_root(frame, [&](const pt_scene *root) { return get_impl(root, start, floor); });
}

int pt_roulette_step(int32_t n, float floor, const float *throughput, const uint32_t *w0, float *out_throughput, int32_t *out_survives) {
    return guarded([&] {
        if (n < 0) return refuse("a negative count");
        if (!std::isfinite(floor) || !pt::roulette_params_ok(1, floor)) return refuse("the floor must lie in [2^-10, 1]");
        if (n > 0 && (!throughput || !w0 || !out_throughput || !out_survives)) return refuse("null argument");
        for (int32_t i = 0; i < n; ++i) {
            float tr = throughput[3 * i], tg = throughput[3 * i + 1], tb = throughput[3 * i + 2];
            const uint32_t word = w0[i];
            out_survives[i] = pt::roulette_step(floor, [word] { return ptc::host_unit_float(word); }, tr, tg, tb) ? 1 : 0;
            out_throughput[3 * i] = tr; out_throughput[3 * i + 1] = tg; out_throughput[3 * i + 2] = tb;
        }
        return static_cast<int>(PT_OK);
    });
}

}  // extern "C"
