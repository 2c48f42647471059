// The host side of Russian roulette (path-tracing_amd/csrc/pt_roulette_capi.cpp with the step of pt_roulette.hpp, the two switches it
// stands on -- pt_direct_capi.cpp, pt_envdirect_capi.cpp with pt_environment_capi.cpp --, the texture setter of pt_texture_capi.cpp and
// the loader of pt_scene.cpp) under AddressSanitizer + UBSan, as a program of its own (tests/test_roulette_host.py builds and runs it
// with the directory of its OBJ files as argument): on host-only handles (device -1: no HIP call is made) the setter and the getter,
// every refusal with a refused call leaving the handle as it was, the two switches' refusals while roulette is set, the frame's
// setter and getter, and pt_roulette_step at its edges.  The helpers the C API's main translation unit defines are defined here.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pt_capi_internal.hpp"

static std::string g_error;
int ptc::fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}
std::atomic<long> ptc::g_live_device_objects{0};
static std::vector<pt_scene *> g_frame_scenes;
const std::vector<pt_scene *> &ptc::frame_scenes(pt_frame *) { return g_frame_scenes; }   // (the "frame": two host-only copies)
int ptc::hip_fail(hipError_t, const char *what) { return ptc::fail(PT_ERR_HIP, what); }

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, g_error.c_str()); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : "./";
    pt_scene scene, copy;   // host-only: device -1
    std::string err;
    bool io = false;
    scene.shared = std::make_shared<pt_scene_host>();
    EXPECT(pt::load_obj(dir, "lamp_room.obj", scene.shared->host, err, io));
    pt::build_device_tables(scene.shared->host, scene.shared->tables);
    copy.shared = scene.shared;

    int32_t start = -1;
    float floor = -1.0f;
    const float nan = std::nanf(""), inf = std::numeric_limits<float>::infinity();

    // neither switch on: refused; clearing is no error
    EXPECT(pt_scene_set_roulette(&scene, 3, 0.0625f) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_get_roulette(&scene, &start, &floor) == PT_OK && start == 0 && floor == 0.0f);
    EXPECT(pt_scene_set_roulette(&scene, 0, nan) == PT_OK);
    EXPECT(pt_scene_set_direct_lighting(&scene, 1) == PT_OK);
    for (float f : {0.0f, 0.00048828125f, 1.5f, -0.5f, nan, inf}) EXPECT(pt_scene_set_roulette(&scene, 3, f) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_set_roulette(&scene, -1, 0.5f) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_get_roulette(&scene, &start, nullptr) == PT_OK && start == 0);
    EXPECT(pt_scene_set_roulette(&scene, 3, PT_ROULETTE_DEFAULT_FLOOR) == PT_OK);
    EXPECT(pt_scene_get_roulette(&scene, &start, &floor) == PT_OK && start == 3 && floor == 0.0625f);
    EXPECT(pt_scene_set_roulette(&scene, 2, 4.0f) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_get_roulette(&scene, &start, &floor) == PT_OK && start == 3 && floor == 0.0625f);

    // the last of the two switches stays while roulette is set
    int32_t on = -1;
    EXPECT(pt_scene_set_direct_lighting(&scene, 0) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_get_direct_lighting(&scene, &on) == PT_OK && on == 1);
    const std::vector<float> map(8 * 8 * 3, 0.5f);
    const pt_env_sampling dflt = {0.0f};
    EXPECT(pt_scene_set_environment_map(&scene, 8, map.data()) == PT_OK);
    EXPECT(pt_scene_set_environment_sampling(&scene, &dflt) == PT_OK);
    EXPECT(pt_scene_set_direct_lighting(&scene, 0) == PT_OK);
    EXPECT(pt_scene_set_environment_sampling(&scene, nullptr) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_get_environment_sampling(&scene, &on, nullptr) == PT_OK && on == 1);
    EXPECT(pt_scene_set_roulette(&scene, 0, 0.0f) == PT_OK);
    EXPECT(pt_scene_set_environment_sampling(&scene, nullptr) == PT_OK);
    EXPECT(pt_scene_set_roulette(&scene, 1, 1.0f) == PT_ERR_INVALID_ARGUMENT);

    // the frame's setter and getter: all copies or none
    g_frame_scenes = {&scene, &copy};
    pt_frame *frame = reinterpret_cast<pt_frame *>(&g_frame_scenes);   // (never dereferenced: frame_scenes above answers for it)
    EXPECT(pt_scene_set_direct_lighting(&scene, 1) == PT_OK);
    EXPECT(pt_frame_set_roulette(frame, 2, 0.25f) == PT_ERR_INVALID_ARGUMENT);   // (the copy has no switch)
    EXPECT(pt_scene_get_roulette(&scene, &start, nullptr) == PT_OK && start == 0);
    EXPECT(pt_frame_set_direct_lighting(frame, 1) == PT_OK);
    EXPECT(pt_frame_set_roulette(frame, 2, 0.25f) == PT_OK);
    EXPECT(pt_frame_get_roulette(frame, &start, &floor) == PT_OK && start == 2 && floor == 0.25f);
    EXPECT(pt_scene_get_roulette(&copy, &start, &floor) == PT_OK && start == 2 && floor == 0.25f);
    EXPECT(pt_frame_set_direct_lighting(frame, 0) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_frame_set_roulette(frame, 0, 0.0f) == PT_OK);
    EXPECT(pt_frame_set_direct_lighting(frame, 0) == PT_OK);
    EXPECT(pt_scene_set_roulette(nullptr, 1, 0.5f) == PT_ERR_INVALID_ARGUMENT && pt_scene_get_roulette(nullptr, nullptr, nullptr) == PT_ERR_INVALID_ARGUMENT);

    // the step at its edges
    const float t[] = {1.0f, 0.5f, 0.25f,   0.5f, -0.25f, 0.0f,   0.5f, 0.25f, 0.0f,   nan, 0.5f, 0.5f,   0.0f, 0.0f, 0.0f,   0.001f, 0.0f, 0.0f};
    const uint32_t w[] = {0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu};
    float out[18];
    int32_t alive[6];
    EXPECT(pt_roulette_step(6, 0.0625f, t, w, out, alive) == PT_OK);
    EXPECT(alive[0] == 1 && out[0] == 1.0f && out[1] == 0.5f);
    EXPECT(alive[1] == 1 && out[3] == 1.0f && out[4] == -0.5f);
    EXPECT(alive[2] == 0 && out[6] == 0.0f && out[7] == 0.0f);
    EXPECT(alive[3] == 1 && out[9] != out[9] && out[10] == 0.5f);
    EXPECT(alive[4] == 1 && out[12] == 0.0f);
    EXPECT(alive[5] == 0 && out[15] == 0.0f);
    EXPECT(pt_roulette_step(0, 1.0f, nullptr, nullptr, nullptr, nullptr) == PT_OK);
    EXPECT(pt_roulette_step(1, 1.0f, nullptr, w, out, alive) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_roulette_step(-1, 1.0f, t, w, out, alive) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_roulette_step(1, nan, t, w, out, alive) == PT_ERR_INVALID_ARGUMENT);

    if (failures) return 1;
    std::printf("roulette host ok\n");
    return 0;
}
