// The dielectric setters and getters (path-tracing_amd/csrc/pt_glass_capi.cpp) under AddressSanitizer + UBSan, as a program of its
// own (tests/test_glass_host.py builds and runs it): on a host-only handle (device -1: no HIP call is made) whose material table is
// filled in here -- five materials, number 0 emissive -- every refusal, a refused call leaving the list as it was, clear and get.  It
// links pt_glass_capi.cpp alone; the helpers that file takes from the C API's main translation unit are defined here.
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

static bool same(const pt_dielectric &a, const pt_dielectric &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main() {
    pt_scene scene, copy;   // host-only: device -1
    scene.shared = std::make_shared<pt_scene_host>();
    for (int m = 0; m < 5; ++m) {
        pt::MatRec r{};
        r.n_lobes = 2;
        r.kind0 = m == 0 ? 0 : 1;   // material 0: emissive + diffuse, the others glossy + diffuse
        r.kind1 = 2;
        scene.shared->tables.mats.push_back(r);
    }
    copy.shared = scene.shared;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    int32_t n = -1;
    EXPECT(pt_scene_get_dielectrics(&scene, nullptr, &n) == PT_OK && n == 0);
    const pt_dielectric first[2] = {{4, 1.5f, {0.9f, 1.0f, 0.9f}}, {2, 0.5f, {0.0f, 0.0f, 0.0f}}};
    EXPECT(pt_scene_set_dielectrics(&scene, first, 2) == PT_OK);
    const pt_dielectric bad[][2] = {
        {{5, 1.5f, {1, 1, 1}}, {1, 1.5f, {1, 1, 1}}},      {{-1, 1.5f, {1, 1, 1}}, {1, 1.5f, {1, 1, 1}}},   {{3, 1.5f, {1, 1, 1}}, {3, 1.3f, {1, 1, 1}}},
        {{3, 0.12f, {1, 1, 1}}, {1, 1.5f, {1, 1, 1}}},     {{3, 8.5f, {1, 1, 1}}, {1, 1.5f, {1, 1, 1}}},    {{3, nan, {1, 1, 1}}, {1, 1.5f, {1, 1, 1}}},
        {{3, inf, {1, 1, 1}}, {1, 1.5f, {1, 1, 1}}},       {{3, 1.5f, {1, -0.1f, 1}}, {1, 1.5f, {1, 1, 1}}}, {{3, 1.5f, {1, 1, 1.1f}}, {1, 1.5f, {1, 1, 1}}},
        {{3, 1.5f, {nan, 1, 1}}, {1, 1.5f, {1, 1, 1}}},    {{1, 1.5f, {1, 1, 1}}, {0, 1.5f, {1, 1, 1}}},
    };
    pt_dielectric got[4];
    for (const auto &b : bad) {
        EXPECT(pt_scene_set_dielectrics(&scene, b, 2) == PT_ERR_INVALID_ARGUMENT);
        EXPECT(pt_scene_get_dielectrics(&scene, got, &n) == PT_OK && n == 2 && same(got[0], first[0]) && same(got[1], first[1]));
    }
    EXPECT(pt_scene_set_dielectrics(&scene, first, -1) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_set_dielectrics(&scene, nullptr, 2) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_set_dielectrics(nullptr, first, 2) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_get_dielectrics(nullptr, got, &n) == PT_ERR_INVALID_ARGUMENT && pt_scene_get_dielectrics(&scene, got, nullptr) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_get_dielectrics(&scene, got, &n) == PT_OK && n == 2 && same(got[0], first[0]) && same(got[1], first[1]));
    // the limits of the ranges are allowed
    const pt_dielectric edge[3] = {{1, 0.125f, {0, 1, 0}}, {2, 8.0f, {1, 1, 1}}, {3, 1.0f, {0.5f, 0.5f, 0.5f}}};
    EXPECT(pt_scene_set_dielectrics(&scene, edge, 3) == PT_OK && pt_scene_get_dielectrics(&scene, got, &n) == PT_OK && n == 3 && same(got[2], edge[2]));
    // the frame's setters: every copy takes the list, a refused call changes none
    g_frame_scenes = {&scene, &copy};
    pt_frame *frame = reinterpret_cast<pt_frame *>(&g_frame_scenes);   // (never dereferenced: frame_scenes above answers for it)
    EXPECT(pt_frame_set_dielectrics(frame, first, 2) == PT_OK);
    EXPECT(pt_scene_get_dielectrics(&copy, got, &n) == PT_OK && n == 2 && same(got[1], first[1]));
    EXPECT(pt_frame_set_dielectrics(frame, bad[0], 2) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_frame_get_dielectrics(frame, got, &n) == PT_OK && n == 2 && same(got[0], first[0]));
    EXPECT(pt_frame_set_dielectrics(nullptr, first, 2) == PT_ERR_INVALID_ARGUMENT && pt_frame_get_dielectrics(nullptr, got, &n) == PT_ERR_INVALID_ARGUMENT);
    // clear: NULL or n == 0
    EXPECT(pt_frame_set_dielectrics(frame, nullptr, 0) == PT_OK && pt_scene_get_dielectrics(&copy, nullptr, &n) == PT_OK && n == 0);
    EXPECT(pt_scene_set_dielectrics(&scene, first, 2) == PT_OK && pt_scene_set_dielectrics(&scene, first, 0) == PT_OK);
    EXPECT(pt_scene_get_dielectrics(&scene, got, &n) == PT_OK && n == 0);
    if (failures) return 1;
    std::printf("glass host ok\n");
    return 0;
}
