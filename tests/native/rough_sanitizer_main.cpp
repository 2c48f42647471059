// The host side of rough specular reflection (path-tracing_amd/csrc/pt_rough_capi.cpp, the dielectric setter of pt_glass_capi.cpp and the
// MTL reader of pt_scene.cpp) under AddressSanitizer + UBSan, as a program of its own (tests/test_rough_host.py builds and runs it with
// the directory of its OBJ files as argument): on host-only handles (device -1: no HIP call is made) the loader's Pr, the setter's
// validation with a refused call leaving the handle as it was, both orders against the dielectric list, the frame's setter, clear and
// get; pt_rough_step on special normals, directions, alphas and words.  The helpers the C API's main translation unit defines are
// defined here.
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
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

    // the step: axis-aligned normals (n.z = +-1, -0.0), head-on, grazing and back-side incidence, both bounds of alpha, extreme words
    const float normals[] = {0, 0, 1, 0, 0, -1, 1, 0, -0.0f, 0, 1, 0, 0.6f, 0.8f, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1};
    const float dirs[] = {0, 0, -1, 0, 0, -1, 0, 1, 0, 0, 1, 0, 0.8f, -0.6f, 0, 1, 0, 0, 0.6f, 0, 0.8f, 0.6f, 0, -0.8f};
    const float alphas[] = {PT_ROUGH_ALPHA_MIN, 1.0f, 0.3f, PT_ROUGH_ALPHA_MIN, 1.0f, 0.05f, 0.5f, 1.0f};
    const uint32_t w1[] = {0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 512u, 0x80000000u, 7u, 0xFFFFFFFFu};
    const uint32_t w2[] = {0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0x40000000u, 0xC0000000u, 9u, 0u};
    float l[24], g1[8], h[24];
    EXPECT(pt_rough_step(8, normals, dirs, alphas, w1, w2, l, g1, h) == PT_OK);
    for (int i = 0; i < 8; ++i) {
        EXPECT(std::isfinite(l[3 * i]) && std::isfinite(l[3 * i + 1]) && std::isfinite(l[3 * i + 2]) && g1[i] >= 0.0f && g1[i] <= 1.0f && h[3 * i + 2] >= 0.0f);
        EXPECT(std::fabs(std::sqrt(l[3 * i] * l[3 * i] + l[3 * i + 1] * l[3 * i + 1] + l[3 * i + 2] * l[3 * i + 2]) - 1.0f) < 1e-6f);
    }
    EXPECT(pt_rough_step(8, normals, dirs, alphas, w1, w2, l, g1, nullptr) == PT_OK && pt_rough_step(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PT_OK);
    EXPECT(pt_rough_step(-1, normals, dirs, alphas, w1, w2, l, g1, h) == PT_ERR_INVALID_ARGUMENT && pt_rough_step(8, nullptr, dirs, alphas, w1, w2, l, g1, h) == PT_ERR_INVALID_ARGUMENT);
    const float bad_alpha[] = {0.3f, nan, 0.3f, 0.3f, 0.3f, 0.3f, 0.3f, 0.3f};
    EXPECT(pt_rough_step(8, normals, dirs, bad_alpha, w1, w2, l, g1, h) == PT_ERR_INVALID_ARGUMENT);

    // the loader's Pr and the setters, on a host-only scene and a "frame" of two copies of it
    pt_scene scene, copy;   // host-only: device -1
    scene.shared = std::make_shared<pt_scene_host>();
    std::string err;
    bool io = false;
    EXPECT(pt::load_obj(dir, "rough_room.obj", scene.shared->host, err, io));
    const pt::HostScene &hs = scene.shared->host;
    EXPECT(hs.n_mat() == 6 && hs.mat_pr.size() == 6 && hs.mat_pr[0] == -1.0f && hs.mat_pr[2] == 0.25f && hs.mat_pr[3] == 1.5f && hs.mat_pr[5] == -1.0f);
    pt::build_device_tables(hs, scene.shared->tables);
    copy.shared = scene.shared;
    float pr[6];
    EXPECT(pt_scene_get_mtl_roughness(&scene, pr) == PT_OK && pr[4] == 0.4f && pt_scene_get_mtl_roughness(nullptr, pr) == PT_ERR_INVALID_ARGUMENT);
    int32_t n = -1;
    pt_rough got[4];
    const pt_rough mine[2] = {{2, 0.25f}, {5, PT_ROUGH_ALPHA_MIN}};
    EXPECT(pt_scene_get_roughness(&scene, nullptr, &n) == PT_OK && n == 0);
    EXPECT(pt_scene_set_roughness(&scene, mine, 2) == PT_OK && pt_scene_get_roughness(&scene, got, &n) == PT_OK && n == 2 && got[1].material == 5 && got[1].alpha == PT_ROUGH_ALPHA_MIN);
    const pt_rough refused[][2] = {{{6, 0.3f}, {2, 0.3f}}, {{-1, 0.3f}, {2, 0.3f}}, {{2, 0.3f}, {2, 0.4f}}, {{2, nan}, {3, 0.3f}}, {{2, inf}, {3, 0.3f}},
                                   {{2, 0.0f}, {3, 0.3f}}, {{2, 1.5f}, {3, 0.3f}}, {{1, 0.3f}, {2, 0.3f}}, {{4, 0.3f}, {2, 0.3f}}, {{0, 0.3f}, {2, 0.3f}}};
    for (const auto &r : refused) {
        EXPECT(pt_scene_set_roughness(&scene, r, 2) == PT_ERR_INVALID_ARGUMENT);
        EXPECT(pt_scene_get_roughness(&scene, got, &n) == PT_OK && n == 2 && got[0].material == 2 && got[0].alpha == 0.25f);   // a refused call changed nothing
    }
    EXPECT(pt_scene_set_roughness(&scene, mine, -1) == PT_ERR_INVALID_ARGUMENT && pt_scene_set_roughness(&scene, nullptr, 2) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_set_roughness(nullptr, mine, 2) == PT_ERR_INVALID_ARGUMENT && pt_scene_get_roughness(nullptr, nullptr, &n) == PT_ERR_INVALID_ARGUMENT);
    const pt_dielectric glass5 = {5, 1.5f, {1.0f, 1.0f, 1.0f}}, glass3 = {3, 1.5f, {1.0f, 1.0f, 1.0f}};
    EXPECT(pt_scene_set_dielectrics(&scene, &glass5, 1) == PT_ERR_INVALID_ARGUMENT);   // a rough material is no dielectric ...
    EXPECT(pt_scene_set_dielectrics(&scene, &glass3, 1) == PT_OK);
    const pt_rough three = {3, 0.3f};
    EXPECT(pt_scene_set_roughness(&scene, &three, 1) == PT_ERR_INVALID_ARGUMENT);      // ... and a dielectric is not rough
    EXPECT(pt_scene_get_roughness(&scene, got, &n) == PT_OK && n == 2);
    EXPECT(pt_scene_set_dielectrics(&scene, nullptr, 0) == PT_OK);
    g_frame_scenes = {&scene, &copy};
    pt_frame *frame = reinterpret_cast<pt_frame *>(&g_frame_scenes);   // (never dereferenced: frame_scenes above answers for it)
    EXPECT(pt_frame_set_roughness(frame, &three, 1) == PT_OK && pt_scene_get_roughness(&copy, got, &n) == PT_OK && n == 1 && got[0].material == 3);
    EXPECT(pt_frame_set_roughness(frame, refused[0], 2) == PT_ERR_INVALID_ARGUMENT && pt_frame_get_roughness(frame, got, &n) == PT_OK && n == 1 && got[0].alpha == 0.3f);
    EXPECT(pt_frame_set_roughness(nullptr, mine, 2) == PT_ERR_INVALID_ARGUMENT && pt_frame_get_roughness(nullptr, nullptr, &n) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_frame_set_roughness(frame, nullptr, 0) == PT_OK && pt_scene_get_roughness(&copy, nullptr, &n) == PT_OK && n == 0);
    if (failures) return 1;
    std::printf("rough host ok\n");
    return 0;
}
