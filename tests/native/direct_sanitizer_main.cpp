// The host side of direct lighting (path-tracing_amd/csrc/pt_direct_capi.cpp, the texture setter of pt_texture_capi.cpp and the loader
// of pt_scene.cpp) under AddressSanitizer + UBSan, as a program of its own (tests/test_direct_host.py builds and runs it with the
// directory of its OBJ files as argument): on host-only handles (device -1: no HIP call is made) the table builder on a scene with
// several lights and a degenerate one, the switch, every refusal in both orders with the texture setter with a refused call leaving the
// handle as it was, the frame's setter and getters; pt_direct_term at its guards.  The helpers the C API's main translation unit
// defines are defined here.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
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
    pt_scene scene, copy, dark;   // host-only: device -1
    scene.shared = std::make_shared<pt_scene_host>();
    std::string err;
    bool io = false;
    EXPECT(pt::load_obj(dir, "lights_room.obj", scene.shared->host, err, io));
    pt::build_device_tables(scene.shared->host, scene.shared->tables);
    scene.surface.texcoords = std::make_shared<const std::vector<float>>(6 * static_cast<size_t>(scene.shared->host.n_tri()), 0.25f);
    copy.shared = scene.shared;
    copy.surface.texcoords = scene.surface.texcoords;

    // the table: five lights (two quads and a triangle; the degenerate emissive triangle is none), cdf ascending to exactly 1
    int32_t n = -1, on = -1;
    float area = 0.0f;
    EXPECT(pt_scene_get_lights(&scene, nullptr, &n, &area) == PT_OK && n == 5 && area > 0.0f);
    std::vector<pt_light> lights(static_cast<size_t>(n) + 1);
    EXPECT(pt_scene_get_lights(&scene, lights.data(), &n, nullptr) == PT_OK && n == 5 && lights[4].cdf == 1.0f);
    for (int i = 1; i < n; ++i) EXPECT(lights[i].cdf > lights[i - 1].cdf && lights[i].triangle > lights[i - 1].triangle);
    EXPECT(pt_scene_get_lights(nullptr, nullptr, &n, nullptr) == PT_ERR_INVALID_ARGUMENT && pt_scene_get_lights(&scene, nullptr, nullptr, nullptr) == PT_ERR_INVALID_ARGUMENT);

    // the switch, and both orders with the texture setter
    const float texel[3] = {0.5f, 0.5f, 0.5f};
    const pt_texture on_lamp = {0, 1, 1, 0, texel}, on_wall = {1, 1, 1, 0, texel};
    EXPECT(pt_scene_get_direct_lighting(&scene, &on) == PT_OK && on == 0);
    EXPECT(pt_scene_set_direct_lighting(&scene, 1) == PT_OK && pt_scene_get_direct_lighting(&scene, &on) == PT_OK && on == 1);
    EXPECT(pt_scene_set_textures(&scene, &on_lamp, 1) == PT_ERR_INVALID_ARGUMENT);   // a light is not textured while the switch is on ...
    EXPECT(pt_scene_set_textures(&scene, &on_wall, 1) == PT_OK);
    EXPECT(pt_scene_set_direct_lighting(&scene, 0) == PT_OK && pt_scene_get_direct_lighting(&scene, &on) == PT_OK && on == 0);
    EXPECT(pt_scene_set_textures(&scene, &on_lamp, 1) == PT_OK);
    EXPECT(pt_scene_set_direct_lighting(&scene, 1) == PT_ERR_INVALID_ARGUMENT);      // ... and the switch refuses a textured light
    EXPECT(pt_scene_get_direct_lighting(&scene, &on) == PT_OK && on == 0);
    EXPECT(pt_scene_set_textures(&scene, nullptr, 0) == PT_OK);
    EXPECT(pt_scene_set_direct_lighting(nullptr, 1) == PT_ERR_INVALID_ARGUMENT && pt_scene_get_direct_lighting(&scene, nullptr) == PT_ERR_INVALID_ARGUMENT);

    // a scene without a light: the walls alone
    dark.shared = std::make_shared<pt_scene_host>();
    pt::HostScene &dh = dark.shared->host;
    dh = scene.shared->host;
    for (int m = 0; m < dh.n_mat(); ++m) dh.mat[10 * m + 3] = dh.mat[10 * m + 4] = dh.mat[10 * m + 5] = 0.0f;
    pt::build_device_tables(dh, dark.shared->tables);
    EXPECT(pt_scene_get_lights(&dark, nullptr, &n, &area) == PT_OK && n == 0);
    EXPECT(pt_scene_set_direct_lighting(&dark, 1) == PT_ERR_INVALID_ARGUMENT && pt_scene_get_direct_lighting(&dark, &on) == PT_OK && on == 0);
    EXPECT(pt_scene_set_direct_lighting(&dark, 0) == PT_OK);

    // the frame's setter: both copies or none
    g_frame_scenes = {&scene, &copy};
    pt_frame *frame = reinterpret_cast<pt_frame *>(&g_frame_scenes);   // (never dereferenced: frame_scenes above answers for it)
    EXPECT(pt_frame_set_direct_lighting(frame, 1) == PT_OK && pt_scene_get_direct_lighting(&copy, &on) == PT_OK && on == 1);
    EXPECT(pt_frame_get_direct_lighting(frame, &on) == PT_OK && on == 1 && pt_frame_get_lights(frame, lights.data(), &n, &area) == PT_OK && n == 5);
    EXPECT(pt_frame_set_direct_lighting(frame, 0) == PT_OK && pt_scene_get_direct_lighting(&copy, &on) == PT_OK && on == 0);
    EXPECT(pt_scene_set_textures(&copy, &on_lamp, 1) == PT_OK);
    EXPECT(pt_frame_set_direct_lighting(frame, 1) == PT_ERR_INVALID_ARGUMENT);       // (the second copy's textured light)
    EXPECT(pt_scene_get_direct_lighting(&scene, &on) == PT_OK && on == 0 && pt_scene_get_direct_lighting(&copy, &on) == PT_OK && on == 0);
    EXPECT(pt_frame_set_direct_lighting(nullptr, 1) == PT_ERR_INVALID_ARGUMENT && pt_frame_get_direct_lighting(nullptr, &on) == PT_ERR_INVALID_ARGUMENT &&
           pt_frame_get_lights(nullptr, nullptr, &n, nullptr) == PT_ERR_INVALID_ARGUMENT);

    // the term at its guards: a point that coincides with the origin (r2 == 0), each cosine at 0, the fold u1 + u2 > 1
    EXPECT(pt_scene_get_lights(&scene, lights.data(), &n, &area) == PT_OK);
    const pt_light &l0 = lights[0];
    const float at_v0[3] = {l0.v0[0], l0.v0[1], l0.v0[2]};
    const float origins[] = {at_v0[0], at_v0[1], at_v0[2], 0, 0, -10, 0, 0, -10, 0, 0, -10, 0, 5.5f, -10};
    const float normals[] = {0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0};
    const float shading[] = {0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0};
    const float ones[15] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    const uint32_t w0[5] = {0u, 0u, 0u, 0u, 0u}, w1[5] = {0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 7u, 0x80000000u}, w2[5] = {0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 9u};
    int32_t which[5], has[5];
    float pts[15], dirs[15], terms[15];
    EXPECT(pt_direct_term(5, lights.data(), n, area, origins, normals, shading, ones, ones, w0, w1, w2, which, pts, dirs, terms, has) == PT_OK);
    for (int i = 0; i < 5; ++i) {
        EXPECT(which[i] >= 0 && which[i] < n);
        if (!has[i]) EXPECT(terms[3 * i] == 0.0f && terms[3 * i + 1] == 0.0f && terms[3 * i + 2] == 0.0f);
        else EXPECT(std::isfinite(terms[3 * i]) && terms[3 * i] > 0.0f);
    }
    EXPECT(has[1] == 1 && has[2] == 0 && has[3] == 0 && has[4] == 0);
    EXPECT(pt_direct_term(0, lights.data(), n, area, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PT_OK);
    EXPECT(pt_direct_term(-1, lights.data(), n, area, origins, normals, shading, ones, ones, w0, w1, w2, which, pts, dirs, terms, has) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_direct_term(5, nullptr, n, area, origins, normals, shading, ones, ones, w0, w1, w2, which, pts, dirs, terms, has) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_direct_term(5, lights.data(), 0, area, origins, normals, shading, ones, ones, w0, w1, w2, which, pts, dirs, terms, has) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_direct_term(5, lights.data(), n, area, nullptr, normals, shading, ones, ones, w0, w1, w2, which, pts, dirs, terms, has) == PT_ERR_INVALID_ARGUMENT);
    if (failures) return 1;
    std::printf("direct host ok\n");
    return 0;
}
