// The host side of environment sampling (path-tracing_amd/csrc/pt_envdirect_capi.cpp with the table builder of pt_envdirect.hpp, the
// environment setters of pt_environment_capi.cpp, the light table of pt_direct_capi.cpp, the texture setter of pt_texture_capi.cpp and
// the loader of pt_scene.cpp) under AddressSanitizer + UBSan, as a program of its own (tests/test_envdirect_host.py builds and runs it
// with the directory of its OBJ files as argument): on host-only handles (device -1: no HIP call is made) the table of the smallest
// map, of one that is no power of two and of one above 256 texels a side, the switch with its share, every refusal with a refused
// call leaving the handle as it was, the rebuild when the environment is replaced, the frame's setter and getters, and
// pt_envdirect_term at its guards.  The helpers the C API's main translation unit defines are defined here.
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

static std::vector<float> map_of(int n, float sky, float sun) {
    std::vector<float> m(static_cast<size_t>(n) * n * 3, sky);
    for (int c = 0; c < 3; ++c) m[3 * (static_cast<size_t>(n) * (3 * n / 4) + n / 2 + 1) + c] = sun;
    return m;
}

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : "./";
    pt_scene scene, copy, dark;   // host-only: device -1
    std::string err;
    bool io = false;
    scene.shared = std::make_shared<pt_scene_host>();
    EXPECT(pt::load_obj(dir, "lamp_room.obj", scene.shared->host, err, io));
    pt::build_device_tables(scene.shared->host, scene.shared->tables);
    scene.surface.texcoords = std::make_shared<const std::vector<float>>(6 * static_cast<size_t>(scene.shared->host.n_tri()), 0.25f);
    copy.shared = scene.shared;
    copy.surface.texcoords = scene.surface.texcoords;
    dark.shared = std::make_shared<pt_scene_host>();
    EXPECT(pt::load_obj(dir, "dark_room.obj", dark.shared->host, err, io));
    pt::build_device_tables(dark.shared->host, dark.shared->tables);

    int32_t on = -1, cells = -1;
    float share = -1.0f;
    pt_env_sampling given = {0.5f};
    const pt_env_sampling dflt = {0.0f}, quarter = {0.25f}, one = {1.0f}, bad_lo = {-0.5f}, bad_nan = {std::nanf("")};

    // no environment: refused, and the table getter says so
    EXPECT(pt_scene_set_environment_sampling(&scene, &dflt) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_get_environment_sampling(&scene, &on, &given) == PT_OK && on == 0 && given.share == 0.0f);
    EXPECT(pt_scene_get_environment_sampling_table(&scene, nullptr, &cells, &share) == PT_OK && cells == 0);

    // the tables of three sizes: every cell positive, aliases in range
    for (int n : {8, 12, 320}) {
        const std::vector<float> m = map_of(n, n == 12 ? 0.0f : 0.2f, 5000.0f);
        EXPECT(pt_scene_set_environment_map(&scene, n, m.data()) == PT_OK);
        EXPECT(pt_scene_get_environment_sampling_table(&scene, nullptr, &cells, &share) == PT_OK && cells == (n < 256 ? n : 256));
        std::vector<pt_env_sample_record> rec(static_cast<size_t>(cells) * cells);
        EXPECT(pt_scene_get_environment_sampling_table(&scene, rec.data(), &cells, &share) == PT_OK && share >= 0.125f && share <= 0.875f);
        for (const pt_env_sample_record &r : rec)
            EXPECT(r.accept > 0.0f && r.accept <= 1.0f && r.alias >= 0 && r.alias < cells * cells && r.pdf_self > 0.0f && r.pdf_alias > 0.0f);
    }

    // the switch and its refusals
    const std::vector<float> m8 = map_of(8, 0.2f, 50.0f), black(8 * 8 * 3, 0.0f);
    EXPECT(pt_scene_set_environment_map(&scene, 8, m8.data()) == PT_OK);
    EXPECT(pt_scene_set_environment_sampling(&scene, &bad_lo) == PT_ERR_INVALID_ARGUMENT && pt_scene_set_environment_sampling(&scene, &one) == PT_ERR_INVALID_ARGUMENT &&
           pt_scene_set_environment_sampling(&scene, &bad_nan) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_get_environment_sampling(&scene, &on, nullptr) == PT_OK && on == 0);
    EXPECT(pt_scene_set_environment_sampling(&scene, &quarter) == PT_OK && pt_scene_get_environment_sampling(&scene, &on, &given) == PT_OK && on == 1 && given.share == 0.25f);
    EXPECT(pt_scene_get_environment_sampling_table(&scene, nullptr, &cells, &share) == PT_OK && cells == 8 && share == 0.25f);
    EXPECT(pt_scene_set_environment_map(&scene, 8, black.data()) == PT_ERR_INVALID_ARGUMENT);       // a black map: nothing changes
    EXPECT(pt_scene_set_environment_file(&scene, nullptr, nullptr) == PT_ERR_INVALID_ARGUMENT);     // removal while the switch is on
    int32_t n_map = 0;
    EXPECT(pt_scene_get_environment(&scene, &n_map, nullptr) == PT_OK && n_map == 8);
    const std::vector<float> m12 = map_of(12, 0.1f, 70.0f);
    EXPECT(pt_scene_set_environment_map(&scene, 12, m12.data()) == PT_OK);                          // replaced: the table follows
    EXPECT(pt_scene_get_environment_sampling_table(&scene, nullptr, &cells, &share) == PT_OK && cells == 12 && share == 0.25f);
    const float texel[3] = {0.5f, 0.5f, 0.5f};
    const pt_texture on_lamp = {0, 1, 1, 0, texel}, on_wall = {1, 1, 1, 0, texel};
    EXPECT(pt_scene_set_textures(&scene, &on_lamp, 1) == PT_ERR_INVALID_ARGUMENT && pt_scene_set_textures(&scene, &on_wall, 1) == PT_OK);
    EXPECT(pt_scene_set_environment_sampling(&scene, nullptr) == PT_OK && pt_scene_get_environment_sampling(&scene, &on, nullptr) == PT_OK && on == 0);
    EXPECT(pt_scene_set_textures(&scene, &on_lamp, 1) == PT_OK);
    EXPECT(pt_scene_set_environment_sampling(&scene, &dflt) == PT_ERR_INVALID_ARGUMENT);            // a textured emitter
    EXPECT(pt_scene_set_textures(&scene, nullptr, 0) == PT_OK);
    EXPECT(pt_scene_set_environment_file(&scene, nullptr, nullptr) == PT_OK);                       // removal with the switch off

    // a scene without emitters: share 1, whatever the map
    EXPECT(pt_scene_set_environment_map(&dark, 8, m8.data()) == PT_OK);
    EXPECT(pt_scene_set_environment_sampling(&dark, &quarter) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_set_environment_sampling(&dark, &dflt) == PT_OK && pt_scene_get_environment_sampling_table(&dark, nullptr, &cells, &share) == PT_OK && share == 1.0f);
    EXPECT(pt_scene_set_environment_sampling(&dark, &one) == PT_OK);

    // the frame's setter: both copies or none
    g_frame_scenes = {&scene, &copy};
    pt_frame *frame = reinterpret_cast<pt_frame *>(&g_frame_scenes);   // (never dereferenced: frame_scenes above answers for it)
    EXPECT(pt_frame_set_environment_sampling(frame, &dflt) == PT_ERR_INVALID_ARGUMENT);             // no environment yet
    EXPECT(pt_frame_set_environment_map(frame, 8, m8.data()) == PT_OK);
    EXPECT(pt_frame_set_environment_sampling(frame, &dflt) == PT_OK && pt_scene_get_environment_sampling(&copy, &on, nullptr) == PT_OK && on == 1);
    EXPECT(pt_frame_get_environment_sampling(frame, &on, &given) == PT_OK && on == 1 && given.share == 0.0f);
    EXPECT(pt_frame_get_environment_sampling_table(frame, nullptr, &cells, &share) == PT_OK && cells == 8);
    EXPECT(pt_frame_set_environment_map(frame, 12, m12.data()) == PT_OK && copy.surface.envdirect->cells == 12 && scene.surface.envdirect->cells == 12);
    EXPECT(pt_frame_set_environment_map(frame, 8, black.data()) == PT_ERR_INVALID_ARGUMENT && copy.surface.envdirect->cells == 12 && copy.env->n == 12);
    EXPECT(pt_frame_set_environment_sampling(frame, nullptr) == PT_OK && !copy.surface.envdirect && !scene.surface.envdirect);
    EXPECT(pt_scene_set_textures(&copy, &on_lamp, 1) == PT_OK);
    EXPECT(pt_frame_set_environment_sampling(frame, &dflt) == PT_ERR_INVALID_ARGUMENT && !scene.surface.envdirect);   // (the second copy's textured light)
    EXPECT(pt_frame_set_environment_sampling(nullptr, &dflt) == PT_ERR_INVALID_ARGUMENT && pt_frame_get_environment_sampling(nullptr, &on, nullptr) == PT_ERR_INVALID_ARGUMENT &&
           pt_scene_set_environment_sampling(nullptr, &dflt) == PT_ERR_INVALID_ARGUMENT && pt_scene_get_environment_sampling(&scene, nullptr, nullptr) == PT_ERR_INVALID_ARGUMENT);

    // the term at its guards: cn = 0, cs <= 0, the extreme words
    EXPECT(pt_scene_get_environment_sampling_table(&dark, nullptr, &cells, &share) == PT_OK && cells == 8);
    std::vector<pt_env_sample_record> rec(64);
    EXPECT(pt_scene_get_environment_sampling_table(&dark, rec.data(), &cells, &share) == PT_OK);
    const float normals[] = {0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, -1, 0};
    const float shading[] = {0, 1, 0, 0, 1, 0, 0, -1, 0, 0, 1, 0, 0, -1, 0};
    const float ones[15] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    const uint32_t e0[5] = {0x90000000u, 0x90000000u, 0x90000000u, 0xFFFFFFFFu, 0u}, e1[5] = {0u, 0u, 0u, 0xFFFFFFFFu, 0u};
    const uint32_t e2[5] = {0x80000000u, 0x80000000u, 0x80000000u, 0xFFFFFFFFu, 0u}, e3[5] = {0x80000000u, 0x80000000u, 0x80000000u, 0xFFFFFFFFu, 0u};
    int32_t cell[5], has[5];
    float dirs[15], pdf[5], terms[15];
    EXPECT(pt_envdirect_term(5, rec.data(), cells, share, 8, m8.data(), normals, shading, ones, ones, e0, e1, e2, e3, cell, dirs, pdf, terms, has) == PT_OK);
    for (int i = 0; i < 5; ++i) {
        EXPECT(cell[i] >= 0 && cell[i] < 64 && pdf[i] > 0.0f && std::isfinite(pdf[i]));
        if (!has[i]) EXPECT(terms[3 * i] == 0.0f && terms[3 * i + 1] == 0.0f && terms[3 * i + 2] == 0.0f);
        else EXPECT(std::isfinite(terms[3 * i]) && terms[3 * i] >= 0.0f);
    }
    EXPECT(has[0] == 1 && has[1] == 0 && has[2] == 0 && has[4] == 1);
    EXPECT(pt_envdirect_term(0, rec.data(), cells, share, 8, m8.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PT_OK);
    EXPECT(pt_envdirect_term(-1, rec.data(), cells, share, 8, m8.data(), normals, shading, ones, ones, e0, e1, e2, e3, cell, dirs, pdf, terms, has) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_envdirect_term(5, nullptr, cells, share, 8, m8.data(), normals, shading, ones, ones, e0, e1, e2, e3, cell, dirs, pdf, terms, has) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_envdirect_term(5, rec.data(), 300, share, 8, m8.data(), normals, shading, ones, ones, e0, e1, e2, e3, cell, dirs, pdf, terms, has) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_envdirect_term(5, rec.data(), cells, share, 4, m8.data(), normals, shading, ones, ones, e0, e1, e2, e3, cell, dirs, pdf, terms, has) == PT_ERR_INVALID_ARGUMENT);
    rec[3].alias = 64;
    EXPECT(pt_envdirect_term(5, rec.data(), cells, share, 8, m8.data(), normals, shading, ones, ones, e0, e1, e2, e3, cell, dirs, pdf, terms, has) == PT_ERR_INVALID_ARGUMENT);
    if (failures) return 1;
    std::printf("envdirect host ok\n");
    return 0;
}
