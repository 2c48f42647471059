// The host side of the albedo textures (path-tracing_amd/csrc/pt_texture_capi.cpp, and the OBJ / MTL loader of pt_scene.cpp) under
// AddressSanitizer + UBSan, as a program of its own (tests/test_texture_host.py builds and runs it with the directory of its OBJ / MTL /
// BMP trio as argument): on host-only handles (device -1: no HIP call is made) the setters with every refusal, a refused call leaving
// the handle as it was, the frame's setters, clear and get; the lookup at the special coordinates, its indices inside the texture; the
// BMP decode; the loader's vt and map_Kd.  The helpers pt_texture_capi.cpp takes from the C API's main translation unit are defined here.
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
    // the loader: vt per corner, map_Kd per material
    pt_scene scene, copy;   // host-only: device -1
    scene.shared = std::make_shared<pt_scene_host>();
    std::string err;
    bool io = false;
    EXPECT(pt::load_obj(dir, "t.obj", scene.shared->host, err, io));
    const pt::HostScene &h = scene.shared->host;
    EXPECT(h.n_tri() == 3 && h.n_mat() == 3 && h.tri_uv.size() == 18 && h.map_kd.size() == 3);
    EXPECT(h.tri_uv[2] == 2.0f && h.tri_uv[5] == -3.0f && h.tri_uv[6] == 0.25f && h.tri_uv[8] == 0.0f && h.tri_uv[17] == 0.0f);
    EXPECT(h.map_kd[0] == "lamp.bmp" && h.map_kd[1].empty() && h.map_kd[2] == "wall.bmp");
    pt::build_device_tables(h, scene.shared->tables);
    copy.shared = scene.shared;
    const char *name = nullptr;
    EXPECT(pt_scene_get_map_kd(&scene, 2, &name) == PT_OK && std::string(name) == "wall.bmp");
    EXPECT(pt_scene_get_map_kd(&scene, 3, &name) == PT_ERR_INVALID_ARGUMENT && pt_scene_get_map_kd(&scene, -1, &name) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_get_map_kd(nullptr, 0, &name) == PT_ERR_INVALID_ARGUMENT && pt_scene_get_map_kd(&scene, 0, nullptr) == PT_ERR_INVALID_ARGUMENT);

    // the barycentrics' record on known values: a right triangle at the origin (exact), the getter on the loaded scene (its three
    // triangles share the plane z = 5), and pt_texture.hpp's evaluation at the corners and at a point inside
    {
        const float a[3] = {0, 0, 0}, b[3] = {1, 0, 0}, c[3] = {0, 1, 0}, l0[3] = {1, 1, 1}, l1[3] = {2, 2, 2}, l2[3] = {4, 4, 4};
        const pt::TexBary r = pt::tex_bary_record(a, b, c), z = pt::tex_bary_record(l0, l1, l2);
        EXPECT(r.a1[0] == 1.0f && r.a1[1] == 0.0f && r.a1[2] == 0.0f && r.c1 == 0.0f && r.a2[0] == 0.0f && r.a2[1] == 1.0f && r.a2[2] == 0.0f && r.c2 == 0.0f);
        EXPECT(z.a1[0] == 0.0f && z.a1[1] == 0.0f && z.a1[2] == 0.0f && z.c1 == 0.0f && z.a2[0] == 0.0f && z.c2 == 0.0f);   // collinear: the zero record
        float b1 = -1.0f, b2 = -1.0f, u = 0.0f, v = 0.0f;
        pt::tex_barycentrics_record(r.a1[0], r.a1[1], r.a1[2], r.c1, r.a2[0], r.a2[1], r.a2[2], r.c2, 0.25f, 0.5f, 7.0f, b1, b2);
        EXPECT(b1 == 0.25f && b2 == 0.5f);
        pt::tex_interpolate(0.0f, 0.0f, 2.0f, 0.0f, 2.0f, -3.0f, b1, b2, u, v);   // b0 = 0.25: u = 0.5 + 1, v = -1.5
        EXPECT(u == 1.5f && v == -1.5f);
        float vx, vy;
        pt::tex_barycentrics(0, 0, 0, 1, 0, 0, 0, 1, 0, 0.25f, 0.5f, 0.0f, vx, vy);   // the vertex form agrees here
        EXPECT(vx == 0.25f && vy == 0.5f);
        std::vector<float> recs(8 * 3, -1.0f);
        EXPECT(pt_scene_get_texture_records(&scene, recs.data()) == PT_OK && recs[2] == 0.0f && recs[6] == 0.0f);   // nothing along z
        EXPECT(pt_scene_get_texture_records(nullptr, recs.data()) == PT_ERR_INVALID_ARGUMENT && pt_scene_get_texture_records(&scene, nullptr) == PT_ERR_INVALID_ARGUMENT);
    }

    // the BMP decode
    int32_t w = 0, hh = 0;
    EXPECT(pt_texture_load_bmp((dir + "wall.bmp").c_str(), 2.2f, &w, &hh, nullptr) == PT_OK && w == 3 && hh == 5);
    std::vector<float> wall(static_cast<size_t>(w) * hh * 3);
    EXPECT(pt_texture_load_bmp((dir + "wall.bmp").c_str(), 2.2f, &w, &hh, wall.data()) == PT_OK);
    for (float t : wall) EXPECT(t >= 0.0f && t <= 1.0f);
    EXPECT(pt_texture_load_bmp((dir + "wall.bmp").c_str(), nan, &w, &hh, wall.data()) == PT_OK);
    EXPECT(pt_texture_load_bmp((dir + "none.bmp").c_str(), 2.2f, &w, &hh, nullptr) == PT_ERR_IO);
    EXPECT(pt_texture_load_bmp((dir + "t.obj").c_str(), 2.2f, &w, &hh, nullptr) == PT_ERR_PARSE);
    EXPECT(pt_texture_load_bmp(nullptr, 2.2f, &w, &hh, nullptr) == PT_ERR_INVALID_ARGUMENT);

    // the lookup at the special coordinates, both filters, 1 x 1 up to 3 x 5
    const float special[] = {0.0f, 0.5f, std::nextafter(1.0f, 0.0f), 1.0f, -1e-9f, -0.25f, 1e6f, 1073741824.0f, -1073741824.0f, nan, inf, -inf, 3.0e38f};
    std::vector<float> uv;
    for (float a : special)
        for (float b : special) { uv.push_back(a); uv.push_back(b); }
    const int32_t n_uv = static_cast<int32_t>(uv.size() / 2);
    std::vector<float> out(3 * static_cast<size_t>(n_uv));
    std::vector<int32_t> idx(4 * static_cast<size_t>(n_uv));
    for (int filter = 0; filter < 2; ++filter) {
        const int sizes[][2] = {{1, 1}, {2, 2}, {3, 5}};
        for (const auto &sz : sizes) {
            EXPECT(pt_texture_lookup(sz[0], sz[1], wall.data(), filter, n_uv, uv.data(), out.data(), idx.data()) == PT_OK);
            for (int32_t i : idx) EXPECT(i >= 0 && i < sz[0] * sz[1]);
            for (float t : out) EXPECT(std::isfinite(t));
        }
    }
    EXPECT(pt_texture_lookup(0, 1, wall.data(), 0, n_uv, uv.data(), out.data(), nullptr) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_texture_lookup(3, 5, wall.data(), 2, n_uv, uv.data(), out.data(), nullptr) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_texture_lookup(3, 5, nullptr, 0, n_uv, uv.data(), out.data(), nullptr) == PT_ERR_INVALID_ARGUMENT);

    // the setters: a list needs coordinates; every refusal leaves the handle as it was
    int32_t n = -1, has = -1;
    EXPECT(pt_scene_get_textures(&scene, nullptr, &n) == PT_OK && n == 0 && pt_scene_get_texcoords(&scene, nullptr, &has) == PT_OK && has == 0);
    const pt_texture first[2] = {{2, 3, 5, PT_TEXTURE_BILINEAR, wall.data()}, {0, 1, 1, PT_TEXTURE_NEAREST, wall.data() + 6}};
    EXPECT(pt_scene_set_textures(&scene, first, 2) == PT_ERR_INVALID_ARGUMENT);   // no coordinates yet
    EXPECT(pt_scene_set_texcoords(&scene, h.tri_uv.data()) == PT_OK && pt_scene_get_texcoords(&scene, nullptr, &has) == PT_OK && has == 1);
    EXPECT(pt_scene_set_textures(&scene, first, 2) == PT_OK);
    std::vector<float> bad_texels(wall.begin(), wall.begin() + 45), nan_texels = bad_texels;
    bad_texels[44] = -1.0f;
    nan_texels[7] = nan;
    const pt_texture bad[][2] = {
        {{3, 3, 5, 1, wall.data()}, {0, 1, 1, 0, wall.data()}},  {{-1, 3, 5, 1, wall.data()}, {0, 1, 1, 0, wall.data()}}, {{2, 3, 5, 1, wall.data()}, {2, 1, 1, 0, wall.data()}},
        {{2, 0, 5, 1, wall.data()}, {0, 1, 1, 0, wall.data()}},  {{2, 3, PT_TEXTURE_MAX_SIDE + 1, 1, wall.data()}, {0, 1, 1, 0, wall.data()}},
        {{2, 3, 5, 2, wall.data()}, {0, 1, 1, 0, wall.data()}},  {{2, 3, 5, 1, nullptr}, {0, 1, 1, 0, wall.data()}},
        {{2, 3, 5, 1, bad_texels.data()}, {0, 1, 1, 0, wall.data()}}, {{2, 3, 5, 1, nan_texels.data()}, {0, 1, 1, 0, wall.data()}},
    };
    pt_texture got[4];
    auto unchanged = [&](const pt_scene *s) {
        return pt_scene_get_textures(s, got, &n) == PT_OK && n == 2 && got[0].material == 2 && got[0].width == 3 && got[0].height == 5 && got[1].material == 0 &&
               std::memcmp(got[0].rgb, wall.data(), 45 * sizeof(float)) == 0 && got[1].rgb[0] == wall[6];
    };
    for (const auto &b : bad) {
        EXPECT(pt_scene_set_textures(&scene, b, 2) == PT_ERR_INVALID_ARGUMENT);
        EXPECT(unchanged(&scene));
    }
    EXPECT(pt_scene_set_textures(&scene, first, -1) == PT_ERR_INVALID_ARGUMENT && pt_scene_set_textures(&scene, nullptr, 2) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_set_textures(nullptr, first, 2) == PT_ERR_INVALID_ARGUMENT && pt_scene_get_textures(nullptr, got, &n) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_set_texcoords(&scene, nullptr) == PT_ERR_INVALID_ARGUMENT && unchanged(&scene));   // not while a list is set
    // a dielectric cannot be textured
    auto glass = std::make_shared<pt_glass_list>();
    glass->table.assign(3, pt::GlassRec{});
    glass->table[1].ior = 1.5f;
    scene.surface.glass = glass;
    const pt_texture on_glass[1] = {{1, 1, 1, 0, wall.data()}};
    EXPECT(pt_scene_set_textures(&scene, on_glass, 1) == PT_ERR_INVALID_ARGUMENT && unchanged(&scene));
    scene.surface.glass.reset();
    // the frame's setters: every copy takes coordinates and list, a refused call changes none
    g_frame_scenes = {&scene, &copy};
    pt_frame *frame = reinterpret_cast<pt_frame *>(&g_frame_scenes);   // (never dereferenced: frame_scenes above answers for it)
    EXPECT(pt_frame_set_texcoords(frame, h.tri_uv.data()) == PT_OK && pt_frame_set_textures(frame, first, 2) == PT_OK && unchanged(&copy));
    EXPECT(pt_frame_set_textures(frame, bad[0], 2) == PT_ERR_INVALID_ARGUMENT && unchanged(&copy) && unchanged(&scene));
    EXPECT(pt_frame_get_textures(frame, got, &n) == PT_OK && n == 2 && pt_frame_get_texcoords(frame, nullptr, &has) == PT_OK && has == 1);
    EXPECT(pt_frame_set_textures(nullptr, first, 2) == PT_ERR_INVALID_ARGUMENT && pt_frame_get_textures(nullptr, got, &n) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_frame_set_texcoords(nullptr, nullptr) == PT_ERR_INVALID_ARGUMENT && pt_frame_get_texcoords(nullptr, nullptr, &has) == PT_ERR_INVALID_ARGUMENT);
    // clear: NULL or n == 0, then the coordinates may go
    EXPECT(pt_frame_set_textures(frame, nullptr, 0) == PT_OK && pt_scene_get_textures(&copy, nullptr, &n) == PT_OK && n == 0);
    EXPECT(pt_frame_set_texcoords(frame, nullptr) == PT_OK && pt_scene_get_texcoords(&copy, nullptr, &has) == PT_OK && has == 0);
    if (failures) return 1;
    std::printf("texture host ok\n");
    return 0;
}
