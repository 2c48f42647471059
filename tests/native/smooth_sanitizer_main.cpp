// The host side of smooth shading (path-tracing_amd/csrc/pt_smooth_capi.cpp, pt_smooth_normals.cpp and the OBJ loader of pt_scene.cpp)
// under AddressSanitizer + UBSan, as a program of its own (tests/test_smooth_host.py builds and runs it with the directory of its OBJ
// files as argument): the generator on small, degenerate and non-finite inputs; on host-only handles (device -1: no HIP call is made)
// the setter's validation with a refused call leaving the handle as it was, the frame's setter, clear and get; the interpolation at
// special points; the loader's vn on a well-formed and on malformed files.  The helpers the C API's main translation unit defines
// are defined here.
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
    // the generator: two triangles of a square share an edge, one degenerate triangle, one with a NaN vertex
    const float v[4 * 9] = {0, 0, 0, 1, 0, 0, 0, 1, 0,   1, 0, 0, 1, 1, 0, 0, 1, 0,   2, 2, 2, 3, 3, 3, 4, 4, 4,   0, 0, 0, nan, 0, 0, 0, 1, 0};
    std::vector<float> out(4 * 9, -1.0f);
    EXPECT(pt_smooth_normals(4, v, 60.0f, out.data()) == PT_OK);
    for (int k = 0; k < 18; ++k) EXPECT(out[k] == (k % 3 == 2 ? 1.0f : 0.0f));
    for (int k = 18; k < 36; ++k) EXPECT(out[k] == 0.0f);
    EXPECT(pt_smooth_normals(0, nullptr, 60.0f, nullptr) == PT_OK);
    EXPECT(pt_smooth_normals(4, v, 0.0f, out.data()) == PT_OK && pt_smooth_normals(4, v, 180.0f, out.data()) == PT_OK);
    EXPECT(pt_smooth_normals(-1, v, 60.0f, out.data()) == PT_ERR_INVALID_ARGUMENT && pt_smooth_normals(4, nullptr, 60.0f, out.data()) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_smooth_normals(4, v, -1.0f, out.data()) == PT_ERR_INVALID_ARGUMENT && pt_smooth_normals(4, v, 180.5f, out.data()) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_smooth_normals(4, v, nan, out.data()) == PT_ERR_INVALID_ARGUMENT && pt_smooth_normals(4, v, 60.0f, nullptr) == PT_ERR_INVALID_ARGUMENT);

    // the interpolation at special points
    const float N[3] = {0, 0, 1}, n9[9] = {0, 0, 1, 1, 0, 1, 0, 1, 1}, zeros[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const float pts[] = {0, 0, 0, 1, 0, 0, 0.25f, 0.25f, 0, 1e6f, -1e6f, 3, nan, 0, 0, inf, 0, 0, 3e38f, 3e38f, 3e38f};
    float ns[21];
    int32_t own[7];
    EXPECT(pt_shading_normal_at(v, N, n9, 7, pts, ns, own) == PT_OK && own[0] == 1 && ns[2] == 1.0f && own[4] == 0 && ns[14] == 1.0f && own[5] == 0);
    EXPECT(pt_shading_normal_at(v, N, zeros, 7, pts, ns, own) == PT_OK && own[2] == 0 && ns[8] == 1.0f);
    EXPECT(pt_shading_normal_at(v + 18, N, n9, 7, pts, ns, nullptr) == PT_OK);   // a collinear triangle: the zero record
    EXPECT(pt_shading_normal_at(nullptr, N, n9, 7, pts, ns, own) == PT_ERR_INVALID_ARGUMENT && pt_shading_normal_at(v, N, n9, -1, pts, ns, own) == PT_ERR_INVALID_ARGUMENT);

    // the loader: vn per corner, the stored normal without an index, malformed files
    pt_scene scene, copy;   // host-only: device -1
    scene.shared = std::make_shared<pt_scene_host>();
    std::string err;
    bool io = false;
    EXPECT(pt::load_obj(dir, "n.obj", scene.shared->host, err, io));
    const pt::HostScene &h = scene.shared->host;
    EXPECT(h.n_tri() == 2 && h.tri_vn.size() == 18);
    EXPECT(h.tri_vn[0] == 0.0f && h.tri_vn[2] == 2.0f && h.tri_vn[3] == 1.0f && h.tri_vn[8] == h.tri[2]);   // raw vn, raw vn, the stored normal
    {
        pt::HostScene bad, geo;
        EXPECT(!pt::load_obj(dir, "bad.obj", bad, err, io) && !io);            // corner 2 names a vn beyond the list
        EXPECT(pt::load_obj(dir, "n.obj", geo, err, io, true) && geo.tri[2] == 1.0f && geo.tri[0] == 0.0f);
        EXPECT(!pt::load_obj(dir, "none.obj", bad, err, io) && io);
    }
    pt::build_device_tables(h, scene.shared->tables);
    copy.shared = scene.shared;
    int32_t has = -1;
    std::vector<float> got(18, -1.0f), mine(18, 0.5f);
    EXPECT(pt_scene_get_vertex_normals(&scene, got.data(), &has) == PT_OK && has == 1 && got[2] == 2.0f);
    EXPECT(pt_scene_get_vertex_normals(nullptr, got.data(), &has) == PT_ERR_INVALID_ARGUMENT && pt_scene_get_vertex_normals(&scene, got.data(), nullptr) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_get_shading_normals(&scene, nullptr, &has) == PT_OK && has == 0);
    EXPECT(pt_scene_set_shading_normals(&scene, mine.data()) == PT_OK && pt_scene_get_shading_normals(&scene, got.data(), &has) == PT_OK && has == 1 && got == mine);
    std::vector<float> bad = mine;
    bad[17] = nan;
    EXPECT(pt_scene_set_shading_normals(&scene, bad.data()) == PT_ERR_INVALID_ARGUMENT);
    bad[17] = -inf;
    EXPECT(pt_scene_set_shading_normals(&scene, bad.data()) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_scene_get_shading_normals(&scene, got.data(), &has) == PT_OK && has == 1 && got == mine);   // a refused call changed nothing
    EXPECT(pt_scene_set_shading_normals(nullptr, mine.data()) == PT_ERR_INVALID_ARGUMENT && pt_scene_get_shading_normals(nullptr, nullptr, &has) == PT_ERR_INVALID_ARGUMENT);
    std::vector<float> z(18, 0.0f);
    EXPECT(pt_scene_set_shading_normals(&scene, z.data()) == PT_OK);   // zeros are allowed
    g_frame_scenes = {&scene, &copy};
    pt_frame *frame = reinterpret_cast<pt_frame *>(&g_frame_scenes);   // (never dereferenced: frame_scenes above answers for it)
    EXPECT(pt_frame_set_shading_normals(frame, mine.data()) == PT_OK && pt_scene_get_shading_normals(&copy, got.data(), &has) == PT_OK && has == 1 && got == mine);
    EXPECT(pt_frame_set_shading_normals(frame, bad.data()) == PT_ERR_INVALID_ARGUMENT && pt_frame_get_shading_normals(frame, got.data(), &has) == PT_OK && has == 1 && got == mine);
    EXPECT(pt_frame_set_shading_normals(nullptr, mine.data()) == PT_ERR_INVALID_ARGUMENT && pt_frame_get_shading_normals(nullptr, nullptr, &has) == PT_ERR_INVALID_ARGUMENT);
    EXPECT(pt_frame_set_shading_normals(frame, nullptr) == PT_OK && pt_scene_get_shading_normals(&copy, nullptr, &has) == PT_OK && has == 0);
    if (failures) return 1;
    std::printf("smooth host ok\n");
    return 0;
}
