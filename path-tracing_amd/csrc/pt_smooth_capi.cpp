// Host side of smooth shading (include/pt_hip.h: shading normals): the validation of a handle's shading normals, their setters and
// getters on a scene and on a frame, the normals the loader kept, the generator's entry point and the host's own interpolation.  A
// setter prepares everything -- the copy and every device's upload -- before it touches a handle, so a failed call leaves every handle
// as it was.
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstring>

#include "pt_host_math.hpp"
#include "pt_smooth_normals.hpp"

using ptc::fail;
using ptc::guarded;

namespace {

int refuse(const std::string &why) { return fail(PT_ERR_INVALID_ARGUMENT, "shading normals: " + why); }

// One handle or every device's copy of a frame's scene (copies of one scene: the same triangles).
int set_impl(pt_scene *const *scenes, size_t n_scenes, const float *n9) {
    SurfaceTables made;
    std::vector<DeviceSurface> fresh(n_scenes);
    return ptc::set_on_copies(
        scenes, n_scenes,
        [&] {
            if (!n9) return static_cast<int>(PT_OK);
            const size_t n_tri = static_cast<size_t>(scenes[0]->shared->host.n_tri());
            if (n_tri == 0) return refuse("normals for a scene without triangles");
            for (size_t k = 0; k < 9 * n_tri; ++k)
                if (!std::isfinite(n9[k])) return refuse("component " + std::to_string(k % 9) + " of triangle " + std::to_string(k / 9) + " is not finite");
            made.smooth = std::make_shared<const std::vector<float>>(n9, n9 + 9 * n_tri);
            return static_cast<int>(PT_OK);
        },
        [&](size_t i) { return ptc::upload_surface(made, scenes[i]->shared->tables, fresh[i], scenes[i]->d_surface); },
        [&](size_t i) {
            scenes[i]->d_surface.normals = std::move(fresh[i].normals);
            scenes[i]->surface.smooth = made.smooth;
        });
}

int get_impl(const pt_scene *scene, float *n9, int32_t *has) {
    if (!scene || !has) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    *has = scene->surface.smooth ? 1 : 0;
    if (n9 && scene->surface.smooth) std::memcpy(n9, scene->surface.smooth->data(), scene->surface.smooth->size() * sizeof(float));
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_scene_set_shading_normals(pt_scene *scene, const float *n9) {
    return guarded([&] { return set_impl(&scene, 1, n9); });
}

int pt_scene_get_shading_normals(const pt_scene *scene, float *n9, int32_t *has) {
    return guarded([&] { return get_impl(scene, n9, has); });
}

int pt_frame_set_shading_normals(pt_frame *frame, const float *n9) {
    return ptc::on_frame(frame, [&](pt_scene *const *sc, size_t n_sc) { return set_impl(sc, n_sc, n9); });
}

int pt_frame_get_shading_normals(pt_frame *frame, float *n9, int32_t *has) {
    return ptc::on_frame_root(frame, [&](const pt_scene *root) { return get_impl(root, n9, has); });
}

int pt_scene_get_vertex_normals(const pt_scene *scene, float *n9, int32_t *has) {
    return guarded([&] {
        if (!scene || !has) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
        const std::vector<float> &vn = scene->shared->host.tri_vn;
        *has = vn.empty() ? 0 : 1;
        if (n9 && !vn.empty()) std::memcpy(n9, vn.data(), vn.size() * sizeof(float));
        return static_cast<int>(PT_OK);
    });
}

int pt_smooth_normals(int32_t n_tri, const float *vertices, float crease_degrees, float *out) {
    return guarded([&] {
        if (n_tri < 0 || (n_tri > 0 && (!vertices || !out))) return refuse("null argument or negative count");
        if (!(crease_degrees >= 0.0f && crease_degrees <= 180.0f)) return refuse("the crease angle must lie in 0 .. 180 degrees");
        if (n_tri > 0) pt::smooth_normals(n_tri, vertices, static_cast<double>(crease_degrees), out);
        return static_cast<int>(PT_OK);
    });
}

int pt_shading_normal_at(const float *vertices, const float *plane_normal, const float *normals, int32_t n, const float *points, float *out,
                         int32_t *interpolated) {
    return guarded([&] {
        if (!vertices || !plane_normal || !normals || n < 0 || (n > 0 && (!points || !out))) return refuse("null argument or negative count");
        const pt::TexBary r = pt::tex_bary_record(vertices, vertices + 3, vertices + 6);
        for (int32_t i = 0; i < n; ++i) {
            float b1, b2;
            pt::tex_barycentrics_record(r.a1[0], r.a1[1], r.a1[2], r.c1, r.a2[0], r.a2[1], r.a2[2], r.c2, points[3 * i], points[3 * i + 1], points[3 * i + 2], b1, b2);
            const bool own = pt::smooth_normal(normals[0], normals[1], normals[2], normals[3], normals[4], normals[5], normals[6], normals[7], normals[8], b1, b2,
                                               plane_normal[0], plane_normal[1], plane_normal[2],
                                               ptc::host_normalize3,
                                               out[3 * i], out[3 * i + 1], out[3 * i + 2]);
            if (interpolated) interpolated[i] = own ? 1 : 0;
        }
        return static_cast<int>(PT_OK);
    });
}

}  // extern "C"
