// Host side of rough specular reflection (include/pt_hip.h: rough specular): the validation of a roughness list, the per-material
// table the kernels read and the handle's setters and getters on a scene and on a frame, the Pr values the loader kept, and the host's
// own evaluation of the step.  A setter prepares everything -- list, table, device copies -- before it touches a handle, so a failed
// call leaves every handle as it was.
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstring>

#include "pt_host_math.hpp"

using ptc::fail;
using ptc::guarded;

namespace {

int refuse(const std::string &why) { return fail(PT_ERR_INVALID_ARGUMENT, "roughness: " + why); }

// The list checked against the scene's materials and turned into the table; nullptr for an empty list (removal).
int make_list(const pt_scene *scene, const pt_rough *list, int32_t n, std::shared_ptr<pt_rough_list> &out) {
    if (n < 0) return refuse("negative count");
    if (n > 0 && !list) return refuse("null list");
    out.reset();
    if (n == 0 || !list) return PT_OK;
    const std::vector<pt::MatRec> &mats = scene->shared->tables.mats;
    auto g = std::make_shared<pt_rough_list>();
    g->table.assign(mats.size(), 0.0f);
    for (int32_t i = 0; i < n; ++i) {
        const pt_rough &d = list[i];
        const std::string who = "entry " + std::to_string(i) + ": ";
        if (d.material < 0 || static_cast<size_t>(d.material) >= mats.size())
            return refuse(who + "material " + std::to_string(d.material) + " is outside the scene's " + std::to_string(mats.size()) + " materials");
        if (!std::isfinite(d.alpha) || d.alpha < PT_ROUGH_ALPHA_MIN || d.alpha > PT_ROUGH_ALPHA_MAX) return refuse(who + "alpha must lie in 2^-10 .. 1");
        const pt::MatRec &m = mats[d.material];
        if (!(m.n_lobes >= 1 && m.kind0 == 1)) return refuse(who + "material " + std::to_string(d.material) + " has no glossy lobe");
        if (scene->surface.glass && scene->surface.glass->table[d.material].ior != 0.0f) return refuse(who + "material " + std::to_string(d.material) + " is a dielectric");
        if (g->table[d.material] != 0.0f) return refuse(who + "material " + std::to_string(d.material) + " is listed twice");
        g->table[d.material] = d.alpha;
    }
    g->list.assign(list, list + n);
    out = std::move(g);
    return PT_OK;
}

// One handle or every device's copy of a frame's scene (copies of one scene: the same materials): ptc::set_on_copies.
int set_impl(pt_scene *const *scenes, size_t n_scenes, const pt_rough *list, int32_t n) {
    SurfaceTables made;
    std::vector<DeviceSurface> fresh(n_scenes);
    return ptc::set_on_copies(
        scenes, n_scenes,
        [&] {
            std::shared_ptr<pt_rough_list> g;
            int rc = PT_OK;
            for (size_t i = 0; i < n_scenes && rc == PT_OK; ++i) rc = make_list(scenes[i], list, n, g);   // (every copy's own dielectrics: a frame's copies may have been given different ones)
            made.rough = std::move(g);
            return rc;
        },
        [&](size_t i) { return ptc::upload_surface(made, scenes[i]->shared->tables, fresh[i], scenes[i]->d_surface); },
        [&](size_t i) {
            scenes[i]->d_surface.alpha = std::move(fresh[i].alpha);
            scenes[i]->surface.rough = made.rough;
        });
}

int get_impl(const pt_scene *scene, pt_rough *list, int32_t *n) {
    if (!scene || !n) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    *n = scene->surface.rough ? static_cast<int32_t>(scene->surface.rough->list.size()) : 0;
    if (list && scene->surface.rough) std::memcpy(list, scene->surface.rough->list.data(), scene->surface.rough->list.size() * sizeof(pt_rough));
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_scene_set_roughness(pt_scene *scene, const pt_rough *list, int32_t n) {
    return guarded([&] { return set_impl(&scene, 1, list, n); });
}

int pt_scene_get_roughness(const pt_scene *scene, pt_rough *list, int32_t *n) {
    return guarded([&] { return get_impl(scene, list, n); });
}

int pt_frame_set_roughness(pt_frame *frame, const pt_rough *list, int32_t n) {
    return ptc::on_frame(frame, [&](pt_scene *const *sc, size_t n_sc) { return set_impl(sc, n_sc, list, n); });
}

int pt_frame_get_roughness(pt_frame *frame, pt_rough *list, int32_t *n) {
    return ptc::on_frame_root(frame, [&](const pt_scene *root) { return get_impl(root, list, n); });
}

int pt_scene_get_mtl_roughness(const pt_scene *scene, float *pr) {
    return guarded([&] {
        if (!scene || !pr) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
        const pt::HostScene &h = scene->shared->host;
        for (int m = 0; m < h.n_mat(); ++m) pr[m] = static_cast<size_t>(m) < h.mat_pr.size() ? h.mat_pr[m] : -1.0f;
        return static_cast<int>(PT_OK);
    });
}

int pt_rough_step(int32_t n, const float *normals, const float *directions, const float *alpha, const uint32_t *w1, const uint32_t *w2,
                  float *out_directions, float *out_g1, float *out_microfacet) {
    return guarded([&] {
        if (n < 0 || (n > 0 && (!normals || !directions || !alpha || !w1 || !w2 || !out_directions || !out_g1))) return refuse("null argument or negative count");
        for (int32_t i = 0; i < n; ++i)
            if (!(alpha[i] >= PT_ROUGH_ALPHA_MIN && alpha[i] <= PT_ROUGH_ALPHA_MAX)) return refuse("alpha " + std::to_string(i) + " must lie in 2^-10 .. 1");
        for (int32_t i = 0; i < n; ++i) {
            float h[3];
            pt::rough_step(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], directions[3 * i], directions[3 * i + 1], directions[3 * i + 2], alpha[i],
                           ptc::host_unit_float(w1[i]), ptc::host_unit_float(w2[i]), ptc::host_sincos, ptc::host_normalize3,
                           out_directions[3 * i], out_directions[3 * i + 1], out_directions[3 * i + 2], out_g1[i], h[0], h[1], h[2]);
            if (out_microfacet) std::memcpy(out_microfacet + 3 * i, h, sizeof h);
        }
        return static_cast<int>(PT_OK);
    });
}

}  // extern "C"
