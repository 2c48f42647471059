// Host side of the dielectric materials (include/pt_hip.h: pt_dielectric): the validation of a list, the per-material table the
// kernels read (pt_kernels.hpp: GlassRec) and the handle's setters.  A setter prepares everything -- list, table, device copies --
// before it touches a handle, so a failed call leaves every handle as it was.
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstring>

using ptc::fail;
using ptc::guarded;

namespace {

int refuse(const std::string &why) { return fail(PT_ERR_INVALID_ARGUMENT, "dielectrics: " + why); }

// The list checked against the scene's materials and turned into the table; nullptr for an empty list (removal).
int make_list(const pt_scene *scene, const pt_dielectric *list, int32_t n, std::shared_ptr<pt_glass_list> &out) {
    if (n < 0) return refuse("negative count");
    if (n > 0 && !list) return refuse("null list");
    out.reset();
    if (n == 0 || !list) return PT_OK;
    const std::vector<pt::MatRec> &mats = scene->shared->tables.mats;
    auto g = std::make_shared<pt_glass_list>();
    g->table.assign(mats.size(), pt::GlassRec{});
    for (int32_t i = 0; i < n; ++i) {
        const pt_dielectric &d = list[i];
        const std::string who = "entry " + std::to_string(i) + ": ";
        if (d.material < 0 || static_cast<size_t>(d.material) >= mats.size())
            return refuse(who + "material " + std::to_string(d.material) + " is outside the scene's " + std::to_string(mats.size()) + " materials");
        if (!std::isfinite(d.ior) || d.ior < 0.125f || d.ior > 8.0f) return refuse(who + "ior must lie in 0.125 .. 8");
        for (float t : d.tint)
            if (!std::isfinite(t) || t < 0.0f || t > 1.0f) return refuse(who + "a tint component must lie in 0 .. 1");
        const pt::MatRec &m = mats[d.material];
        if ((m.n_lobes >= 1 && m.kind0 == 0) || (m.n_lobes >= 2 && m.kind1 == 0)) return refuse(who + "material " + std::to_string(d.material) + " has an emissive lobe");
        if (scene->surface.textures && scene->surface.textures->recs[d.material].w != 0) return refuse(who + "material " + std::to_string(d.material) + " is textured");
        if (scene->surface.rough && scene->surface.rough->table[d.material] != 0.0f) return refuse(who + "material " + std::to_string(d.material) + " is in the roughness list");
        pt::GlassRec &r = g->table[d.material];
        if (r.ior != 0.0f) return refuse(who + "material " + std::to_string(d.material) + " is listed twice");
        r.ior = d.ior;
        r.inv_ior = 1.0f / d.ior;
        std::memcpy(r.tint, d.tint, sizeof r.tint);
    }
    g->list.assign(list, list + n);
    out = std::move(g);
    return PT_OK;
}

// One handle or every device's copy of a frame's scene (copies of one scene: the same materials): ptc::set_on_copies.
int set_impl(pt_scene *const *scenes, size_t n_scenes, const pt_dielectric *list, int32_t n) {
    SurfaceTables made;
    std::vector<DeviceSurface> fresh(n_scenes);
    return ptc::set_on_copies(
        scenes, n_scenes,
        [&] {
            std::shared_ptr<pt_glass_list> g;
            const int rc = make_list(scenes[0], list, n, g);
            made.glass = std::move(g);
            return rc;
        },
        [&](size_t i) { return ptc::upload_surface(made, scenes[i]->shared->tables, fresh[i], scenes[i]->d_surface); },
        [&](size_t i) {
            scenes[i]->d_surface.glass = std::move(fresh[i].glass);
            scenes[i]->surface.glass = made.glass;
        });
}

int get_impl(const pt_scene *scene, pt_dielectric *list, int32_t *n) {
    if (!scene || !n) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    *n = scene->surface.glass ? static_cast<int32_t>(scene->surface.glass->list.size()) : 0;
    if (list && scene->surface.glass) std::memcpy(list, scene->surface.glass->list.data(), scene->surface.glass->list.size() * sizeof(pt_dielectric));
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_scene_set_dielectrics(pt_scene *scene, const pt_dielectric *list, int32_t n) {
    return guarded([&] { return set_impl(&scene, 1, list, n); });
}

int pt_scene_get_dielectrics(const pt_scene *scene, pt_dielectric *list, int32_t *n) {
    return guarded([&] { return get_impl(scene, list, n); });
}

int pt_frame_set_dielectrics(pt_frame *frame, const pt_dielectric *list, int32_t n) {
    return ptc::on_frame(frame, [&](pt_scene *const *sc, size_t n_sc) { return set_impl(sc, n_sc, list, n); });
}

int pt_frame_get_dielectrics(pt_frame *frame, pt_dielectric *list, int32_t *n) {
    return ptc::on_frame_root(frame, [&](const pt_scene *root) { return get_impl(root, list, n); });
}

}  // extern "C"
