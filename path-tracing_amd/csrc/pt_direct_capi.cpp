// Host side of direct lighting (include/pt_hip.h: direct lighting): the light table of a scene, the switch on a scene and on a frame,
// the table's getter, and the host's own evaluation of the direct term.  A setter prepares everything -- table, device copies -- before
// it touches a handle, so a failed call leaves every handle as it was.
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstring>

#include "pt_host_math.hpp"

using ptc::fail;
using ptc::guarded;

namespace {

int refuse(const std::string &why) { return fail(PT_ERR_INVALID_ARGUMENT, "direct lighting: " + why); }

static_assert(sizeof(pt_light) == sizeof(pt::LightRec), "pt_light is the table's record");

// The table of a scene (pt_hip.h: THE LIGHT TABLE): the triangles of non-zero area whose material is the single emissive lobe, in the
// original order; areas in double from the float edges, summed in double in table order.
std::shared_ptr<pt_light_table> build_table(const pt::DeviceTables &tables) {
    auto t = std::make_shared<pt_light_table>();
    std::vector<double> areas;
    for (size_t i = 0; i < tables.exact.size(); ++i) {
        const pt::ExactRec &r = tables.exact[i];
        if (r.material < 0 || static_cast<size_t>(r.material) >= tables.mats.size()) continue;
        const pt::MatRec &m = tables.mats[r.material];
        if (!ptc::material_is_light(m)) continue;
        pt::LightRec l{};
        for (int c = 0; c < 3; ++c) {
            l.v0[c] = r.v0[c];
            l.e1[c] = r.v1[c] - r.v0[c];
            l.e2[c] = r.v2[c] - r.v0[c];
            l.nl[c] = r.plane[c];
            l.le[c] = m.kd[c];
        }
        const double ax = l.e1[0], ay = l.e1[1], az = l.e1[2], bx = l.e2[0], by = l.e2[1], bz = l.e2[2];
        const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        const double area = 0.5 * std::sqrt((cx * cx + cy * cy) + cz * cz);
        if (!(area > 0.0) || !std::isfinite(area)) continue;
        l.orig = static_cast<int32_t>(i);
        t->lights.push_back(l);
        areas.push_back(area);
    }
    double total = 0.0;
    for (double a : areas) total += a;
    double cum = 0.0;
    for (size_t i = 0; i < areas.size(); ++i) {
        cum += areas[i];
        t->lights[i].cdf = static_cast<float>(cum / total);
    }
    if (!t->lights.empty()) t->lights.back().cdf = 1.0f;
    t->area = static_cast<float>(total);
    return t;
}

// One handle or every device's copy of a frame's scene (copies of one scene: the same triangles and materials).
int set_impl(pt_scene *const *scenes, size_t n_scenes, int32_t on) {
    SurfaceTables made;
    std::vector<DeviceSurface> fresh(n_scenes);
    return ptc::set_on_copies(
        scenes, n_scenes,
        [&] {
            if (!on) {   // (roulette needs per-path accounting: the last of the two switches that give it stays while roulette is on)
                for (size_t i = 0; i < n_scenes; ++i)
                    if (scenes[i]->surface.rr_start > 0 && scenes[i]->surface.direct && !scenes[i]->surface.envdirect)
                        return refuse("the scene handle has Russian roulette set and no environment sampling; clear the roulette first");
                return static_cast<int>(PT_OK);
            }
            const std::shared_ptr<pt_light_table> t = build_table(scenes[0]->shared->tables);
            if (t->lights.empty() || !(t->area > 0.0f) || !std::isfinite(t->area)) return refuse("the scene has no light (a triangle of non-zero area whose material is the emissive lobe alone)");
            const std::vector<pt::MatRec> &mats = scenes[0]->shared->tables.mats;
            for (size_t i = 0; i < n_scenes; ++i) {   // (every copy's own textures: a frame's copies may have been given different ones)
                if (!scenes[i]->surface.textures) continue;
                for (size_t m = 0; m < mats.size(); ++m)
                    if (ptc::material_is_light(mats[m]) && scenes[i]->surface.textures->recs[m].w != 0)
                        return refuse("emissive material " + std::to_string(m) + " is in the texture list");
            }
            made.direct = t;
            return static_cast<int>(PT_OK);
        },
        [&](size_t i) { return ptc::upload_surface(made, scenes[i]->shared->tables, fresh[i], scenes[i]->d_surface); },
        [&](size_t i) {
            scenes[i]->d_surface.lights = std::move(fresh[i].lights);
            scenes[i]->surface.direct = made.direct;
        });
}

int get_impl(const pt_scene *scene, int32_t *on) {
    if (!scene || !on) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    *on = scene->surface.direct ? 1 : 0;
    return PT_OK;
}

int lights_impl(const pt_scene *scene, pt_light *lights, int32_t *n, float *area) {
    if (!scene || !n) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_ptr<const pt_light_table> t = scene->surface.direct;
    if (!t) t = build_table(scene->shared->tables);   // (what the switch would build)
    *n = static_cast<int32_t>(t->lights.size());
    if (area) *area = t->area;
    if (lights && !t->lights.empty()) std::memcpy(lights, t->lights.data(), t->lights.size() * sizeof(pt_light));
    return PT_OK;
}

}  // namespace

std::shared_ptr<pt_light_table> ptc::light_table_of(const pt::DeviceTables &tables) { return build_table(tables); }

extern "C" {

int pt_scene_set_direct_lighting(pt_scene *scene, int32_t on) {
    return guarded([&] { return set_impl(&scene, 1, on); });
}

int pt_scene_get_direct_lighting(const pt_scene *scene, int32_t *on) {
    return guarded([&] { return get_impl(scene, on); });
}

int pt_scene_get_lights(const pt_scene *scene, pt_light *lights, int32_t *n, float *area) {
    return guarded([&] { return lights_impl(scene, lights, n, area); });
}

int pt_frame_set_direct_lighting(pt_frame *frame, int32_t on) {
    return ptc::on_frame(frame, [&](pt_scene *const *sc, size_t n_sc) { return set_impl(sc, n_sc, on); });
}

int pt_frame_get_direct_lighting(pt_frame *frame, int32_t *on) {
    return ptc::on_frame_root(frame, [&](const pt_scene *root) { return get_impl(root, on); });
}

int pt_frame_get_lights(pt_frame *frame, pt_light *lights, int32_t *n, float *area) {
    return ptc::on_frame_root(frame, [&](const pt_scene *root) { return lights_impl(root, lights, n, area); });
}

int pt_direct_term(int32_t n, const pt_light *lights, int32_t n_lights, float area, const float *origins, const float *normals,
                   const float *shading_normals, const float *throughput, const float *kd, const uint32_t *l0, const uint32_t *l1,
                   const uint32_t *l2, int32_t *out_light, float *out_points, float *out_directions, float *out_terms, int32_t *out_has_term) {
    return guarded([&] {
        if (n < 0 || n_lights < 1 || !lights) return refuse("a negative count or no light table");
        if (n > 0 && (!origins || !normals || !shading_normals || !throughput || !kd || !l0 || !l1 || !l2 || !out_light || !out_points ||
                      !out_directions || !out_terms || !out_has_term))
            return refuse("null argument");
        const pt::LightRec *table = reinterpret_cast<const pt::LightRec *>(lights);
        for (int32_t i = 0; i < n; ++i) {
            const int32_t li = pt::direct_pick(table, n_lights, ptc::host_unit_float(l0[i]));
            const float *o = origins + 3 * i, *N = normals + 3 * i, *s = shading_normals + 3 * i, *t = throughput + 3 * i, *k = kd + 3 * i;
            float *p = out_points + 3 * i, *w = out_directions + 3 * i, *c = out_terms + 3 * i;
            const bool has = pt::direct_term(table[li], area, ptc::host_unit_float(l1[i]), ptc::host_unit_float(l2[i]), o[0], o[1], o[2], N[0], N[1], N[2], s[0], s[1],
                                             s[2], t[0], t[1], t[2], k[0], k[1], k[2],
                                             ptc::host_normalize3,
                                             p[0], p[1], p[2], w[0], w[1], w[2], c[0], c[1], c[2]);
            out_light[i] = li;
            out_has_term[i] = has ? 1 : 0;
        }
        return static_cast<int>(PT_OK);
    });
}

}  // extern "C"
