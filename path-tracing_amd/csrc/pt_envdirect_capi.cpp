// Host side of environment sampling (include/pt_hip.h: environment sampling): the alias table of a handle's environment and the share,
// the switch on a scene and on a frame, the table's getter, and the host's own evaluation of the sample and the term.  (The rebuild
// when a switched-on handle's environment is replaced is pt_capi_internal.hpp's envdirect_prepare / envdirect_commit, inline there so
// that the environment's translation unit needs no other.)  A setter prepares everything -- table, device copies -- before it touches a
// handle, so a failed call leaves every handle as it was.
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstring>

#include "pt_host_math.hpp"

using ptc::fail;
using ptc::guarded;

namespace {

int refuse(const std::string &why) { return fail(PT_ERR_INVALID_ARGUMENT, "environment sampling: " + why); }

static_assert(sizeof(pt_env_sample_record) == sizeof(pt::EnvAliasRec), "pt_env_sample_record is the table's record");

// The rule of direct lighting: no emissive material in any copy's texture list.
int check_textures(pt_scene *const *scenes, size_t n_scenes) {
    const std::vector<pt::MatRec> &mats = scenes[0]->shared->tables.mats;
    for (size_t i = 0; i < n_scenes; ++i) {
        if (!scenes[i]->surface.textures) continue;
        for (size_t m = 0; m < mats.size(); ++m)
            if (ptc::material_is_light(mats[m]) && scenes[i]->surface.textures->recs[m].w != 0)
                return refuse("emissive material " + std::to_string(m) + " is in the texture list");
    }
    return PT_OK;
}

// One handle or every device's copy of a frame's scene (copies of one scene: the same triangles, materials and environment).
int set_impl(pt_scene *const *scenes, size_t n_scenes, const pt_env_sampling *params) {
    SurfaceTables made;
    std::vector<DeviceSurface> fresh(n_scenes);
    return ptc::set_on_copies(
        scenes, n_scenes,
        [&] {
            if (!params) {   // (roulette needs per-path accounting: the last of the two switches that give it stays while roulette is on)
                for (size_t i = 0; i < n_scenes; ++i)
                    if (scenes[i]->surface.rr_start > 0 && scenes[i]->surface.envdirect && !scenes[i]->surface.direct)
                        return refuse("the scene handle has Russian roulette set and no direct lighting; clear the roulette first");
                return static_cast<int>(PT_OK);
            }
            for (size_t i = 0; i < n_scenes; ++i)
                if (!scenes[i]->env) return refuse("the scene handle has no environment (pt_scene_set_environment_*)");
            if (!std::isfinite(params->share)) return refuse("the share is not finite");
            int rc = check_textures(scenes, n_scenes);
            if (rc != PT_OK) return rc;
            return ptc::envdirect_sampler(*scenes[0]->env, ptc::light_table_of(scenes[0]->shared->tables), *params, made.envdirect);
        },
        [&](size_t i) { return ptc::upload_surface(made, scenes[i]->shared->tables, fresh[i], scenes[i]->d_surface); },
        [&](size_t i) {
            scenes[i]->d_surface.env_alias = std::move(fresh[i].env_alias);
            scenes[i]->d_surface.env_lights = std::move(fresh[i].env_lights);
            scenes[i]->surface.envdirect = made.envdirect;
        });
}

int get_impl(const pt_scene *scene, int32_t *on, pt_env_sampling *params) {
    if (!scene || !on) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    *on = scene->surface.envdirect ? 1 : 0;
    if (params) *params = scene->surface.envdirect ? scene->surface.envdirect->given : pt_env_sampling{};
    return PT_OK;
}

int table_impl(const pt_scene *scene, pt_env_sample_record *records, int32_t *cells, float *share) {
    if (!scene || !cells) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_ptr<const pt_env_sampler> t = scene->surface.envdirect;
    if (!t) {   // (what the switch would build)
        if (!scene->env) {
            *cells = 0;
            if (share) *share = 0.0f;
            return PT_OK;
        }
        const int rc = ptc::envdirect_sampler(*scene->env, ptc::light_table_of(scene->shared->tables), pt_env_sampling{}, t);
        if (rc != PT_OK) return rc;
    }
    *cells = t->cells;
    if (share) *share = t->share;
    if (records) std::memcpy(records, t->records.data(), t->records.size() * sizeof(pt_env_sample_record));
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_scene_set_environment_sampling(pt_scene *scene, const pt_env_sampling *params) {
    return guarded([&] { return set_impl(&scene, 1, params); });
}

int pt_scene_get_environment_sampling(const pt_scene *scene, int32_t *on, pt_env_sampling *params) {
    return guarded([&] { return get_impl(scene, on, params); });
}

int pt_scene_get_environment_sampling_table(const pt_scene *scene, pt_env_sample_record *records, int32_t *cells, float *share) {
    return guarded([&] { return table_impl(scene, records, cells, share); });
}

int pt_frame_set_environment_sampling(pt_frame *frame, const pt_env_sampling *params) {
    return ptc::on_frame(frame, [&](pt_scene *const *sc, size_t n_sc) { return set_impl(sc, n_sc, params); });
}

int pt_frame_get_environment_sampling(pt_frame *frame, int32_t *on, pt_env_sampling *params) {
    return ptc::on_frame_root(frame, [&](const pt_scene *root) { return get_impl(root, on, params); });
}

int pt_frame_get_environment_sampling_table(pt_frame *frame, pt_env_sample_record *records, int32_t *cells, float *share) {
    return ptc::on_frame_root(frame, [&](const pt_scene *root) { return table_impl(root, records, cells, share); });
}

int pt_envdirect_term(int32_t n, const pt_env_sample_record *records, int32_t cells, float share, int32_t map_n, const float *map_rgb,
                      const float *normals, const float *shading_normals, const float *throughput, const float *kd, const uint32_t *e0,
                      const uint32_t *e1, const uint32_t *e2, const uint32_t *e3, int32_t *out_cell, float *out_directions, float *out_pdf,
                      float *out_terms, int32_t *out_has_term) {
    return guarded([&] {
        if (n < 0 || !records || !map_rgb || cells < 1 || cells > pt::kEnvSampleMaxCells) return refuse("a negative count, no table or no map");
        if (map_n < pt::kEnvMinSize || map_n > pt::kEnvMaxSize) return refuse("the map's size must lie in 8 .. 4096");
        if (n > 0 && (!normals || !shading_normals || !throughput || !kd || !e0 || !e1 || !e2 || !e3 || !out_cell || !out_directions || !out_pdf ||
                      !out_terms || !out_has_term))
            return refuse("null argument");
        const pt::EnvAliasRec *table = reinterpret_cast<const pt::EnvAliasRec *>(records);
        const int32_t n_cells = cells * cells;
        for (int32_t c = 0; c < n_cells; ++c)
            if (table[c].alias < 0 || table[c].alias >= n_cells) return refuse("a record's alias is not a cell of the table");
        const std::vector<pt::EnvTexel> texels = pt::env_with_apron(map_n, map_rgb);
        for (int32_t i = 0; i < n; ++i) {
            const float *N = normals + 3 * i, *s = shading_normals + 3 * i, *t = throughput + 3 * i, *k = kd + 3 * i;
            float *w = out_directions + 3 * i, *c = out_terms + 3 * i;
            pt::envdirect_sample(table, cells, e0[i], ptc::host_unit_float(e1[i]), ptc::host_unit_float(e2[i]), ptc::host_unit_float(e3[i]),
                                 ptc::host_normalize3, [](float v) { return std::sqrt(v); }, out_cell[i], w[0], w[1], w[2], out_pdf[i]);
            float lr, lg, lb;
            pt::env_lookup(texels.data(), map_n, w[0], w[1], w[2], lr, lg, lb);
            out_has_term[i] = pt::envdirect_term(w[0], w[1], w[2], out_pdf[i], share, lr, lg, lb, N[0], N[1], N[2], s[0], s[1], s[2], t[0], t[1], t[2],
                                                 k[0], k[1], k[2], c[0], c[1], c[2])
                                  ? 1
                                  : 0;
        }
        return static_cast<int>(PT_OK);
    });
}

}  // extern "C"
