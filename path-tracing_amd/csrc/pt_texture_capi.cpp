// Host side of the albedo textures (include/pt_hip.h: pt_texture): the validation of texture coordinates and of a texture list, the
// per-material table and the texel pool the kernels read (pt_texture.hpp: TexRec, TexTexel), the handle's setters and getters, the
// MTL's map_Kd names, the BMP decode and the host's own lookup.  A setter prepares everything -- list, table, device copies -- before
// it touches a handle, so a failed call leaves every handle as it was.
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstring>

#include "pt_bmp.hpp"

using ptc::fail;
using ptc::guarded;

namespace {

int refuse(const std::string &why) { return fail(PT_ERR_INVALID_ARGUMENT, "textures: " + why); }

// The list checked against the scene's materials and the handle's dielectrics and turned into table and pool; nullptr for an empty list.
int make_list(const pt_scene *scene, const pt_texture *list, int32_t n, std::shared_ptr<pt_texture_list> &out) {
    if (n < 0) return refuse("negative count");
    if (n > 0 && !list) return refuse("null list");
    out.reset();
    if (n == 0 || !list) return PT_OK;
    if (!scene->surface.texcoords) return refuse("the scene handle has no texture coordinates");
    const std::vector<pt::MatRec> &mats = scene->shared->tables.mats;
    auto t = std::make_shared<pt_texture_list>();
    t->recs.assign(mats.size(), pt::TexRec{0, 0, 0, 0});
    uint64_t total = 0;
    for (int32_t i = 0; i < n; ++i) {
        const pt_texture &e = list[i];
        const std::string who = "entry " + std::to_string(i) + ": ";
        if (e.material < 0 || static_cast<size_t>(e.material) >= mats.size())
            return refuse(who + "material " + std::to_string(e.material) + " is outside the scene's " + std::to_string(mats.size()) + " materials");
        if (e.width < 1 || e.height < 1 || e.width > pt::kTexMaxSide || e.height > pt::kTexMaxSide)
            return refuse(who + "width and height must lie in 1 .. " + std::to_string(pt::kTexMaxSide));
        if (e.filter != pt::kTexNearest && e.filter != pt::kTexBilinear) return refuse(who + "unknown filter " + std::to_string(e.filter));
        if (!e.rgb) return refuse(who + "null texels");
        if (t->recs[e.material].w != 0) return refuse(who + "material " + std::to_string(e.material) + " is listed twice");
        if (scene->surface.glass && scene->surface.glass->table[e.material].ior != 0.0f)
            return refuse(who + "material " + std::to_string(e.material) + " is a dielectric");
        if (scene->surface.direct && ptc::material_is_light(mats[e.material]))
            return refuse(who + "material " + std::to_string(e.material) + " is a light of the handle's direct lighting");
        if (scene->surface.envdirect && ptc::material_is_light(mats[e.material]))
            return refuse(who + "material " + std::to_string(e.material) + " is a light of the handle's environment sampling");
        const uint64_t texels = static_cast<uint64_t>(e.width) * static_cast<uint64_t>(e.height);
        if (total + texels > pt::kTexMaxTexels) return refuse(who + "the list holds more than 2^28 texels");
        for (uint64_t k = 0; k < 3 * texels; ++k)
            if (!std::isfinite(e.rgb[k]) || e.rgb[k] < 0.0f) return refuse(who + "a texel is not finite or is negative");
        t->recs[e.material] = pt::TexRec{static_cast<uint32_t>(total), e.width, e.height, e.filter};
        total += texels;
    }
    t->pool.reserve(total);
    t->list.reserve(n);
    for (int32_t i = 0; i < n; ++i) {
        const pt_texture &e = list[i];
        const size_t texels = static_cast<size_t>(e.width) * static_cast<size_t>(e.height);
        t->list.push_back({e.material, e.width, e.height, e.filter, std::vector<float>(e.rgb, e.rgb + 3 * texels)});
        for (size_t k = 0; k < texels; ++k) t->pool.push_back({e.rgb[3 * k], e.rgb[3 * k + 1], e.rgb[3 * k + 2], 0.0f});
    }
    out = std::move(t);
    return PT_OK;
}

// One handle or every device's copy of a frame's scene (copies of one scene: the same materials and triangles): ptc::set_on_copies.
// set_uv: the handles get the coordinates `uv` (nullptr: none) and keep their list; otherwise they get the list and keep their coordinates.
int set_impl(pt_scene *const *scenes, size_t n_scenes, bool set_uv, const float *uv, const pt_texture *list, int32_t n) {
    SurfaceTables made;
    std::vector<DeviceSurface> fresh(n_scenes);
    return ptc::set_on_copies(
        scenes, n_scenes,
        [&] {
            made.textures = scenes[0]->surface.textures;
            made.texcoords = scenes[0]->surface.texcoords;
            if (set_uv) {
                const size_t n_tri = static_cast<size_t>(scenes[0]->shared->host.n_tri());
                if (uv && n_tri == 0) return refuse("texture coordinates for a scene without triangles");
                made.texcoords = uv ? std::make_shared<const std::vector<float>>(uv, uv + 6 * n_tri) : nullptr;
            } else {
                std::shared_ptr<pt_texture_list> t;
                const int rc = make_list(scenes[0], list, n, t);
                if (rc != PT_OK) return rc;
                made.textures = std::move(t);
            }
            if (made.textures && !made.texcoords) return refuse("the texture coordinates cannot be cleared while a texture list is set");
            return static_cast<int>(PT_OK);
        },
        [&](size_t i) { return ptc::upload_surface(made, scenes[i]->shared->tables, fresh[i], scenes[i]->d_surface); },
        [&](size_t i) {
            DeviceSurface &d = scenes[i]->d_surface;
            d.tex_recs = std::move(fresh[i].tex_recs);
            d.tex_uv = std::move(fresh[i].tex_uv);
            d.tex_texels = std::move(fresh[i].tex_texels);
            scenes[i]->surface.textures = made.textures;
            scenes[i]->surface.texcoords = made.texcoords;
        });
}

int get_texcoords_impl(const pt_scene *scene, float *uv, int32_t *has) {
    if (!scene || !has) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    *has = scene->surface.texcoords ? 1 : 0;
    if (uv && scene->surface.texcoords) std::memcpy(uv, scene->surface.texcoords->data(), scene->surface.texcoords->size() * sizeof(float));
    return PT_OK;
}

int get_textures_impl(const pt_scene *scene, pt_texture *list, int32_t *n) {
    if (!scene || !n) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    *n = scene->surface.textures ? static_cast<int32_t>(scene->surface.textures->list.size()) : 0;
    if (list && scene->surface.textures)
        for (size_t i = 0; i < scene->surface.textures->list.size(); ++i) {
            const pt_texture_list::Entry &e = scene->surface.textures->list[i];
            list[i] = pt_texture{e.material, e.width, e.height, e.filter, e.rgb.data()};
        }
    return PT_OK;
}

// pt_texture_lookup's view of caller's texels: three floats each
struct RgbTexels {
    const float *p;
    pt::TexTexel operator[](size_t i) const { return {p[3 * i], p[3 * i + 1], p[3 * i + 2], 0.0f}; }
};

}  // namespace

extern "C" {

int pt_scene_set_texcoords(pt_scene *scene, const float *uv) {
    return guarded([&] { return set_impl(&scene, 1, true, uv, nullptr, 0); });
}

int pt_scene_get_texcoords(const pt_scene *scene, float *uv, int32_t *has) {
    return guarded([&] { return get_texcoords_impl(scene, uv, has); });
}

int pt_scene_set_textures(pt_scene *scene, const pt_texture *list, int32_t n) {
    return guarded([&] { return set_impl(&scene, 1, false, nullptr, list, n); });
}

int pt_scene_get_textures(const pt_scene *scene, pt_texture *list, int32_t *n) {
    return guarded([&] { return get_textures_impl(scene, list, n); });
}

int pt_frame_set_texcoords(pt_frame *frame, const float *uv) {
    return ptc::on_frame(frame, [&](pt_scene *const *sc, size_t n_sc) { return set_impl(sc, n_sc, true, uv, nullptr, 0); });
}

int pt_frame_get_texcoords(pt_frame *frame, float *uv, int32_t *has) {
    return ptc::on_frame_root(frame, [&](const pt_scene *root) { return get_texcoords_impl(root, uv, has); });
}

int pt_frame_set_textures(pt_frame *frame, const pt_texture *list, int32_t n) {
    return ptc::on_frame(frame, [&](pt_scene *const *sc, size_t n_sc) { return set_impl(sc, n_sc, false, nullptr, list, n); });
}

int pt_frame_get_textures(pt_frame *frame, pt_texture *list, int32_t *n) {
    return ptc::on_frame_root(frame, [&](const pt_scene *root) { return get_textures_impl(root, list, n); });
}

int pt_scene_get_map_kd(const pt_scene *scene, int32_t material, const char **name) {
    return guarded([&] {
        if (!scene || !name) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
        const pt::HostScene &h = scene->shared->host;
        if (material < 0 || material >= h.n_mat()) return refuse("material " + std::to_string(material) + " is outside the scene's " + std::to_string(h.n_mat()) + " materials");
        *name = static_cast<size_t>(material) < h.map_kd.size() ? h.map_kd[material].c_str() : "";
        return static_cast<int>(PT_OK);
    });
}

int pt_scene_get_texture_records(const pt_scene *scene, float *records) {
    return guarded([&] {
        if (!scene || !records) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
        const std::vector<pt::TexBary> r = ptc::texture_bary_records(scene->shared->tables.exact);
        static_assert(sizeof(pt::TexBary) == 8 * sizeof(float), "a record is eight floats");
        if (!r.empty()) std::memcpy(records, r.data(), r.size() * sizeof(pt::TexBary));
        return static_cast<int>(PT_OK);
    });
}

int pt_texture_load_bmp(const char *path, float gamma, int32_t *width, int32_t *height, float *rgb) {
    return guarded([&] {
        if (!path || !width || !height) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
        std::vector<uint8_t> bgr;
        int w = 0, h = 0;
        std::string why;
        bool cannot_open = false;
        if (!pt::read_bmp24(path, bgr, w, h, why, cannot_open))
            return cannot_open ? fail(PT_ERR_IO, "texture: " + why) : fail(PT_ERR_PARSE, std::string("texture ") + path + ": " + why);
        if (w > pt::kTexMaxSide || h > pt::kTexMaxSide) return fail(PT_ERR_PARSE, std::string("texture ") + path + ": a side above " + std::to_string(pt::kTexMaxSide));
        *width = w;
        *height = h;
        if (!rgb) return static_cast<int>(PT_OK);
        const double g = (std::isfinite(gamma) && gamma > 0.0f) ? static_cast<double>(gamma) : 2.2;
        float table[256];
        for (int b = 0; b < 256; ++b) table[b] = static_cast<float>(g == 1.0 ? b / 255.0 : std::pow(b / 255.0, g));
        const size_t n = static_cast<size_t>(w) * static_cast<size_t>(h);
        for (size_t k = 0; k < n; ++k) {   // B, G, R bytes -> R, G, B floats
            rgb[3 * k] = table[bgr[3 * k + 2]];
            rgb[3 * k + 1] = table[bgr[3 * k + 1]];
            rgb[3 * k + 2] = table[bgr[3 * k]];
        }
        return static_cast<int>(PT_OK);
    });
}

int pt_texture_lookup(int32_t width, int32_t height, const float *rgb, int32_t filter, int32_t n, const float *uv, float *out_rgb, int32_t *indices) {
    return guarded([&] {
        if (width < 1 || height < 1 || width > pt::kTexMaxSide || height > pt::kTexMaxSide) return refuse("width and height must lie in 1 .. " + std::to_string(pt::kTexMaxSide));
        if (filter != pt::kTexNearest && filter != pt::kTexBilinear) return refuse("unknown filter " + std::to_string(filter));
        if (n < 0 || !rgb || (n > 0 && (!uv || !out_rgb))) return refuse("null argument or negative count");
        const RgbTexels texels{rgb};
        for (int32_t i = 0; i < n; ++i) {
            pt::tex_lookup(texels, width, height, filter, uv[2 * i], uv[2 * i + 1], out_rgb[3 * i], out_rgb[3 * i + 1], out_rgb[3 * i + 2]);
            if (indices) {
                const pt::TexTaps k = pt::tex_taps(width, height, filter, uv[2 * i], uv[2 * i + 1]);
                indices[4 * i] = k.i00; indices[4 * i + 1] = k.i10; indices[4 * i + 2] = k.i01; indices[4 * i + 3] = k.i11;
            }
        }
        return static_cast<int>(PT_OK);
    });
}

}  // extern "C"
