// Host side of rough specular reflection (include/pt_hip.h: rough specular): the validation of a roughness list, the per-material
// table the kernels read and the handle's setters and getters on a scene and on a frame, the Pr values the loader kept, and the host's
// own evaluation of the step.  A setter prepares everything -- list, table, device copies -- before it touches a handle, so a failed
// call leaves every handle as it was.
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstring>

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
        if (scene->glass && scene->glass->table[d.material].ior != 0.0f) return refuse(who + "material " + std::to_string(d.material) + " is a dielectric");
        if (g->table[d.material] != 0.0f) return refuse(who + "material " + std::to_string(d.material) + " is listed twice");
        g->table[d.material] = d.alpha;
    }
    g->list.assign(list, list + n);
    out = std::move(g);
    return PT_OK;
}

// One handle or every device's copy of a frame's scene (copies of one scene: the same materials).  The list is made once, every
// device's table is uploaded, and only then do the handles change.
int set_impl(pt_scene *const *scenes, size_t n_scenes, const pt_rough *list, int32_t n) {
    for (size_t i = 0; i < n_scenes; ++i)
        if (!scenes[i]) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
    std::shared_ptr<pt_rough_list> g;
    int rc = PT_OK;
    for (size_t i = 0; i < n_scenes; ++i)   // (every copy's own dielectrics: a frame's copies may have been given different ones)
        if ((rc = make_list(scenes[i], list, n, g)) != PT_OK) return rc;
    std::vector<DeviceRough> fresh(n_scenes);
    for (size_t i = 0; i < n_scenes; ++i) {
        if (scenes[i]->device < 0) continue;
        PT_HIP_TRY(hipSetDevice(scenes[i]->device));
        if (g && (rc = ptc::upload_rough(g->table, scenes[i]->shared->tables, fresh[i])) != PT_OK) return rc;
        PT_HIP_TRY(hipDeviceSynchronize());   // (a launch in flight may still read the old table)
    }
    for (size_t i = 0; i < n_scenes; ++i) {
        scenes[i]->d_rough = std::move(fresh[i]);
        scenes[i]->rough = g;
    }
    return PT_OK;
}

int get_impl(const pt_scene *scene, pt_rough *list, int32_t *n) {
    if (!scene || !n) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    *n = scene->rough ? static_cast<int32_t>(scene->rough->list.size()) : 0;
    if (list && scene->rough) std::memcpy(list, scene->rough->list.data(), scene->rough->list.size() * sizeof(pt_rough));
    return PT_OK;
}

// The kernels' portable_sincos on the host: double +, -, * only, the same constants in the same order.
void host_sincos(float a, float &s_out, float &c_out) {
    static const double t[16] = {
        0.63661977236758138, 1.57079632673412561417e+00, 6.07710050650619224932e-11, 0.5,
        -1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04, 2.75573137070700676789e-06,
        -2.50507602534068634195e-08, 1.58969099521155010221e-10,
        4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05, -2.75573143513906633035e-07,
        2.08757232129817482790e-09, -1.13596475577881948265e-11};
    const double x = static_cast<double>(a);
    const int k = static_cast<int>(x * t[0] + t[3]);
    const double kd = static_cast<double>(k);
    const double r = (x - kd * t[1]) - kd * t[2];
    const double z = r * r;
    const double ps = t[4] + z * (t[5] + z * (t[6] + z * (t[7] + z * (t[8] + z * t[9]))));
    const double sn = r + r * (z * ps);
    const double pc = t[10] + z * (t[11] + z * (t[12] + z * (t[13] + z * (t[14] + z * t[15]))));
    const double cs = (1.0 - t[3] * z) + (z * z) * pc;
    const float sf = static_cast<float>(sn), cf = static_cast<float>(cs);
    switch (static_cast<unsigned>(k) & 3u) {
        case 0: s_out = sf; c_out = cf; break;
        case 1: s_out = cf; c_out = -sf; break;
        case 2: s_out = -sf; c_out = -cf; break;
        default: s_out = -cf; c_out = sf; break;
    }
}

float host_unit_float(uint32_t w) { return static_cast<float>(((w >> 9) << 1) | 1u) * 5.9604644775390625e-08f; }

}  // namespace

extern "C" {

int pt_scene_set_roughness(pt_scene *scene, const pt_rough *list, int32_t n) {
    return guarded([&] { return set_impl(&scene, 1, list, n); });
}

int pt_scene_get_roughness(const pt_scene *scene, pt_rough *list, int32_t *n) {
    return guarded([&] { return get_impl(scene, list, n); });
}

int pt_frame_set_roughness(pt_frame *frame, const pt_rough *list, int32_t n) {
    return guarded([&] {
        if (!frame) return fail(PT_ERR_INVALID_ARGUMENT, "null frame");
        const auto &sc = ptc::frame_scenes(frame);
        return set_impl(sc.data(), sc.size(), list, n);
    });
}

int pt_frame_get_roughness(pt_frame *frame, pt_rough *list, int32_t *n) {
    return guarded([&] {
        if (!frame) return fail(PT_ERR_INVALID_ARGUMENT, "null frame");
        return get_impl(ptc::frame_scenes(frame)[0], list, n);
    });
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
                           host_unit_float(w1[i]), host_unit_float(w2[i]), host_sincos,
                           [](float &x, float &y, float &z) {
                               const float inv = 1.0f / std::sqrt((x * x + y * y) + z * z);
                               x = x * inv; y = y * inv; z = z * inv;
                           },
                           out_directions[3 * i], out_directions[3 * i + 1], out_directions[3 * i + 2], out_g1[i], h[0], h[1], h[2]);
            if (out_microfacet) std::memcpy(out_microfacet + 3 * i, h, sizeof h);
        }
        return static_cast<int>(PT_OK);
    });
}

}  // extern "C"
