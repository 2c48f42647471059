// C ABI of libpt_hip.so (include/pt_hip.h).  Host side only: owns the device copies of the scene tables, maps HIP
// errors to status codes, and implements the reference's host-side resolve and BMP writer.  (pt_frame.cpp holds the
// multi-device frame on top of what is here.)
#include "pt_capi_internal.hpp"
#include "pt_bmp.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "pt_filters.hpp"

// Overrides of the launch plan: set by pt_test_set_mutation in the test builds, never in the product (which has no such entry point).
static pt::plan::Overrides g_plan_overrides;
// plan::variant_id of the kernel the last enqueued launch took (-1: none yet); the test builds export it as pt_test_last_variant.
static std::atomic<int> g_last_variant{-1};

namespace ptc {

thread_local std::string g_error;

int fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}
int hip_fail(hipError_t e, const char *what) {
    const int code = (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver)
                         ? PT_ERR_NO_DEVICE
                         : (e == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_HIP);
    return fail(code, std::string(what) + ": " + hipGetErrorString(e));
}

std::atomic<long> g_live_device_objects{0};

int use_device(int device, const char *stage) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n)
        return fail(PT_ERR_NO_DEVICE, std::string(stage) + ": device " + std::to_string(device) + " is not a visible HIP device (there is no CPU fallback)");
    PT_HIP_TRY(hipSetDevice(device));
    return PT_OK;
}

}  // namespace ptc

using ptc::fail;
using ptc::guarded;
using ptc::hip_fail;

namespace {

// The layouts the kernels read pack indices into bit fields; a hierarchy that does not fit them must be refused, never
// truncated: (ray, slot) pairs keep the slot in 24 bits (pt_kernels.hip: `e & 0xFFFFFF`), a box-tree node keeps its child
// base in 20 bits (BvhNode::meta, `base << 12`: a child node, or a leaf's first slot / 8 -- fewer leaves than nodes; stack entries have 26), a sphere tree has at most kMaxLevels levels.
int check_table_limits(unsigned long long n_slots, unsigned long long n_bvh_nodes, long long n_levels, long long bvh_depth = 0) {
    if (n_slots >= (1ull << 24))
        return fail(PT_ERR_UNSUPPORTED, "the culling hierarchy has " + std::to_string(n_slots) + " slots; (ray, slot) work items hold 24 bits");
    if (n_bvh_nodes >= (1ull << 20))
        return fail(PT_ERR_UNSUPPORTED, "the box tree has " + std::to_string(n_bvh_nodes) + " nodes; a node's child base holds 20 bits");
    // a leaf's base is its first slot / 8 in the global slot order: with a box tree the slots themselves must stay below 2^23
    // (the builder puts the tree's slots first, so a leaf's base is below the node count anyway: this is the field's own bound)
    if (n_bvh_nodes > 0 && n_slots >= (1ull << 23))
        return fail(PT_ERR_UNSUPPORTED, "the culling hierarchy has " + std::to_string(n_slots) + " slots under a box tree; a leaf's base (first slot / 8) holds 20 bits");
    if (bvh_depth > pt::kMaxBvhDepth)
        return fail(PT_ERR_UNSUPPORTED, "the box tree has " + std::to_string(bvh_depth) + " levels; the walk's stack slack holds " + std::to_string(pt::kMaxBvhDepth));
    if (n_levels > pt::kMaxLevels)
        return fail(PT_ERR_UNSUPPORTED, "a sphere tree has " + std::to_string(n_levels) + " levels; the walk holds " + std::to_string(pt::kMaxLevels));
    return PT_OK;
}

// The culling hierarchy of a scene for one eps: built once per (scene, eps) on the host, whatever number of devices,
// sessions or diagnostic calls ask for it.  (The test-hook build rebuilds every time: its mutations change the result.)
// Keyed on (eps, envelope radius): a camera whose origin lies inside the camera-free envelope shares its tables.
// r_camera: largest |component| of the camera origin (20 = the reference's fixed camera).
int get_cull(pt_scene_host &h, float eps, double r_camera, std::shared_ptr<const pt::CullTables> &out) {
    std::lock_guard<std::mutex> lock(h.cull_mutex);
#ifndef PT_TEST_HOOKS
    const double r_max = pt::cull_r_max(h.vertex_extent, r_camera);
    for (const auto &t : h.cull_cache)
        if (std::memcmp(&t->eps, &eps, sizeof eps) == 0 && t->r_max == r_max) {
            out = t;
            return PT_OK;
        }
#endif
    const auto t0 = std::chrono::steady_clock::now();
    auto t = std::make_shared<pt::CullTables>();
    pt::build_cull_tables(h.host, eps, *t, r_camera);
    t->eps = eps;
    h.cull_build_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    long long levels = 0;
    for (const auto &c : t->clusters)
        if (c.kind == 0) levels = std::max<long long>(levels, c.n_levels);
    const int rc = check_table_limits(t->slot_tri.size(), t->bvh.size(), levels, t->bvh_depth);
    if (rc != PT_OK) return rc;
    // the small-scene kernels' closest-hit key packs (original index, slot) into 16 bits each
    if (!t->big && (t->slot_tri.size() >= 65536u || h.host.n_tri() >= 65536))
        return fail(PT_ERR_UNSUPPORTED, "a scene on the sphere-tree path has " + std::to_string(t->slot_tri.size()) + " slots; its closest-hit key holds 16 bits");
    if (h.cull_cache.size() >= 4) h.cull_cache.erase(h.cull_cache.begin());
    h.cull_cache.push_back(t);
    out = t;
    return PT_OK;
}

int upload(pt_scene *s, int device) {
    int rc = ptc::use_device(device, "scene");
    if (rc != PT_OK) return rc;
    s->device = device;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) s->cu_count = cus;
    const auto &t = s->shared->tables;
    if ((rc = s->d_exact.upload(t.exact, "exact records", 64)) != PT_OK || (rc = s->d_mats.upload(t.mats, "materials", 64)) != PT_OK) return rc;
    if (s->sky && !s->sky->texels.empty()) {   // (a copy's skybox is the one of the handle it was made from)
        if ((rc = s->d_sky.upload(s->sky->texels, "skybox", 64)) != PT_OK) return rc;
        s->sky_w = s->sky->w;
        s->sky_h = s->sky->h;
    }
    if (s->env && (rc = s->d_env.upload(pt::env_with_apron(s->env->n, s->env->rgb.data()), "environment map", 64)) != PT_OK) return rc;
    if ((rc = ptc::upload_surface(s->surface, t, s->d_surface, s->d_surface)) != PT_OK) return rc;
    return PT_OK;
}

// statistics block and timing events of a launch context, on first use (the scene's device is current)
int ctx_stats_ready(LaunchCtx &c) {
    int rc = c.d_stats ? static_cast<int>(PT_OK) : c.d_stats.alloc(24 * sizeof(unsigned long long), "statistics block");
    if (rc == PT_OK && !c.ev0) rc = c.ev0.create("statistics");
    if (rc == PT_OK && !c.ev1) rc = c.ev1.create("statistics");
    return rc;
}

// The cull hierarchy's radii and margins depend on eps (-EPS): upload on first use, replace if eps changes.
// Callers hold scene->launch_mutex from here until their kernel has been enqueued: a concurrent render with another eps
// must not free the tables between this call and that launch.
const pt_camera kReferenceCamera = {{0.0f, 0.0f, -20.0f}, {1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}};   // main.cpp:126-129

using ptc::view_camera;

// r^, u^, f^ of a lens on camera c (pt_hip.h: pt_lens): right, up, forward normalised in double, rounded to float once.
void lens_axes(const pt_camera &c, float out[9]) {
    const float *v[3] = {c.right, c.up, c.forward};
    for (int a = 0; a < 3; ++a) {
        const double x = v[a][0], y = v[a][1], z = v[a][2];
        const double n = std::sqrt(x * x + y * y + z * z);
        for (int i = 0; i < 3; ++i) out[3 * a + i] = static_cast<float>(v[a][i] / n);
    }
}

// Largest |component| an origin of lens l on camera c can have: max_i(|o_i| + radius sqrt(r^_i^2 + u^_i^2)), which bounds
// |o_i + L_i| because |L_i| <= rho sqrt(cs^2 + sn^2) sqrt(r^_i^2 + u^_i^2) -- times 1 + 2^-18 for the rounding of rho, of the
// sine and cosine, of the products and of the sums (a dozen half-ulps).  A component in which the disc does not extend
// (r^_i = u^_i = 0: L_i is exactly 0) keeps |o_i| exactly, so a lens in front of the reference eye keeps its envelope.
double lens_extent(const pt_camera &c, const pt_lens &l) {
    float ax[9];
    lens_axes(c, ax);
    double e = 0.0;
    for (int i = 0; i < 3; ++i) {
        const double lat = std::sqrt(static_cast<double>(ax[i]) * ax[i] + static_cast<double>(ax[3 + i]) * ax[3 + i]);
        double ei = std::fabs(static_cast<double>(c.origin[i]));
        if (lat > 0.0) ei = (ei + static_cast<double>(l.radius) * lat) * (1.0 + 0x1p-18);
        e = std::max(e, ei);
    }
    return e;
}

// Does the handle's camera move during a launch?  An end pose equal to the start pose bit for bit is no motion (pt_hip.h).
bool motion_active(const pt_scene *s) { return s->has_motion && std::memcmp(&view_camera(s), &s->motion_end, sizeof(pt_camera)) != 0; }

// The same bound for a camera that moves from a to b (pt_hip.h: camera motion), with lens l or none: per component the larger of
// the two poses' values, each pose with its own axes.  Both |o_i(t)| and sqrt(r^_i(t)^2 + u^_i(t)^2) are convex in t (the absolute
// value and the Euclidean norm of functions linear in t), so their largest value over [0, 1] is taken at an end.  A component that
// moves gets lens_extent's rounding allowance (o_i + t * delta_i adds three roundings to its dozen); one that neither moves nor
// lies in the disc keeps |o_i| exactly.
double motion_extent(const pt_camera &a, const pt_camera &b, const pt_lens *l) {
    float axa[9] = {0}, axb[9] = {0};
    if (l) {
        lens_axes(a, axa);
        lens_axes(b, axb);
    }
    double e = 0.0;
    for (int i = 0; i < 3; ++i) {
        const double lata = std::sqrt(static_cast<double>(axa[i]) * axa[i] + static_cast<double>(axa[3 + i]) * axa[3 + i]);
        const double latb = std::sqrt(static_cast<double>(axb[i]) * axb[i] + static_cast<double>(axb[3 + i]) * axb[3 + i]);
        const double radius = l ? static_cast<double>(l->radius) : 0.0;
        double ei = std::max(std::fabs(static_cast<double>(a.origin[i])) + radius * lata, std::fabs(static_cast<double>(b.origin[i])) + radius * latb);
        if (lata > 0.0 || latb > 0.0 || std::memcmp(&a.origin[i], &b.origin[i], sizeof(float)) != 0) ei *= 1.0 + 0x1p-18;
        e = std::max(e, ei);
    }
    return e;
}

// Largest |component| an origin of the orthographic view of camera c can have (pt_hip.h: pt_projection): origin_i = o_i +
// (u r_i + v p_i) with |u|, |v| <= 0.5 up to half a pixel of jitter, which the factor 1 + 2^-18 covers for every image at least two
// pixels wide together with the three roundings -- as stated in the header: max_i(|o_i| + 0.5 (|r_i| + |p_i|)) (1 + 2^-18).
double ortho_extent(const pt_camera &c) {
    double e = 0.0;
    for (int i = 0; i < 3; ++i)
        e = std::max(e, std::fabs(static_cast<double>(c.origin[i])) + 0.5 * (std::fabs(static_cast<double>(c.right[i])) + std::fabs(static_cast<double>(c.up[i]))));
    return e * (1.0 + 0x1p-18);
}

// The envelope radius for the cull tables (get_cull): the largest |component| of every origin a primary ray can have -- 20 for
// the reference's camera at (0, 0, -20).  Only origins matter: the culling is direction-agnostic, so a fisheye or an
// equirectangular view, whose rays start at the eye, has its camera's radius, and an orthographic view adds the extent of its image
// plane.  The cull cache is keyed on (eps, radius): an orthographic view whose origins stay within 20 shares the camera-free tables.
double camera_radius(const pt_scene *s) {
    if (s->has_projection && s->projection.kind == PT_PROJECTION_ORTHOGRAPHIC) return std::max(20.0, ortho_extent(view_camera(s)));
    if (motion_active(s)) return std::max(20.0, motion_extent(view_camera(s), s->motion_end, s->has_lens ? &s->lens : nullptr));
    if (s->has_lens) return std::max(20.0, lens_extent(view_camera(s), s->lens));
    if (!s->has_camera) return 20.0;
    const float *o = s->camera.origin;
    return std::max({20.0, static_cast<double>(std::fabs(o[0])), static_cast<double>(std::fabs(o[1])), static_cast<double>(std::fabs(o[2]))});
}

int ensure_cull(pt_scene *s, float eps) {
    DeviceCull &c = s->cull;
    const double r_camera = camera_radius(s);
    if (c.valid && std::memcmp(&c.eps, &eps, sizeof eps) == 0 && c.r_max == pt::cull_r_max(s->shared->vertex_extent, r_camera)) return PT_OK;
    std::shared_ptr<const pt::CullTables> t;
    int rc = get_cull(*s->shared, eps, r_camera, t);
    if (rc != PT_OK) return rc;
    if (c.valid) PT_HIP_TRY(hipDeviceSynchronize());   // a previous launch may still read the old tables
    c.valid = false;
    c.host = t;
    const char *what = "cull tables";
    if ((rc = c.clusters.upload(t->clusters, what)) != PT_OK || (rc = c.spheres.upload(t->spheres, what)) != PT_OK || (rc = c.bary.upload(t->bary, what)) != PT_OK) return rc;
    c.bary_all.reset();   // (and bvh: no table where the host vector is empty)
    if (!t->bary_all.empty() && (rc = c.bary_all.upload(t->bary_all, what)) != PT_OK) return rc;
    if ((rc = c.exact_slot.upload(t->exact_slot, what)) != PT_OK) return rc;
    c.bvh.reset();
    if (!t->bvh.empty() && (rc = c.bvh.upload(t->bvh, what)) != PT_OK) return rc;
    c.eps = eps;
    c.r_max = t->r_max;
    c.valid = true;
    return PT_OK;
}

struct SceneDeleter {
    void operator()(pt_scene *s) const { pt_scene_destroy(s); }
};
using ScenePtr = std::unique_ptr<pt_scene, SceneDeleter>;   // frees host and device side on every early return / exception

int finish_scene(ScenePtr s, int device, pt_scene **out) {
    pt_scene_host &h = *s->shared;
    if (h.host.n_tri() >= (1 << 23))   // a first, cheap bound; what the layouts really hold is checked on the built hierarchy (get_cull)
        return fail(PT_ERR_INVALID_ARGUMENT, "more than 8 388 607 triangles");
    for (int m : h.host.tri_mat)
        if (m < 0 || m >= h.host.n_mat()) return fail(PT_ERR_INVALID_ARGUMENT, "triangle refers to material " + std::to_string(m));
    pt::build_device_tables(h.host, h.tables);
    h.vertex_extent = pt::vertex_extent(h.host);
    if (!h.host.tri_uv.empty()) s->surface.texcoords = std::make_shared<const std::vector<float>>(h.host.tri_uv);   // a loaded scene: the OBJ's own
    if (device >= 0) {
        const int rc = upload(s.get(), device);
        if (rc != PT_OK) return rc;
    }
    *out = s.release();
    return PT_OK;
}

// The surface tables of the kernel arguments (pt_kernels.hpp: SurfaceUnit).  The rule: the highest table the handle has on its device
// picks the unit; every slot below it holds the handle's own table where it has one and the all-zero stand-in where it has none (no
// material is a dielectric or textured, every Ns is N, every glossy lobe is the mirror); every slot above it stays null.
void bind_surface(const pt_scene &scene, pt::RenderArgs &a) {
    const SurfaceTables &h = scene.surface;
    const DeviceSurface &d = scene.d_surface;
    const bool glass = h.glass && d.glass, tex = h.textures && d.tex_recs, smooth = h.smooth && d.normals, rough = h.rough && d.alpha,
               direct = h.direct && d.lights, envdirect = h.envdirect && d.env_alias && d.env_lights && scene.env && scene.d_env;
    const int unit = envdirect ? pt::kEnvDirectUnit : direct ? pt::kDirectUnit : rough ? pt::kRoughUnit : smooth ? pt::kSmoothUnit : tex ? pt::kTextureUnit : glass ? pt::kGlassUnit : pt::kNoSurfaceUnit;
    if (unit >= pt::kGlassUnit) a.glass = (glass ? d.glass : d.no_glass).get<void>();
    if (unit >= pt::kTextureUnit) {   // (the stand-in marks no material: its coordinates and texels, the table itself, are never read)
        a.tex_recs = (tex ? d.tex_recs : d.no_tex).get<void>();
        a.tex_uv = (tex ? d.tex_uv : d.no_tex).get<float>();
        a.tex_texels = (tex ? d.tex_texels : d.no_tex).get<void>();
        a.tex_bary = d.bary.get<void>();
    }
    if (unit >= pt::kSmoothUnit) a.smooth_normals = (smooth ? d.normals : d.no_normals).get<void>();
    if (unit >= pt::kRoughUnit) a.rough_alpha = (rough ? d.alpha : d.no_alpha).get<float>();
    if (unit == pt::kDirectUnit) {
        a.lights = d.lights.get<void>();
        a.n_lights = static_cast<int32_t>(h.direct->lights.size());
        a.light_area = h.direct->area;
    }
    if (unit == pt::kEnvDirectUnit) {   // (its own copy of the light table: the switch does not depend on direct lighting's)
        a.lights = d.env_lights.get<void>();
        a.n_lights = static_cast<int32_t>(h.envdirect->lights->lights.size());
        a.light_area = h.envdirect->lights->area;
        a.env_alias = d.env_alias.get<void>();
        a.env_cells = h.envdirect->cells;
        a.env_share = h.envdirect->share;
    }
    // (Russian roulette is no table: two numbers of the handle, for the unit that holds the kernels of both switches with the step)
    if ((unit == pt::kDirectUnit || unit == pt::kEnvDirectUnit) && h.rr_start > 0) {
        a.rr_start = h.rr_start;
        a.rr_floor = h.rr_floor;
    }
}

// The part of the kernel arguments that describes the scene (its tables for the current eps).
void fill_scene_args(const pt_scene *scene, float eps, pt::RenderArgs &a) {
    std::memset(&a, 0, sizeof a);
    const pt::CullTables &t = *scene->cull.host;
    const pt::CullConstants &cc = t.cc, &ca = t.cc_all;
    a.clusters = scene->cull.clusters.get<pt::ClusterDesc>();
    a.spheres = scene->cull.spheres.get<pt::SphereRec>();
    a.bary = scene->cull.bary.get<pt::CullRec>();
    a.bary_all = scene->cull.bary_all.get<pt::CullRec>();
    a.a_max_all = ca.a_max; a.m0_all = ca.m0; a.t_guard_all = ca.t_guard;
    a.exact = scene->d_exact.get<pt::ExactRec>();
    a.exact_slot = scene->cull.exact_slot.get<pt::ExactRec>();
    a.bvh = scene->cull.bvh.get<pt::BvhNode>();
    a.n_bvh = static_cast<uint32_t>(t.bvh.size());
    a.bvh_err = t.bvh_err;
    a.mats = scene->d_mats.get<pt::MatRec>();
    a.n_mats = static_cast<int32_t>(scene->shared->tables.mats.size());
    a.sky = scene->d_sky.get<uint8_t>();
    a.sky_w = scene->d_sky ? scene->sky_w : 0;
    a.sky_h = scene->d_sky ? scene->sky_h : 0;
    if (scene->env && scene->d_env) {   // the environment kernels of the skybox kernels (integrate_kernel_environment); never with a skybox
        a.env_map = scene->d_env.get<void>();
        a.env_n = scene->env->n;
    }
    bind_surface(*scene, a);
    a.n_clusters = static_cast<int32_t>(t.clusters.size());
    a.n_tri = scene->shared->host.n_tri();
    a.big = t.big ? 1 : 0;
    a.n_slots = static_cast<uint32_t>(t.slot_tri.size());
    a.eps = eps;
    a.k1 = cc.k1; a.k2 = cc.k2; a.a_max = cc.a_max; a.m0 = cc.m0; a.m0_quad = cc.m0_quad; a.t_guard = cc.t_guard;
    a.r_org = t.r_org;
    a.may_leave_envelope = t.may_leave_envelope ? 1 : 0;
    a.last_segment_filter = 1;
#ifdef PT_TEST_HOOKS
    if (pt::g_cull_mutation.no_last_segment_filter) a.last_segment_filter = 0;
#endif
    a.regen_min_dead = 64;   // (set per launch from -MRR: enqueue_render)
    a.emis_clusters = t.emis_clusters;
    a.emis_large_w0 = t.emis_large_w0;
    a.emis_bvh = t.emis_bvh ? 1u : 0u;
    const bool moving = motion_active(scene);
    if (scene->has_camera || scene->has_lens || moving) {   // the camera twins of the kernels (pt_kernels.hip: integrate_kernel<..., ADAPT | 1>)
        a.camera = 1;
        std::memcpy(a.cam, &view_camera(scene), sizeof a.cam);
    }
    if (scene->has_lens) {   // their lens kernels (integrate_kernel_lens)
        a.lens = 1;
        a.lns[0] = scene->lens.radius;
        a.lns[1] = scene->lens.focus_distance;
        lens_axes(view_camera(scene), a.lns + 2);
    }
    if (scene->has_projection) {   // the projection kernels of the camera twins (integrate_kernel_projection); never with a lens or a motion
        a.camera = 1;
        std::memcpy(a.cam, &view_camera(scene), sizeof a.cam);
        a.projection = scene->projection.kind;
        a.prj_span[0] = scene->projection.span_x;
        a.prj_span[1] = scene->projection.span_y;
        lens_axes(view_camera(scene), a.lns + 2);   // r^, u^, f^ in the slots a lens would fill (a.lens stays 0)
    }
    if (moving) {   // the motion twins of either (integrate_kernel_motion, integrate_kernel_motion_lens): end - start, one float subtraction each
        a.motion = 1;
        float end_pose[12];
        static_assert(sizeof end_pose == sizeof(pt_camera), "pt_camera: twelve floats");
        std::memcpy(end_pose, &scene->motion_end, sizeof end_pose);
        for (int j = 0; j < 12; ++j) a.cam_d[j] = end_pose[j] - a.cam[j];
        if (scene->has_lens) {
            float end_axes[9];
            lens_axes(scene->motion_end, end_axes);
            for (int j = 0; j < 9; ++j) a.lns_d[j] = end_axes[j] - a.lns[2 + j];
        }
    }
}

void zero_stats(const pt_scene *scene, pt_render_stats *stats) {
    std::memset(stats, 0, sizeof *stats);
    stats->n_triangles = scene->shared->host.n_tri();
}

// Enqueue one integrator launch on `stream` for the context `ctx` (its scheduler words, its statistics block).  Never waits
// for the device except to grow the scheduler words.  The caller holds ctx.mutex.
int enqueue_render(pt_scene *scene, LaunchCtx &ctx, const pt_render_params *p, const ptc::AccumPlanes &planes, hipStream_t stream,
                   bool want_stats) {
    ctx.stats_pending = false;
    ctx.last_chunks = 0;
    PT_HIP_TRY(hipSetDevice(scene->device));
    std::lock_guard<std::mutex> launch_lock(scene->launch_mutex);
    const int crc = ensure_cull(scene, p->eps);
    if (crc != PT_OK) return crc;
    pt::RenderArgs a;
    fill_scene_args(scene, p->eps, a);
    // (a handle that answers 1 to get_direct_lighting never renders without its light table)
    if (scene->surface.direct && !a.lights) return fail(PT_ERR_INVALID_ARGUMENT, "direct lighting: the handle has the switch set and no light table on its device");
    if (scene->surface.rr_start > 0 && a.rr_start <= 0) return fail(PT_ERR_INVALID_ARGUMENT, "Russian roulette: the handle has it set and neither direct lighting nor environment sampling on its device");
    if (scene->surface.envdirect && !a.env_alias) return fail(PT_ERR_INVALID_ARGUMENT, "environment sampling: the handle has the switch set and no table on its device");
    a.vec_ok = (p->width % 4 == 0) &&
               ((reinterpret_cast<uintptr_t>(planes.sum) | reinterpret_cast<uintptr_t>(planes.sum2) | reinterpret_cast<uintptr_t>(planes.count)) % 16 == 0);
    a.sum = planes.sum;
    a.sum2 = planes.sum2;
    a.count = planes.count;
    a.width = p->width; a.height = p->height; a.row_begin = p->row_begin; a.row_end = p->row_end;
    a.row_stride = std::max(1, p->row_stride);
    a.band_rows = ptc::band_rows(p);
    const pt::plan::Overrides &ov = g_plan_overrides;
    a.regen_min_dead = ov.regen_min_dead > 0 ? static_cast<uint32_t>(ov.regen_min_dead) : pt::regen_min_dead_for(p->max_ray_reflections);
    a.pass_begin = p->pass_begin; a.pass_count = p->pass_count; a.mrr = p->max_ray_reflections;
    a.error = p->error; a.seed = p->seed;
    if (p->row_end == p->row_begin) return PT_OK;
    int rc;
    if (a.projection == PT_PROJECTION_ORTHOGRAPHIC) {
        // u and v reach 0.5 + half a pixel at the left and the top edge (the jitter of column 0 and row 0): origins may leave
        // ortho_extent by 0.5 (|r_i| / W + |p_i| / H), which must stay within half of the envelope's slack of one scene unit
        for (int i = 0; i < 3; ++i)
            if (!(0.5 * (std::fabs(static_cast<double>(a.cam[3 + i])) / a.width + std::fabs(static_cast<double>(a.cam[6 + i])) / a.height) <= 0.5))
                return fail(PT_ERR_UNSUPPORTED, "orthographic projection: a pixel of this image is wider than one scene unit (|right_i| / width + |up_i| / height > 1)");
    }
    if (!ctx.ev_done && (rc = ctx.ev_done.create("launch context", hipEventDisableTiming)) != PT_OK) return rc;
    if (want_stats) {
        if ((rc = ctx_stats_ready(ctx)) != PT_OK) return rc;
        a.stats = ctx.d_stats.get<unsigned long long>();
    }
    // one wave = one tile of 8 rows; how many pixels wide depends on the kernel this launch runs
    const bool sky = a.sky != nullptr || a.env_map != nullptr;   // (an environment launch is planned as the skybox launch it would be)
    const pt::plan::Tiles tiles = pt::plan::plan_tiles({a.width, a.band_rows, sky, a.big != 0, want_stats, a.may_leave_envelope != 0, a.error,
                                                        a.pass_begin, a.pass_count, pt::plan::view_of(a.camera != 0, a.lens != 0, a.motion != 0), scene->cu_count,
                                                        // (the scene's flag, and a handle with nothing a plain launch does not read)
                                                        scene->cull.host->room && a.env_map == nullptr && a.projection == 0 && pt::surface_unit_of(a) == pt::kNoSurfaceUnit},
                                                       pt::integrator_build(), ov);
    a.narrow = tiles.narrow;
    a.adapt_pool = tiles.adapt_pool;
    a.blocks_x = tiles.blocks_x;
    const uint32_t n_tiles = tiles.n_tiles;
    int waves_per_cu = 24;
    PT_HIP_TRY(pt::integrator_waves_per_cu(tiles.variant, &waves_per_cu));   // (a projection launch: its camera twin's, which are its own)
    const uint32_t slots = static_cast<uint32_t>(scene->cu_count) * static_cast<uint32_t>(std::max(1, waves_per_cu));
    const auto [n_chunks, chunk_passes] = pt::plan::plan_chunks(n_tiles, slots, p->pass_count, sky, a.narrow != 0, want_stats, ov);
    if (static_cast<unsigned long long>(n_tiles) * n_chunks > 0x7fffffffull) return fail(PT_ERR_INVALID_ARGUMENT, "too many work items");
    if (ctx.has_prev && ctx.prev_stream != stream) PT_HIP_TRY(hipStreamWaitEvent(stream, ctx.ev_done.get(), 0));
    const size_t sched_bytes = (1 + static_cast<size_t>(n_tiles)) * sizeof(uint32_t);
    if (ctx.d_sched.bytes() < sched_bytes) {
        if (ctx.has_prev) PT_HIP_TRY(hipStreamSynchronize(stream));   // an earlier launch of this context may still use the old words
        if ((rc = ctx.d_sched.alloc(sched_bytes, "scheduler words")) != PT_OK) return rc;
    }
    PT_HIP_TRY(hipMemsetAsync(ctx.d_sched.get<void>(), 0, sched_bytes, stream));
    a.sched = ctx.d_sched.get<uint32_t>();
    a.n_tiles = n_tiles;
    a.n_chunks = n_chunks;
    a.chunk_passes = chunk_passes;
    if (want_stats) {
        PT_HIP_TRY(hipMemsetAsync(ctx.d_stats.get<void>(), 0, 24 * sizeof(unsigned long long), stream));
        PT_HIP_TRY(hipEventRecord(ctx.ev0.get(), stream));
    }
    const hipError_t launched = pt::launch_integrator(a, tiles.variant, stream);
    if (const int unit = pt::surface_unit_of(a); launched == hipErrorNotSupported && unit != pt::kNoSurfaceUnit) {
        static const char *const kWhat[][2] = {{"dielectrics", "dielectric"}, {"textures", "texture"}, {"shading normals", "smooth"}, {"roughness", "rough"}, {"direct lighting", "direct"}, {"environment sampling", "environment-sampling"}, {"Russian roulette", "roulette"}};
        const char *const *w = kWhat[unit - pt::kGlassUnit];
        return fail(PT_ERR_UNSUPPORTED, std::string(w[0]) + ": this diagnostic build of the library has no " + w[1] + " kernels");
    }
    PT_HIP_TRY(launched);
    g_last_variant.store(pt::plan::variant_id(tiles.variant), std::memory_order_relaxed);
    if (want_stats) PT_HIP_TRY(hipEventRecord(ctx.ev1.get(), stream));
    PT_HIP_TRY(hipEventRecord(ctx.ev_done.get(), stream));
    ctx.has_prev = true;
    ctx.prev_stream = stream;
    ctx.last_chunks = n_chunks;
    ctx.stats_pending = want_stats;
    return PT_OK;
}

// Wait for the launch enqueue_render put on `stream` and read its statistics.  The caller holds ctx.mutex.
int collect_stats(pt_scene *scene, LaunchCtx &ctx, hipStream_t stream, pt_render_stats *stats) {
    zero_stats(scene, stats);
    if (!ctx.stats_pending) return PT_OK;   // an empty band
    ctx.stats_pending = false;
    PT_HIP_TRY(hipSetDevice(scene->device));
    unsigned long long h[24];
    PT_HIP_TRY(hipMemcpyAsync(h, ctx.d_stats.get<void>(), sizeof h, hipMemcpyDeviceToHost, stream));
    PT_HIP_TRY(hipStreamSynchronize(stream));
    float ms = -1.0f;
    PT_HIP_TRY(hipEventElapsedTime(&ms, ctx.ev0.get(), ctx.ev1.get()));
    stats->samples_traced = h[0];
    stats->segments = h[1];
    stats->contributing = h[2];
    stats->exact_tests = h[3];
    stats->misses = h[4];
    stats->wave_segments = h[5];
    stats->wave_node_rounds = h[6];
    stats->wave_exact_iterations = h[7];
    stats->kernel_ms = ms;
    stats->n_chunks = static_cast<int32_t>(ctx.last_chunks);
    stats->partial_commit_rounds = static_cast<int32_t>(std::min<unsigned long long>(h[8], 0x7fffffffull));
    stats->verify_checked = h[9];      // both stay 0 unless this is a verification build (-DPT_VERIFY_BRUTE / -DPT_VERIFY_SHIPPED)
    stats->verify_mismatches = h[10];
#ifdef PT_TEST_HOOKS
    if (h[10] != 0) {   // verification build: one disagreeing segment, for diagnosis
        auto f = [](unsigned long long w, int hi) { const uint32_t b = static_cast<uint32_t>(hi ? w >> 32 : w); float x; std::memcpy(&x, &b, 4); return x; };
        std::fprintf(stderr, "PT_VERIFY example: all-triangles loop -> triangle %d (key %016llx), culled search -> triangle %d (key %016llx); "
                             "ray o = (%.9g, %.9g, %.9g) d = (%.9g, %.9g, %.9g)\n",
                     static_cast<int>(h[11] & 0xFFFFFFFFu), h[11], static_cast<int>(h[12] & 0xFFFFFFFFu), h[12],
                     f(h[13], 1), f(h[13], 0), f(h[14], 1), f(h[14], 0), f(h[15], 1), f(h[15], 0));
    }
#endif
#ifdef PT_PHASE_TIMERS
    std::fprintf(stderr, "PT_PHASE_TIMERS cycles:");
    for (int k = 0; k < 8; ++k) std::fprintf(stderr, " %llu", h[16 + k]);
    std::fprintf(stderr, "\n");
#endif
    return PT_OK;
}

}  // namespace

namespace ptc {

// Rows the accumulator planes of a call hold: the band's rows, or with a row stride eight per tile row of the band.
int32_t band_rows(const pt_render_params *p) {
    const int32_t rows = p->row_end - p->row_begin;
    if (p->row_stride <= 1 || rows <= 0) return rows;
    const int32_t period = 8 * p->row_stride;
    return 8 * ((rows + period - 1) / period);
}

int check_params(const pt_scene *scene, const pt_render_params *p) {
    if (!scene || !p) return fail(PT_ERR_INVALID_ARGUMENT, "null scene or params");
    if (const int rc = check_has_device(scene)) return rc;
    if (p->width <= 0 || p->height <= 0) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive");
    if (p->row_begin < 0 || p->row_end > p->height || p->row_begin > p->row_end)
        return fail(PT_ERR_INVALID_ARGUMENT, "row band outside the image");
    if (p->row_stride < 0 || (p->row_stride > 1 && p->row_begin % 8 != 0))
        return fail(PT_ERR_INVALID_ARGUMENT, "row_stride must be 0 / 1 (contiguous rows) or n > 1 with row_begin a multiple of 8 (every n-th tile row of 8 rows)");
    if (p->pass_begin < 0 || p->pass_count < 0) return fail(PT_ERR_INVALID_ARGUMENT, "negative pass range");
    if (static_cast<long long>(p->width) * p->height > 0x7fffffffLL)
        return fail(PT_ERR_INVALID_ARGUMENT, "image has more than 2^31 pixels");
    if (p->rng_policy == PT_RNG_REFERENCE_STREAM)
        return fail(PT_ERR_UNSUPPORTED, "PT_RNG_REFERENCE_STREAM: the reference's serial minstd_rand0 streams (material.h:16-20) have no "
                                        "parallel evaluation order; the device implements PT_RNG_COUNTER");
    if (p->rng_policy != PT_RNG_COUNTER) return fail(PT_ERR_INVALID_ARGUMENT, "unknown rng_policy");
    return PT_OK;
}

int session_create_on(pt_scene *scene, int32_t width, int32_t height, int32_t row_begin, int32_t row_end, const AccumPlanes *borrowed,
                      pt_session **out, int32_t row_stride) {
    if (!out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    pt_render_params p;
    std::memset(&p, 0, sizeof p);
    p.width = width; p.height = height; p.row_begin = row_begin; p.row_end = row_end; p.row_stride = row_stride;
    int rc = check_params(scene, &p);
    if (rc != PT_OK) return rc;
    PT_HIP_TRY(hipSetDevice(scene->device));
    std::unique_ptr<pt_session> s(new pt_session);
    s->scene = scene;
    s->width = width; s->height = height; s->row_begin = row_begin; s->row_end = row_end; s->row_stride = std::max(1, row_stride);
    s->n = static_cast<size_t>(band_rows(&p)) * width;
    if ((rc = s->stream.create("pt_session_create")) != PT_OK) return rc;
    if (borrowed) {   // the caller zeroes and frees them
        s->planes = *borrowed;
        s->planes.n = s->n;
    } else {
        PlaneLayout l;
        s->planes = AccumPlanes::in(l, s->n);
        if ((rc = s->d_band.alloc(l.end + 256, "pt_session_create")) != PT_OK) return rc;
        PT_HIP_TRY(hipMemsetAsync(s->d_band.get<void>(), 0, s->d_band.bytes(), s->stream.get()));
        s->planes.bind(s->d_band);
    }
    *out = s.release();
    return PT_OK;
}

int session_enqueue(pt_session *s, const pt_render_params *p, bool want_stats) {
    if (!s || !p) return fail(PT_ERR_INVALID_ARGUMENT, "null session or params");
    if (p->width != s->width || p->height != s->height || p->row_begin != s->row_begin || p->row_end != s->row_end ||
        std::max(1, p->row_stride) != s->row_stride)
        return fail(PT_ERR_INVALID_ARGUMENT, "params describe another band than the session's");
    const int rc = check_params(s->scene, p);
    if (rc != PT_OK) return rc;
    return enqueue_render(s->scene, s->ctx, p, s->planes, s->stream.get(), want_stats);
}

const pt_camera &view_camera(const pt_scene *s) { return s->has_camera ? s->camera : kReferenceCamera; }

int scene_trace_args(pt_scene *scene, float eps, pt::RenderArgs &a) {
    const int rc = ensure_cull(scene, eps);
    if (rc != PT_OK) return rc;
    fill_scene_args(scene, eps, a);
    return PT_OK;
}

int session_collect(pt_session *s, pt_render_stats *stats) {
    if (!s || !stats) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    return collect_stats(s->scene, s->ctx, s->stream.get(), stats);
}

}  // namespace ptc

using ptc::check_params;

extern "C" {

int pt_abi_version(void) { return PT_ABI_VERSION; }

void *pt_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        ptc::g_error = "pt_host_alloc: hipHostMalloc failed";
        return nullptr;
    }
    return p;
}

void pt_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

int pt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *pt_last_error(void) { return ptc::g_error.c_str(); }

int pt_scene_timings(const pt_scene *scene, double *seconds) {
    if (!scene || !seconds) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lock(scene->shared->cull_mutex);
    seconds[0] = scene->shared->load_seconds;
    seconds[1] = scene->shared->cull_build_seconds;
    return PT_OK;
}

int pt_table_limits_check(uint64_t n_slots, uint64_t n_bvh_nodes, int32_t n_levels) {
    return guarded([&] { return check_table_limits(n_slots, n_bvh_nodes, n_levels); });
}
int pt_table_limits_check_tree(uint64_t n_slots, uint64_t n_bvh_nodes, int32_t n_levels, int32_t bvh_depth) {
    return guarded([&] { return check_table_limits(n_slots, n_bvh_nodes, n_levels, bvh_depth); });
}
static_assert(PT_MAX_BVH_DEPTH == pt::kMaxBvhDepth, "the ABI header states the box tree's depth limit");

int pt_scene_skybox_size(const pt_scene *scene, int32_t *width, int32_t *height) {
    if (!scene || !width || !height) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    *width = scene->sky ? scene->sky->w : 0;
    *height = scene->sky ? scene->sky->h : 0;
    return PT_OK;
}

static int scene_load_obj_impl(const char *model_dir, const char *model_name, int device, uint32_t flags, pt_scene **out) {
    if (!model_dir || !model_name || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (flags & ~static_cast<uint32_t>(PT_LOAD_GEOMETRIC_PLANES)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_scene_load_obj_ex: unknown flag");
    ScenePtr s(new pt_scene);
    s->shared = std::make_shared<pt_scene_host>();
    std::string err;
    bool io = false;
    const auto t0 = std::chrono::steady_clock::now();
    if (!pt::load_obj(model_dir, model_name, s->shared->host, err, io, (flags & PT_LOAD_GEOMETRIC_PLANES) != 0)) return fail(io ? PT_ERR_IO : PT_ERR_PARSE, err);
    // (finish_scene destroys the pt_scene on failure -- no device, bad ordinal, upload error --: keep the host side alive here)
    const std::shared_ptr<pt_scene_host> h = s->shared;
    const int rc = finish_scene(std::move(s), device, out);
    h->load_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();   // (includes the first device's upload)
    return rc;
}

static int scene_create_impl(const float *triangles, const int32_t *triangle_material, int32_t n_triangles, const float *materials,
                    int32_t n_materials, int device, pt_scene **out) {
    if (!out || n_triangles < 0 || n_materials < 0 || (n_triangles > 0 && (!triangles || !triangle_material)) ||
        (n_materials > 0 && !materials))
        return fail(PT_ERR_INVALID_ARGUMENT, "null table or negative count");
    *out = nullptr;
    ScenePtr s(new pt_scene);
    s->shared = std::make_shared<pt_scene_host>();
    pt::HostScene &h = s->shared->host;
    h.tri.assign(triangles, triangles + static_cast<size_t>(n_triangles) * PT_TRIANGLE_FLOATS);
    h.tri_mat.assign(triangle_material, triangle_material + n_triangles);
    h.mat.assign(materials, materials + static_cast<size_t>(n_materials) * PT_MATERIAL_FLOATS);
    return finish_scene(std::move(s), device, out);
}

static int scene_clone_impl(const pt_scene *src, int device, pt_scene **out) {
    if (!src || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    ScenePtr s(new pt_scene);
    s->shared = src->shared;   // parsed model, tables, hierarchies built so far
    s->sky = src->sky;         // the skybox of the handle the copy is made from
    s->env = src->env;         // or its environment
    s->surface = src->surface;   // and its dielectrics, texture coordinates and textures, shading normals, roughness list and light table
    s->has_camera = src->has_camera;   // and its camera
    s->camera = src->camera;
    s->has_lens = src->has_lens;       // and lens
    s->lens = src->lens;
    s->has_motion = src->has_motion;   // and camera motion
    s->motion_end = src->motion_end;
    s->has_projection = src->has_projection;   // and projection
    s->projection = src->projection;
    if (device >= 0) {
        const int rc = upload(s.get(), device);
        if (rc != PT_OK) return rc;
    }
    *out = s.release();
    return PT_OK;
}

static int scene_set_skybox_bmp_impl(pt_scene *scene, const char *path) {
    if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
    if (path && *path && scene->surface.envdirect) return fail(PT_ERR_INVALID_ARGUMENT, "skybox: the scene handle has environment sampling switched on");
    if (path && *path && scene->env) return fail(PT_ERR_INVALID_ARGUMENT, "skybox: the scene handle has an environment; a handle has a skybox or an environment");
    std::vector<uint8_t> texels;
    int w = 0, h = 0;
    if (path && *path) {
        std::string why;   // (pt_bmp.hpp: the reader pt_texture_load_bmp shares)
        bool cannot_open = false;
        if (!pt::read_bmp24(path, texels, w, h, why, cannot_open) && cannot_open) return fail(PT_ERR_IO, "skybox: " + why);
        if (!why.empty()) return fail(PT_ERR_PARSE, std::string("skybox ") + path + ": " + why);
    }
    if (scene->device >= 0) {
        PT_HIP_TRY(hipSetDevice(scene->device));
        PT_HIP_TRY(hipDeviceSynchronize());
        scene->d_sky.reset();
        int rc;
        if (!texels.empty() && (rc = scene->d_sky.upload(texels, "skybox", 64)) != PT_OK) return rc;
    }
    // (per-device copies made from THIS handle afterwards inherit the skybox; other handles of the same model keep theirs)
    scene->sky_w = w;
    scene->sky_h = h;
    if (texels.empty()) {
        scene->sky.reset();
    } else {
        auto sk = std::make_shared<pt_sky_texels>();
        sk->texels.swap(texels);
        sk->w = w;
        sk->h = h;
        scene->sky = std::move(sk);
    }
    return PT_OK;
}

static bool finite3(const float *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// The camera at `eye` looking at `target` whose up vector has length sy and whose right vector sy * aspect (pt_camera_look_at:
// sy = 2 tan(fov_y / 2); pt_camera_ortho: sy = the view height), in double, rounded to float once.  `who` names the caller.
static int camera_frame(const std::string &who, const float eye[3], const float target[3], const float up[3], double sy, float aspect, pt_camera *out) {
    double f[3], u[3], r[3];
    for (int i = 0; i < 3; ++i) {
        f[i] = static_cast<double>(target[i]) - static_cast<double>(eye[i]);
        u[i] = up[i];
    }
    const double fl = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    const double ul = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    if (!(fl > 0.0) || !(ul > 0.0)) return fail(PT_ERR_INVALID_ARGUMENT, who + ": eye == target or a zero up vector");
    for (double &x : f) x /= fl;
    r[0] = u[1] * f[2] - u[2] * f[1];   // cross(up, forward)
    r[1] = u[2] * f[0] - u[0] * f[2];
    r[2] = u[0] * f[1] - u[1] * f[0];
    const double rl = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (!(rl > 1e-6 * ul)) return fail(PT_ERR_INVALID_ARGUMENT, who + ": up is parallel to the view direction");
    for (double &x : r) x /= rl;
    const double sx = sy * (aspect > 0.0f ? static_cast<double>(aspect) : 1.0);
    const double v[3] = {f[1] * r[2] - f[2] * r[1], f[2] * r[0] - f[0] * r[2], f[0] * r[1] - f[1] * r[0]};   // cross(forward, right)
    for (int i = 0; i < 3; ++i) {
        out->origin[i] = eye[i];
        out->right[i] = static_cast<float>(r[i] * sx);
        out->up[i] = static_cast<float>(v[i] * sy);
        out->forward[i] = static_cast<float>(f[i]);
    }
    return PT_OK;
}

static int camera_look_at_impl(const float eye[3], const float target[3], const float up[3], float fov_y_degrees, float aspect,
                               pt_camera *out) {
    if (!eye || !target || !up || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    if (!finite3(eye) || !finite3(target) || !finite3(up) || !std::isfinite(fov_y_degrees) || !std::isfinite(aspect))
        return fail(PT_ERR_INVALID_ARGUMENT, "look_at: non-finite input");
    if (!(fov_y_degrees > 0.0f && fov_y_degrees < 180.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "look_at: fov_y must lie in (0, 180) degrees");
    return camera_frame("look_at", eye, target, up, 2.0 * std::tan(static_cast<double>(fov_y_degrees) * (M_PI / 360.0)), aspect, out);
}

static int camera_ortho_impl(const float eye[3], const float target[3], const float up[3], float view_height, float aspect, pt_camera *out) {
    if (!eye || !target || !up || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    if (!finite3(eye) || !finite3(target) || !finite3(up) || !std::isfinite(view_height) || !std::isfinite(aspect))
        return fail(PT_ERR_INVALID_ARGUMENT, "camera_ortho: non-finite input");
    if (!(view_height > 0.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "camera_ortho: the view height must be positive");
    return camera_frame("camera_ortho", eye, target, up, static_cast<double>(view_height), aspect, out);
}

// pt_projection_make: the spans in double, rounded to float once.
static int projection_make_impl(int32_t kind, float fov_y_degrees, float aspect, pt_projection *out) {
    if (!out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    if (kind < PT_PROJECTION_PERSPECTIVE || kind > PT_PROJECTION_EQUIRECTANGULAR) return fail(PT_ERR_INVALID_ARGUMENT, "projection: unknown kind " + std::to_string(kind));
    pt_projection p = {kind, 0.0f, 0.0f};
    if (kind == PT_PROJECTION_FISHEYE || kind == PT_PROJECTION_EQUIRECTANGULAR) {
        if (!std::isfinite(fov_y_degrees) || !std::isfinite(aspect)) return fail(PT_ERR_INVALID_ARGUMENT, "projection: non-finite input");
        if (kind == PT_PROJECTION_EQUIRECTANGULAR && fov_y_degrees <= 0.0f) {   // the full sphere
            p.span_x = static_cast<float>(2.0 * M_PI);
            p.span_y = static_cast<float>(M_PI);
        } else {
            if (!(fov_y_degrees > 0.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "projection: fov_y must be positive");
            const double rad = static_cast<double>(fov_y_degrees) * (M_PI / 180.0);
            p.span_y = static_cast<float>(rad);
            p.span_x = static_cast<float>(rad * (aspect > 0.0f ? static_cast<double>(aspect) : 1.0));
        }
    }
    *out = p;
    return PT_OK;
}

// Can lens l (radius > 0, focus distance > 0) be used with camera c?  D . f^ = u (right . f^) + v (up . f^) + |forward| with
// |u|, |v| < 1 stays positive if |forward| > |right . f^| + |up . f^|; and every lens origin must lie within PT_CAMERA_MAX_ORIGIN.
static int check_lens_on(const pt_camera &c, const pt_lens &l) {
    double f[3], fl = 0.0;
    for (int i = 0; i < 3; ++i) {
        f[i] = c.forward[i];
        fl += f[i] * f[i];
    }
    fl = std::sqrt(fl);
    double rf = 0.0, uf = 0.0;
    for (int i = 0; i < 3; ++i) {
        rf += static_cast<double>(c.right[i]) * (f[i] / fl);
        uf += static_cast<double>(c.up[i]) * (f[i] / fl);
    }
    if (!(fl > std::fabs(rf) + std::fabs(uf)))
        return fail(PT_ERR_INVALID_ARGUMENT, "lens: the camera's view direction can reach the lens plane (|forward| <= |right . f| + |up . f|)");
    if (!(lens_extent(c, l) <= PT_CAMERA_MAX_ORIGIN))
        return fail(PT_ERR_UNSUPPORTED, "lens: an origin on the lens could lie beyond PT_CAMERA_MAX_ORIGIN (" + std::to_string(PT_CAMERA_MAX_ORIGIN) + ")");
    return PT_OK;
}

static int recheck_motion(const pt_scene *scene, const pt_camera &cam, const pt_lens *l);   // (below, with the motion's checks)

// NULL or radius 0: back to the pinhole.  Checks everything before it changes anything.
static int scene_set_lens_impl(pt_scene *scene, const pt_lens *lens) {
    if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
    if (lens) {
        if (!std::isfinite(lens->radius) || !std::isfinite(lens->focus_distance)) return fail(PT_ERR_INVALID_ARGUMENT, "lens: non-finite value");
        if (lens->radius < 0.0f) return fail(PT_ERR_INVALID_ARGUMENT, "lens: negative radius");
    }
    if (!lens || lens->radius == 0.0f) {
        const int mrc = recheck_motion(scene, view_camera(scene), nullptr);   // (without a lens the origin bound is the camera's)
        if (mrc != PT_OK) return mrc;
        scene->has_lens = false;
        scene->lens = pt_lens{};
        return PT_OK;
    }
    if (!(lens->focus_distance > 0.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "lens: the focus distance must be positive");
    if (scene->has_projection) return fail(PT_ERR_UNSUPPORTED, "lens: the handle has a non-perspective projection; clear one of the two first");
    int rc = check_lens_on(view_camera(scene), *lens);
    if (rc != PT_OK) return rc;
    if (scene->has_motion && (rc = check_lens_on(scene->motion_end, *lens)) != PT_OK) return rc;
    if ((rc = recheck_motion(scene, view_camera(scene), lens)) != PT_OK) return rc;
    scene->lens = *lens;
    scene->has_lens = true;
    return PT_OK;
}

static int scene_get_lens_impl(const pt_scene *scene, pt_lens *lens, int32_t *is_set) {
    if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
    if (lens) *lens = scene->has_lens ? scene->lens : pt_lens{};
    if (is_set) *is_set = scene->has_lens ? 1 : 0;
    return PT_OK;
}

// Can the camera move from a to b within one launch (pt_hip.h: camera motion), with lens l or none?  Every axis is linear in t, so
// det(right(t), up(t), forward(t)) is a combination, with non-negative weights that sum to 1, of the eight mixed determinants
// det(right_X, up_Y, forward_Z), X, Y, Z in {a, b}: with all eight of one sign and away from 0 no t in [0, 1] makes the axes
// dependent, and D = u right + v up + forward (coefficient 1 on forward) cannot vanish.  Likewise D(t) . f^(t) is such a combination
// of D_X . f^_Y, each positive in the image if forward_X . f^_Y > |right_X . f^_Y| + |up_X . f^_Y|.
static int check_motion(const pt_scene *scene, const pt_camera &a, const pt_lens *l, const pt_camera &b) {
    const pt_camera *pose[2] = {&a, &b};
    auto len = [](const float *v) { return std::sqrt(static_cast<double>(v[0]) * v[0] + static_cast<double>(v[1]) * v[1] + static_cast<double>(v[2]) * v[2]); };
    int sign = 0;
    for (int k = 0; k < 8; ++k) {
        const float *rf = pose[k & 1]->right, *uf = pose[(k >> 1) & 1]->up, *ff = pose[k >> 2]->forward;
        const double r[3] = {rf[0], rf[1], rf[2]}, u[3] = {uf[0], uf[1], uf[2]}, f[3] = {ff[0], ff[1], ff[2]};
        const double det = r[0] * (u[1] * f[2] - u[2] * f[1]) - r[1] * (u[0] * f[2] - u[2] * f[0]) + r[2] * (u[0] * f[1] - u[1] * f[0]);
        if (!(std::fabs(det) > 1e-6 * len(rf) * len(uf) * len(ff)))
            return fail(PT_ERR_INVALID_ARGUMENT, "camera motion: right, up and forward can become linearly dependent between the two poses");
        const int sg = det > 0.0 ? 1 : -1;
        if (sign != 0 && sg != sign)
            return fail(PT_ERR_INVALID_ARGUMENT, "camera motion: the orientation of right, up and forward changes between the two poses");
        sign = sg;
    }
    if (l) {
        float ax[2][9];
        lens_axes(a, ax[0]);
        lens_axes(b, ax[1]);
        for (int x = 0; x < 2; ++x)
            for (int y = 0; y < 2; ++y) {
                const float *fh = ax[y] + 6;
                double rf = 0.0, uf = 0.0, ff = 0.0;
                for (int i = 0; i < 3; ++i) {
                    rf += static_cast<double>(pose[x]->right[i]) * fh[i];
                    uf += static_cast<double>(pose[x]->up[i]) * fh[i];
                    ff += static_cast<double>(pose[x]->forward[i]) * fh[i];
                }
                if (!(ff > std::fabs(rf) + std::fabs(uf)))
                    return fail(PT_ERR_INVALID_ARGUMENT, "camera motion: a view direction can reach the lens plane between the two poses (forward . f <= |right . f| + |up . f|)");
            }
    }
    const double bound = l ? static_cast<double>(PT_CAMERA_MAX_ORIGIN) : std::max(static_cast<double>(PT_CAMERA_MAX_ORIGIN), scene->shared->vertex_extent);
    if (!(motion_extent(a, b, l) <= bound))
        return fail(PT_ERR_UNSUPPORTED, "camera motion: an origin between the two poses could lie beyond PT_CAMERA_MAX_ORIGIN (" + std::to_string(PT_CAMERA_MAX_ORIGIN) + ")");
    return PT_OK;
}

static int check_camera(const pt_scene *scene, const pt_camera *cam);

// Can camera c carry an orthographic projection on this scene?  Every origin of its image plane must lie within the bound a camera
// origin has (check_camera).
static int check_ortho_on(const pt_scene *scene, const pt_camera &c) {
    const double max_origin = std::max(static_cast<double>(PT_CAMERA_MAX_ORIGIN), scene->shared->vertex_extent);
    if (!(ortho_extent(c) <= max_origin))
        return fail(PT_ERR_UNSUPPORTED, "orthographic projection: an origin of the image plane could lie beyond PT_CAMERA_MAX_ORIGIN (" +
                                            std::to_string(PT_CAMERA_MAX_ORIGIN) + ") and beyond the scene's largest |vertex coordinate|");
    return PT_OK;
}
static bool ortho_on(const pt_scene *scene) { return scene->has_projection && scene->projection.kind == PT_PROJECTION_ORTHOGRAPHIC; }

// The motion the handle has against a camera and lens it is about to get (an end pose equal to the new camera is no motion).
static int recheck_motion(const pt_scene *scene, const pt_camera &cam, const pt_lens *l) {
    if (!scene->has_motion || std::memcmp(&cam, &scene->motion_end, sizeof cam) == 0) return PT_OK;
    return check_motion(scene, cam, l, scene->motion_end);
}

// NULL: back to the reference's camera.  Checks everything before it changes anything.
static int scene_set_camera_impl(pt_scene *scene, const pt_camera *cam) {
    if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
    if (!cam) {
        if (scene->has_lens) {   // (the lens stays: it must fit the reference camera as well)
            const int rc = check_lens_on(kReferenceCamera, scene->lens);
            if (rc != PT_OK) return rc;
        }
        const int mrc = recheck_motion(scene, kReferenceCamera, scene->has_lens ? &scene->lens : nullptr);
        if (mrc != PT_OK) return mrc;
        if (ortho_on(scene)) {
            const int orc = check_ortho_on(scene, kReferenceCamera);
            if (orc != PT_OK) return orc;
        }
        scene->has_camera = false;
        scene->camera = pt_camera{};
        return PT_OK;
    }
    int rc = check_camera(scene, cam);
    if (rc != PT_OK) return rc;
    if (scene->has_lens && (rc = check_lens_on(*cam, scene->lens)) != PT_OK) return rc;
    if ((rc = recheck_motion(scene, *cam, scene->has_lens ? &scene->lens : nullptr)) != PT_OK) return rc;
    if (ortho_on(scene) && (rc = check_ortho_on(scene, *cam)) != PT_OK) return rc;
    scene->camera = *cam;
    scene->has_camera = true;
    return PT_OK;
}

// What pt_scene_set_camera asks of a camera by itself (the end pose of a motion passes the same).
static int check_camera(const pt_scene *scene, const pt_camera *cam) {
    if (!finite3(cam->origin) || !finite3(cam->right) || !finite3(cam->up) || !finite3(cam->forward))
        return fail(PT_ERR_INVALID_ARGUMENT, "camera: non-finite component");
    double r[3], u[3], f[3];
    for (int i = 0; i < 3; ++i) {
        r[i] = cam->right[i];
        u[i] = cam->up[i];
        f[i] = cam->forward[i];
    }
    auto len = [](const double *v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
    if (!(len(f) > 0.0)) return fail(PT_ERR_INVALID_ARGUMENT, "camera: zero forward vector");
    const double det = r[0] * (u[1] * f[2] - u[2] * f[1]) - r[1] * (u[0] * f[2] - u[2] * f[0]) + r[2] * (u[0] * f[1] - u[1] * f[0]);
    if (!(std::fabs(det) > 1e-6 * len(r) * len(u) * len(f)))
        return fail(PT_ERR_INVALID_ARGUMENT, "camera: right, up and forward are not linearly independent");
    // (an origin within the scene's own extent does not enlarge the envelope the margins are derived for: a scene of any
    // size can be viewed from inside its bounding cube, the scaled reference view included)
    const double max_origin = std::max(static_cast<double>(PT_CAMERA_MAX_ORIGIN), scene->shared->vertex_extent);
    for (int i = 0; i < 3; ++i)
        if (!(std::fabs(cam->origin[i]) <= max_origin))
            return fail(PT_ERR_UNSUPPORTED, "camera: origin component beyond PT_CAMERA_MAX_ORIGIN (" + std::to_string(PT_CAMERA_MAX_ORIGIN) +
                                                ") and beyond the scene's largest |vertex coordinate|: the culling margins are not derived that far out");
    return PT_OK;
}

// NULL, or an end pose equal to the handle's camera bit for bit: no motion.  Checks everything before it changes anything.
static int scene_set_camera_motion_impl(pt_scene *scene, const pt_camera *end) {
    if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
    if (end) {
        int rc = check_camera(scene, end);
        if (rc != PT_OK) return rc;
        if (scene->has_lens && (rc = check_lens_on(*end, scene->lens)) != PT_OK) return rc;
    }
    if (!end || std::memcmp(end, &view_camera(scene), sizeof *end) == 0) {
        scene->has_motion = false;
        scene->motion_end = pt_camera{};
        return PT_OK;
    }
    if (scene->has_projection) return fail(PT_ERR_UNSUPPORTED, "camera motion: the handle has a non-perspective projection; clear one of the two first");
    const int rc = check_motion(scene, view_camera(scene), scene->has_lens ? &scene->lens : nullptr, *end);
    if (rc != PT_OK) return rc;
    scene->motion_end = *end;
    scene->has_motion = true;
    return PT_OK;
}

static int scene_get_camera_motion_impl(const pt_scene *scene, pt_camera *end, int32_t *is_set) {
    if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
    const bool on = motion_active(scene);
    if (end) *end = on ? scene->motion_end : view_camera(scene);
    if (is_set) *is_set = on ? 1 : 0;
    return PT_OK;
}

static int scene_get_camera_impl(const pt_scene *scene, pt_camera *cam, int32_t *is_set) {
    if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
    if (cam) {
        if (scene->has_camera) {
            *cam = scene->camera;
        } else {   // the reference's fixed camera, main.cpp:126-129
            *cam = kReferenceCamera;
        }
    }
    if (is_set) *is_set = scene->has_camera ? 1 : 0;
    return PT_OK;
}

// NULL or kind perspective: back to the pinhole.  Checks everything before it changes anything.
static int scene_set_projection_impl(pt_scene *scene, const pt_projection *prj) {
    if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
    if (!prj || prj->kind == PT_PROJECTION_PERSPECTIVE) {
        scene->has_projection = false;
        scene->projection = pt_projection{};
        return PT_OK;
    }
    if (prj->kind < PT_PROJECTION_PERSPECTIVE || prj->kind > PT_PROJECTION_EQUIRECTANGULAR)
        return fail(PT_ERR_INVALID_ARGUMENT, "projection: unknown kind " + std::to_string(prj->kind));
    pt_projection p = {prj->kind, 0.0f, 0.0f};   // (the spans of an orthographic view are ignored)
    if (p.kind != PT_PROJECTION_ORTHOGRAPHIC) {
        const double sx = prj->span_x, sy = prj->span_y;
        if (!std::isfinite(prj->span_x) || !std::isfinite(prj->span_y) || !(sx > 0.0) || !(sy > 0.0))
            return fail(PT_ERR_INVALID_ARGUMENT, "projection: span_x and span_y must be finite and positive");
        if (p.kind == PT_PROJECTION_FISHEYE && 0.5 * std::sqrt(sx * sx + sy * sy) > 2.0 * M_PI)
            return fail(PT_ERR_INVALID_ARGUMENT, "projection: the fisheye's corner angle, sqrt(span_x^2 + span_y^2) / 2, exceeds 2 pi");
        if (p.kind == PT_PROJECTION_EQUIRECTANGULAR && (sx > 4.0 * M_PI || sy > 4.0 * M_PI))
            return fail(PT_ERR_INVALID_ARGUMENT, "projection: an equirectangular span exceeds 4 pi");
        p.span_x = prj->span_x;
        p.span_y = prj->span_y;
    }
    if (scene->has_lens) return fail(PT_ERR_UNSUPPORTED, "projection: the handle has a lens; a non-perspective projection has a pinhole only -- clear the lens first");
    if (scene->has_motion) return fail(PT_ERR_UNSUPPORTED, "projection: the handle has a camera motion; a non-perspective projection stands still -- clear the motion first");
    if (p.kind == PT_PROJECTION_ORTHOGRAPHIC) {
        const int rc = check_ortho_on(scene, view_camera(scene));
        if (rc != PT_OK) return rc;
    }
    scene->projection = p;
    scene->has_projection = true;
    return PT_OK;
}

static int scene_get_projection_impl(const pt_scene *scene, pt_projection *prj, int32_t *is_set) {
    if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
    if (prj) *prj = scene->has_projection ? scene->projection : pt_projection{};
    if (is_set) *is_set = scene->has_projection ? 1 : 0;
    return PT_OK;
}

int pt_scene_counts(const pt_scene *scene, int32_t *n_triangles, int32_t *n_materials) {
    if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
    if (n_triangles) *n_triangles = scene->shared->host.n_tri();
    if (n_materials) *n_materials = scene->shared->host.n_mat();
    return PT_OK;
}

int pt_scene_get_triangles(const pt_scene *scene, float *triangles, int32_t *triangle_material) {
    if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
    const pt::HostScene &h = scene->shared->host;
    if (triangles) std::memcpy(triangles, h.tri.data(), h.tri.size() * sizeof(float));
    if (triangle_material) std::memcpy(triangle_material, h.tri_mat.data(), h.tri_mat.size() * sizeof(int32_t));
    return PT_OK;
}

int pt_scene_get_materials(const pt_scene *scene, float *materials) {
    if (!scene || !materials) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    std::memcpy(materials, scene->shared->host.mat.data(), scene->shared->host.mat.size() * sizeof(float));
    return PT_OK;
}

void pt_scene_destroy(pt_scene *s) { delete s; }   // (~pt_scene makes the scene's device current for its owners)

static int render_device_impl(pt_scene *scene, const pt_render_params *p, float *d_sum, float *d_sum2, int32_t *d_count,
                     void *hip_stream, pt_render_stats *stats) {
    const int rc = check_params(scene, p);
    if (rc != PT_OK) return rc;
    if (!d_sum || !d_sum2 || !d_count) return fail(PT_ERR_INVALID_ARGUMENT, "null accumulator pointer");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> ctx_lock(scene->ctx.mutex);
    const int r = enqueue_render(scene, scene->ctx, p, {d_sum, d_sum2, d_count, 0}, stream, stats != nullptr);
    if (r != PT_OK || !stats) return r;
    return collect_stats(scene, scene->ctx, stream, stats);
}

static int trace_rays_host_impl(pt_scene *scene, int32_t n_rays, const float *origins, const float *directions, float eps,
                       int32_t *hit_index, float *hit_t) {
    if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
    if (const int rc = ptc::check_has_device(scene)) return rc;
    if (n_rays < 0 || (n_rays > 0 && (!origins || !directions || !hit_index || !hit_t)))
        return fail(PT_ERR_INVALID_ARGUMENT, "null ray buffer or negative count");
    if (n_rays == 0) return PT_OK;
    PT_HIP_TRY(hipSetDevice(scene->device));
    std::lock_guard<std::mutex> launch_lock(scene->launch_mutex);
    const int crc = ensure_cull(scene, eps);
    if (crc != PT_OK) return crc;
    pt::RenderArgs a;
    fill_scene_args(scene, eps, a);
    ptc::DeviceBuffer d_o, d_d, d_t, d_i;
    const size_t n = static_cast<size_t>(n_rays);
    int rc;
    if ((rc = d_o.alloc(n * 12, "pt_trace_rays_host")) != PT_OK || (rc = d_d.alloc(n * 12, "pt_trace_rays_host")) != PT_OK ||
        (rc = d_t.alloc(n * 4, "pt_trace_rays_host")) != PT_OK || (rc = d_i.alloc(n * 4, "pt_trace_rays_host")) != PT_OK)
        return rc;
    PT_HIP_TRY(hipMemcpy(d_o.get<void>(), origins, n * 12, hipMemcpyHostToDevice));
    PT_HIP_TRY(hipMemcpy(d_d.get<void>(), directions, n * 12, hipMemcpyHostToDevice));
    PT_HIP_TRY(pt::launch_trace_rays(a, d_o.get<float>(), d_d.get<float>(), n_rays, d_i.get<int32_t>(), d_t.get<float>(), nullptr));
    PT_HIP_TRY(hipDeviceSynchronize());
    PT_HIP_TRY(hipMemcpy(hit_index, d_i.get<void>(), n * 4, hipMemcpyDeviceToHost));
    PT_HIP_TRY(hipMemcpy(hit_t, d_t.get<void>(), n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

static int render_host_impl(pt_scene *scene, const pt_render_params *p, float *sum, float *sum2, int32_t *count,
                   pt_render_stats *stats) {
    const int rc = check_params(scene, p);
    if (rc != PT_OK) return rc;
    if (!sum || !sum2 || !count) return fail(PT_ERR_INVALID_ARGUMENT, "null accumulator pointer");
    PT_HIP_TRY(hipSetDevice(scene->device));
    const int rows = ptc::band_rows(p);
    const size_t W = static_cast<size_t>(p->width), n = static_cast<size_t>(rows) * W;
    if (n == 0) {
        if (stats) zero_stats(scene, stats);
        return PT_OK;
    }
    std::lock_guard<std::mutex> host_lock(scene->host_mutex);
    // device band (sum | sum2 | count planes, 256-byte aligned planes), grown on demand and kept
    ptc::PlaneLayout l;
    ptc::AccumPlanes band = ptc::AccumPlanes::in(l, n);
    int r;
    if (scene->d_host_band.bytes() < l.end + 256 && (r = scene->d_host_band.alloc(l.end + 256, "pt_render_host")) != PT_OK) return r;
    if (!scene->host_stream && (r = scene->host_stream.create("pt_render_host")) != PT_OK) return r;
    band.bind(scene->d_host_band);
    // One launch for the whole band between plain synchronous copies.  (Measured and dropped: cutting the band into row
    // slabs so that copies overlap kernels.  A tile's passes run strictly in order, so every launch lasts at least one
    // tile's whole pass chain -- 13.6 ms at 256 spp whatever the slab's height -- and ten slabs took 189 ms where one
    // launch takes 96 ms + 3.4 ms of copies; profiles/r02_host_path_slabs.txt.  hipMemcpyAsync into pageable memory ran
    // at about 1 GB/s here, the synchronous call at PCIe speed.)
    if ((r = band.upload(sum, sum2, count)) != PT_OK) return r;
    if ((r = render_device_impl(scene, p, band.sum, band.sum2, band.count, scene->host_stream.get(), stats)) != PT_OK) return r;
    PT_HIP_TRY(hipStreamSynchronize(scene->host_stream.get()));
    return band.download(sum, sum2, count);
}

static int session_render_impl(pt_session *s, const pt_render_params *p, pt_render_stats *stats) {
    if (!s) return fail(PT_ERR_INVALID_ARGUMENT, "null session or params");
    std::lock_guard<std::mutex> ctx_lock(s->ctx.mutex);
    const int r = ptc::session_enqueue(s, p, stats != nullptr);
    if (r != PT_OK || !stats) return r;
    return ptc::session_collect(s, stats);
}

static int session_read_impl(pt_session *s, float *sum, float *sum2, int32_t *count) {
    if (!s || !sum || !sum2 || !count) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    if (s->n == 0) return PT_OK;
    PT_HIP_TRY(hipSetDevice(s->scene->device));
    // wait for the session's kernels, then plain synchronous copies: the runtime's fast path for pageable destinations
    // (hipMemcpyAsync into pageable memory ran at about 1 GB/s here)
    PT_HIP_TRY(hipStreamSynchronize(s->stream.get()));
    return s->planes.download(sum, sum2, count);
}

static int session_clear_impl(pt_session *s) {
    if (!s) return fail(PT_ERR_INVALID_ARGUMENT, "null session");
    PT_HIP_TRY(hipSetDevice(s->scene->device));
    PT_HIP_TRY(hipMemsetAsync(s->planes.sum, 0, 3 * s->n * sizeof(float), s->stream.get()));
    PT_HIP_TRY(hipMemsetAsync(s->planes.sum2, 0, 3 * s->n * sizeof(float), s->stream.get()));
    PT_HIP_TRY(hipMemsetAsync(s->planes.count, 0, s->n * sizeof(int32_t), s->stream.get()));
    return PT_OK;
}


static int scene_cull_tables_impl(pt_scene *scene, float eps, int32_t *counts, float *clusters, float *spheres, float *bary,
                         float *constants) {
    if (!scene || !counts) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_ptr<const pt::CullTables> tp;
    const int rc = get_cull(*scene->shared, eps, camera_radius(scene), tp);
    if (rc != PT_OK) return rc;
    const pt::CullTables &t = *tp;
    counts[0] = static_cast<int32_t>(t.clusters.size());
    counts[1] = static_cast<int32_t>(t.spheres.size());
    counts[2] = static_cast<int32_t>(t.bary.size());
    int32_t large = 0;
    for (const auto &c : t.clusters)
        if (c.kind == 1) large += static_cast<int32_t>(c.n_tri);
    counts[3] = large;
    if (clusters) std::memcpy(clusters, t.clusters.data(), t.clusters.size() * sizeof(pt::ClusterDesc));
    if (spheres) std::memcpy(spheres, t.spheres.data(), t.spheres.size() * sizeof(pt::SphereRec));
    if (bary) std::memcpy(bary, t.bary.data(), t.bary.size() * sizeof(pt::CullRec));
    if (constants) {
        constants[0] = t.cc.k1; constants[1] = t.cc.k2; constants[2] = t.cc.a_max; constants[3] = t.cc.m0;
        constants[4] = t.cc.t_guard;
    }
    return PT_OK;
}

static int scene_cull_layout_impl(pt_scene *scene, float eps, int32_t *counts, int32_t *slot_triangle, void *bvh_nodes) {
    if (!scene || !counts) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_ptr<const pt::CullTables> tp;
    const int rc = get_cull(*scene->shared, eps, camera_radius(scene), tp);
    if (rc != PT_OK) return rc;
    const pt::CullTables &t = *tp;
    counts[0] = static_cast<int32_t>(t.slot_tri.size());
    counts[1] = static_cast<int32_t>(t.bvh.size());
    counts[2] = static_cast<int32_t>(t.bvh_inner);
    counts[3] = static_cast<int32_t>(t.clusters.size());
    if (slot_triangle)
        for (size_t k = 0; k < t.slot_tri.size(); ++k) slot_triangle[k] = t.slot_tri[k] == pt::kNoTriangle ? -1 : static_cast<int32_t>(t.slot_tri[k]);
    if (bvh_nodes && !t.bvh.empty()) std::memcpy(bvh_nodes, t.bvh.data(), t.bvh.size() * sizeof(pt::BvhNode));
    return PT_OK;
}

}  // extern "C"

// main.cpp:162-185 for the rows [y0, y1): per-pixel variance estimate d (written to contrib: d, or 1 for a pixel without samples,
// main.cpp:165-168), running max / min of d in row order, and the tonemapped pixel through `put`.
template <class Put>
static void resolve_rows(int32_t width, int y0, int y1, const float *sum, const float *sum2, const int32_t *count, float gamma,
                         float *contrib, float &max_d, float &min_d, Put &&put) {
    for (int y = y0; y < y1; ++y) {
        for (int x = 0; x < width; ++x) {
            const size_t p = static_cast<size_t>(y) * width + x;
            if (!count[p]) {   // main.cpp:165-168
                contrib[p] = 1.0f;
                put(p, nullptr);
                continue;
            }
            const float n = static_cast<float>(count[p]);
            float c[3], dd[3];
            for (int k = 0; k < 3; ++k) {
                const float mean = sum[3 * p + k] / n;
                dd[k] = sum2[3 * p + k] / n - mean * mean;
                c[k] = ptc::tonemap_value(sum[3 * p + k] / n, gamma);   // main.cpp:179-182
            }
            const float d = dd[0] + dd[1] + dd[2];
            if (d > max_d) max_d = d;
            if (d < min_d) min_d = d;
            contrib[p] = d;
            put(p, c);
        }
    }
}

// The resolve is the reference's, value for value; only its schedule differs: bands of rows on the host's cores (powf per
// channel is 20 ms of one core at 1080p), then what depends on the pixel ORDER in order -- the bands' max / min combined first
// to last with the reference's own strict comparisons (ties, signed zeros: the first one in pixel order stays), and the float
// sum of the per-pixel terms as one sequential pass.
template <class Put>
static void resolve_all(int32_t width, int32_t height, const float *sum, const float *sum2, const int32_t *count, float gamma,
                        float *dispersion, Put &&put) {
    const size_t n_px = static_cast<size_t>(width) * height;
    std::vector<float> contrib(n_px);
    unsigned n_thr = n_px >= (1u << 18) ? std::min(16u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
    n_thr = std::min<unsigned>(n_thr, static_cast<unsigned>(height));
    std::vector<float> mx(n_thr, 0.0f), mn(n_thr, INFINITY);
    auto band = [&](unsigned t) {
        const int y0 = static_cast<int>(static_cast<long long>(height) * t / n_thr), y1 = static_cast<int>(static_cast<long long>(height) * (t + 1) / n_thr);
        resolve_rows(width, y0, y1, sum, sum2, count, gamma, contrib.data(), mx[t], mn[t], put);
    };
    if (n_thr == 1) {
        band(0);
    } else {
        std::vector<std::thread> th;
        for (unsigned t = 1; t < n_thr; ++t) th.emplace_back(band, t);
        band(0);
        for (auto &t : th) t.join();
    }
    float max_d = 0.0f, min_d = INFINITY, avg_d = 0.0f;
    for (unsigned t = 0; t < n_thr; ++t) {
        if (mx[t] > max_d) max_d = mx[t];
        if (mn[t] < min_d) min_d = mn[t];
    }
    for (size_t p = 0; p < n_px; ++p) avg_d += contrib[p];
    avg_d /= width * height;
    if (dispersion) {
        dispersion[0] = max_d;
        dispersion[1] = min_d;
        dispersion[2] = avg_d;
    }
}

extern "C" {

int pt_resolve(int32_t width, int32_t height, const float *sum, const float *sum2, const int32_t *count, float gamma,
               uint8_t *bgr, float *dispersion) {
    if (width <= 0 || height <= 0 || !sum || !sum2 || !count || !bgr)
        return fail(PT_ERR_INVALID_ARGUMENT, "null buffer or empty image");
    return guarded([&] {
        resolve_all(width, height, sum, sum2, count, gamma, dispersion, [bgr](size_t p, const float *c) {
            if (!c) {   // image.clear(), main.cpp:106: pixels without samples stay black
                bgr[3 * p + 0] = bgr[3 * p + 1] = bgr[3 * p + 2] = 0;
                return;
            }
            // set_pixel(x, y, float, float, float): float -> unsigned char (bitmap_image.hpp:194-206)
            bgr[3 * p + 0] = ptc::quantize_value(c[2]);
            bgr[3 * p + 1] = ptc::quantize_value(c[1]);
            bgr[3 * p + 2] = ptc::quantize_value(c[0]);
        });
        return static_cast<int>(PT_OK);
    });
}

int pt_resolve_float(int32_t width, int32_t height, const float *sum, const float *sum2, const int32_t *count, float gamma,
                     float *rgb, float *dispersion) {
    if (width <= 0 || height <= 0 || !sum || !sum2 || !count || !rgb)
        return fail(PT_ERR_INVALID_ARGUMENT, "null buffer or empty image");
    return guarded([&] {
        resolve_all(width, height, sum, sum2, count, gamma, dispersion, [rgb, sum](size_t p, const float *c) {
            // color_map keeps its raw sums where nothing was counted
            for (int k = 0; k < 3; ++k) rgb[3 * p + k] = c ? c[k] : sum[3 * p + k];
        });
        return static_cast<int>(PT_OK);
    });
}

static int post_filter_host_impl(int device, int32_t width, int32_t height, float *rgb, int32_t gauss, int32_t median) {
    if (width <= 0 || height <= 0 || !rgb) return fail(PT_ERR_INVALID_ARGUMENT, "null buffer or empty image");
    if (gauss < 0 || median < 0) return fail(PT_ERR_INVALID_ARGUMENT, "negative filter size");
    if (median * median / 2 > pt::kMedianMaxRank) return fail(PT_ERR_INVALID_ARGUMENT, "-MEDIAN window larger than 11 is not supported");
    if (!gauss && !median) return PT_OK;
    int rc = ptc::use_device(device, "post filters");
    if (rc != PT_OK) return rc;
    const size_t bytes = static_cast<size_t>(width) * height * 3 * sizeof(float);
    ptc::DeviceBuffer buf_a, buf_b, d_w;
    if ((rc = buf_a.alloc(bytes, "pt_post_filter_host")) != PT_OK || (rc = buf_b.alloc(bytes, "pt_post_filter_host")) != PT_OK) return rc;
    float *d_a = buf_a.get<float>(), *d_b = buf_b.get<float>();   // input and output of the next filter
    PT_HIP_TRY(hipMemcpy(d_a, rgb, bytes, hipMemcpyHostToDevice));
    if (gauss) {   // main.cpp:187-189
        const float r = static_cast<float>(gauss), pi = 3.141593f;
        const int rs = static_cast<int>(std::ceil(r * 2.57));
        const int side = 2 * rs + 1;
        std::vector<float> w(static_cast<size_t>(side) * side);
        for (int dy = -rs; dy <= rs; ++dy)
            for (int dx = -rs; dx <= rs; ++dx) {
                const int dsq = dx * dx + dy * dy;
                w[static_cast<size_t>(dy + rs) * side + (dx + rs)] = std::exp(-dsq / (2 * r * r)) / (pi * 2 * r * r);   // main.cpp:25
            }
        if ((rc = d_w.alloc(w.size() * sizeof(float), "pt_post_filter_host")) != PT_OK) return rc;
        PT_HIP_TRY(hipMemcpy(d_w.get<void>(), w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
        PT_HIP_TRY(pt::launch_gauss(d_a, d_b, d_w.get<float>(), width, height, rs, nullptr));
        std::swap(d_a, d_b);
    }
    if (median) {   // main.cpp:190-192
        PT_HIP_TRY(pt::launch_median(d_a, d_b, width, height, median, nullptr));
        std::swap(d_a, d_b);
    }
    PT_HIP_TRY(hipDeviceSynchronize());
    PT_HIP_TRY(hipMemcpy(rgb, d_a, bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_tonemap(int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float gamma, float *rgb) {
    if (width <= 0 || height <= 0 || !mean_rgb || !count || !rgb) return fail(PT_ERR_INVALID_ARGUMENT, "null buffer or empty image");
    const size_t n = static_cast<size_t>(width) * height;
    for (size_t p = 0; p < n; ++p)
        for (int k = 0; k < 3; ++k)   // main.cpp:179-182
            rgb[3 * p + k] = count[p] ? ptc::tonemap_value(mean_rgb[3 * p + k], gamma) : mean_rgb[3 * p + k];
    return PT_OK;
}

int pt_quantize(int32_t width, int32_t height, const float *rgb, const int32_t *count, uint8_t *bgr) {
    if (width <= 0 || height <= 0 || !rgb || !count || !bgr) return fail(PT_ERR_INVALID_ARGUMENT, "null buffer or empty image");
    const size_t n = static_cast<size_t>(width) * height;
    std::memset(bgr, 0, n * 3);
    for (size_t p = 0; p < n; ++p) {   // main.cpp:193-201: only pixels with samples are written
        if (!count[p]) continue;
        bgr[3 * p + 0] = ptc::quantize_value(rgb[3 * p + 2]);
        bgr[3 * p + 1] = ptc::quantize_value(rgb[3 * p + 1]);
        bgr[3 * p + 2] = ptc::quantize_value(rgb[3 * p + 0]);
    }
    return PT_OK;
}

int pt_write_bmp(const char *path, int32_t width, int32_t height, const uint8_t *bgr) {
    if (!path || width <= 0 || height <= 0 || !bgr) return fail(PT_ERR_INVALID_ARGUMENT, "null argument or empty image");
    FILE *f = std::fopen(path, "wb");
    if (!f) return fail(PT_ERR_IO, std::string("cannot open ") + path + " for writing");
    const uint32_t row_bytes = static_cast<uint32_t>(width) * 3u;
    const uint32_t size_image = ((row_bytes + 3u) & 0x0000FFFCu) * static_cast<uint32_t>(height);   // sic: 16-bit mask
    uint8_t hdr[54];
    std::memset(hdr, 0, sizeof hdr);
    auto put32 = [&](int at, uint32_t v) { for (int i = 0; i < 4; ++i) hdr[at + i] = static_cast<uint8_t>(v >> (8 * i)); };
    auto put16 = [&](int at, uint16_t v) { hdr[at] = static_cast<uint8_t>(v); hdr[at + 1] = static_cast<uint8_t>(v >> 8); };
    put16(0, 19778);
    put32(2, 54u + size_image);
    put32(10, 54u);
    put32(14, 40u);
    put32(18, static_cast<uint32_t>(width));
    put32(22, static_cast<uint32_t>(height));
    put16(26, 1);
    put16(28, 24);
    put32(34, size_image);
    bool ok = std::fwrite(hdr, 1, sizeof hdr, f) == sizeof hdr;
    const uint32_t pad = (4u - row_bytes % 4u) % 4u;
    const uint8_t zeros[4] = {0, 0, 0, 0};
    for (int i = 0; ok && i < height; ++i) {
        ok = std::fwrite(bgr + static_cast<size_t>(height - i - 1) * row_bytes, 1, row_bytes, f) == row_bytes;
        if (ok && pad) ok = std::fwrite(zeros, 1, pad, f) == pad;
    }
    ok = (std::fclose(f) == 0) && ok;
    return ok ? PT_OK : fail(PT_ERR_IO, std::string("short write to ") + path);
}

// ---- the guarded entry points (definitions above are the bodies) ----

int pt_scene_load_obj(const char *model_dir, const char *model_name, int device, pt_scene **out) {
    return guarded([&] { return scene_load_obj_impl(model_dir, model_name, device, 0u, out); });
}

int pt_scene_load_obj_ex(const char *model_dir, const char *model_name, int device, uint32_t flags, pt_scene **out) {
    return guarded([&] { return scene_load_obj_impl(model_dir, model_name, device, flags, out); });
}

int pt_scene_create(const float *triangles, const int32_t *triangle_material, int32_t n_triangles, const float *materials, int32_t n_materials, int device, pt_scene **out) {
    return guarded([&] { return scene_create_impl(triangles, triangle_material, n_triangles, materials, n_materials, device, out); });
}

int pt_scene_clone_to_device(const pt_scene *scene, int device, pt_scene **out) {
    return guarded([&] { return scene_clone_impl(scene, device, out); });
}

int pt_scene_set_skybox_bmp(pt_scene *scene, const char *path) {
    return guarded([&] { return scene_set_skybox_bmp_impl(scene, path); });
}

int pt_camera_look_at(const float eye[3], const float target[3], const float up[3], float fov_y_degrees, float aspect, pt_camera *out) {
    return guarded([&] { return camera_look_at_impl(eye, target, up, fov_y_degrees, aspect, out); });
}

int pt_scene_set_camera(pt_scene *scene, const pt_camera *camera) {
    return guarded([&] {
        if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
        std::lock_guard<std::mutex> launch_lock(scene->launch_mutex);   // (a launch being enqueued reads the camera under it)
        return scene_set_camera_impl(scene, camera);
    });
}

int pt_scene_get_camera(const pt_scene *scene, pt_camera *camera, int32_t *is_set) {
    return guarded([&] { return scene_get_camera_impl(scene, camera, is_set); });
}

int pt_scene_set_lens(pt_scene *scene, const pt_lens *lens) {
    return guarded([&] {
        if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
        std::lock_guard<std::mutex> launch_lock(scene->launch_mutex);   // (a launch being enqueued reads the lens under it)
        return scene_set_lens_impl(scene, lens);
    });
}

int pt_scene_get_lens(const pt_scene *scene, pt_lens *lens, int32_t *is_set) {
    return guarded([&] { return scene_get_lens_impl(scene, lens, is_set); });
}

int pt_scene_set_camera_motion(pt_scene *scene, const pt_camera *end) {
    return guarded([&] {
        if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
        std::lock_guard<std::mutex> launch_lock(scene->launch_mutex);   // (a launch being enqueued reads the motion under it)
        return scene_set_camera_motion_impl(scene, end);
    });
}

int pt_scene_get_camera_motion(const pt_scene *scene, pt_camera *end, int32_t *is_set) {
    return guarded([&] { return scene_get_camera_motion_impl(scene, end, is_set); });
}

int pt_projection_make(int32_t kind, float fov_y_degrees, float aspect, pt_projection *out) {
    return guarded([&] { return projection_make_impl(kind, fov_y_degrees, aspect, out); });
}

int pt_camera_ortho(const float eye[3], const float target[3], const float up[3], float view_height, float aspect, pt_camera *out) {
    return guarded([&] { return camera_ortho_impl(eye, target, up, view_height, aspect, out); });
}

int pt_scene_set_projection(pt_scene *scene, const pt_projection *projection) {
    return guarded([&] {
        if (!scene) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
        std::lock_guard<std::mutex> launch_lock(scene->launch_mutex);   // (a launch being enqueued reads the projection under it)
        return scene_set_projection_impl(scene, projection);
    });
}

int pt_scene_get_projection(const pt_scene *scene, pt_projection *projection, int32_t *is_set) {
    return guarded([&] { return scene_get_projection_impl(scene, projection, is_set); });
}

int pt_render_device(pt_scene *scene, const pt_render_params *p, float *d_sum, float *d_sum2, int32_t *d_count, void *hip_stream, pt_render_stats *stats) {
    return guarded([&] { return render_device_impl(scene, p, d_sum, d_sum2, d_count, hip_stream, stats); });
}

int pt_trace_rays_host(pt_scene *scene, int32_t n_rays, const float *origins, const float *directions, float eps, int32_t *hit_index, float *hit_t) {
    return guarded([&] { return trace_rays_host_impl(scene, n_rays, origins, directions, eps, hit_index, hit_t); });
}

int pt_render_host(pt_scene *scene, const pt_render_params *p, float *sum, float *sum2, int32_t *count, pt_render_stats *stats) {
    return guarded([&] { return render_host_impl(scene, p, sum, sum2, count, stats); });
}

int32_t pt_band_rows(const pt_render_params *params) { return params ? ptc::band_rows(params) : 0; }

int pt_session_create_strided(pt_scene *scene, int32_t width, int32_t height, int32_t row_begin, int32_t row_end, int32_t row_stride,
                              pt_session **out) {
    return guarded([&] { return ptc::session_create_on(scene, width, height, row_begin, row_end, nullptr, out, row_stride); });
}

int pt_session_create(pt_scene *scene, int32_t width, int32_t height, int32_t row_begin, int32_t row_end, pt_session **out) {
    return guarded([&] { return ptc::session_create_on(scene, width, height, row_begin, row_end, nullptr, out, 1); });
}

int pt_session_render(pt_session *session, const pt_render_params *params, pt_render_stats *stats) {
    return guarded([&] { return session_render_impl(session, params, stats); });
}

int pt_session_wait(pt_session *session) {
    return guarded([&] {
        if (!session) return fail(PT_ERR_INVALID_ARGUMENT, "null session");
        PT_HIP_TRY(hipSetDevice(session->scene->device));
        PT_HIP_TRY(hipStreamSynchronize(session->stream.get()));
        return static_cast<int>(PT_OK);
    });
}

int pt_session_read(pt_session *session, float *sum, float *sum2, int32_t *count) {
    return guarded([&] { return session_read_impl(session, sum, sum2, count); });
}

int pt_session_clear(pt_session *session) {
    return guarded([&] { return session_clear_impl(session); });
}

void pt_session_destroy(pt_session *s) { delete s; }   // (~pt_session: the scene's device current, the stream drained)

int pt_scene_cull_tables(pt_scene *scene, float eps, int32_t *counts, float *clusters, float *spheres, float *bary, float *constants) {
    return guarded([&] { return scene_cull_tables_impl(scene, eps, counts, clusters, spheres, bary, constants); });
}

int pt_scene_cull_layout(pt_scene *scene, float eps, int32_t *counts, int32_t *slot_triangle, void *bvh_nodes) {
    return guarded([&] { return scene_cull_layout_impl(scene, eps, counts, slot_triangle, bvh_nodes); });
}

int pt_post_filter_host(int device, int32_t width, int32_t height, float *rgb, int32_t gauss, int32_t median) {
    return guarded([&] { return post_filter_host_impl(device, width, height, rgb, gauss, median); });
}

#ifdef PT_TEST_HOOKS
// Test build only (libpt_testhooks.so).  family: "sphere_r2", "m0", "k12", "a_max", "quad_slack" (scale on that family of
// conservative margins; 1 = as shipped), "no_absorb" (0/1), "reset".  Affects scenes whose cull tables are built afterwards.
// Scheduler / instantiation choices of launches enqueued afterwards: "items_per_slot" (n > 0: equal pass chunks, about n work items
// per wave slot; < 0: the 3/4 - of - the - rest chunks always; 0: the library's rule), "chunk_min" (the smallest last chunk of that
// scheme), "tile_width" (1: 8 x 8 tiles always; 2: 16 x 8 where the instantiation has them, batches over 16 x 8 tiles for adaptive
// launches; 3: the same with 32 x 8 batch tiles; 0: by tile count), "regen_min_dead" (path regeneration threshold), "no_room_kernel"
// (1: a room-shaped scene, CullTables::room, runs the generic kernel too; 0: the room kernel).
// Test builds only: the box tree's child test (pt_kernels.hip: box_children_kept) on n caller-supplied items -- nodes:
// n x 64 bytes (BvhNode), rays: n x 6 floats (origin, unit direction), t_best: n floats -- out: n masks, one per item.
// Host pointers; device 0.
int pt_test_box_masks(const void *nodes, const float *rays, const float *t_best, float err, int32_t n, uint32_t *out) {
    if (!nodes || !rays || !t_best || !out || n < 0) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return PT_OK;
    PT_HIP_TRY(hipSetDevice(0));
    ptc::DeviceBuffer d_nodes, d_rays, d_t, d_out;
    const size_t nn = static_cast<size_t>(n);
    int rc;
    if ((rc = d_nodes.alloc(nn * 64, "pt_test_box_masks")) != PT_OK || (rc = d_rays.alloc(nn * 24, "pt_test_box_masks")) != PT_OK ||
        (rc = d_t.alloc(nn * 4, "pt_test_box_masks")) != PT_OK || (rc = d_out.alloc(nn * 4, "pt_test_box_masks")) != PT_OK)
        return rc;
    PT_HIP_TRY(hipMemcpy(d_nodes.get<void>(), nodes, nn * 64, hipMemcpyHostToDevice));
    PT_HIP_TRY(hipMemcpy(d_rays.get<void>(), rays, nn * 24, hipMemcpyHostToDevice));
    PT_HIP_TRY(hipMemcpy(d_t.get<void>(), t_best, nn * 4, hipMemcpyHostToDevice));
    PT_HIP_TRY(pt::launch_box_masks(d_nodes.get<pt::BvhNode>(), d_rays.get<float>(), d_t.get<float>(), err, n, d_out.get<uint32_t>(), nullptr));
    PT_HIP_TRY(hipDeviceSynchronize());
    PT_HIP_TRY(hipMemcpy(out, d_out.get<void>(), nn * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

long pt_test_live_device_objects(void) { return ptc::g_live_device_objects.load(std::memory_order_relaxed); }

// The kernel the last enqueued integrator launch took, as the plan names it: plan::variant_id (pt_launch_plan.hpp; the two room
// kernels are kAllVariants = 120, wide, and 121, narrow), -1 before the first launch.
int pt_test_last_variant(void) { return g_last_variant.load(std::memory_order_relaxed); }

int pt_test_set_mutation(const char *family, double value) {
    if (!family) return PT_ERR_INVALID_ARGUMENT;
    const std::string f = family;
    pt::CullMutation &m = pt::g_cull_mutation;
    if (f == "reset") { m = pt::CullMutation(); g_plan_overrides = pt::plan::Overrides(); }
    else if (f == "regen_min_dead") g_plan_overrides.regen_min_dead = static_cast<int>(value);
    else if (f == "chunk_min") g_plan_overrides.chunk_min = static_cast<int>(value);
    else if (f == "sphere_r2") m.sphere_r2 = value;
    else if (f == "m0") m.m0 = value;
    else if (f == "k12") m.k12 = value;
    else if (f == "a_max") m.a_max = value;
    else if (f == "quad_slack") m.quad_slack = value;
    else if (f == "box") m.box = value;
    else if (f == "box_err") m.box_err = value;
    else if (f == "no_absorb") m.no_absorb = value != 0;
    else if (f == "no_last_segment_filter") m.no_last_segment_filter = value != 0;
    else if (f == "emis_drop") m.emis_drop = value != 0;
    else if (f == "order_mode") m.order_mode = static_cast<int>(value);
    else if (f == "bvh_fill") m.bvh_fill = value;
    else if (f == "bvh_mode") m.bvh_mode = static_cast<int>(value);
    else if (f == "bvh_depth_cap") m.bvh_depth_cap = static_cast<int>(value);
    else if (f == "big_threshold") m.big_threshold = static_cast<int>(value);
    else if (f == "max_clusters") m.max_clusters = static_cast<int>(value);
    else if (f == "items_per_slot") g_plan_overrides.items_per_slot = static_cast<int>(value);
    else if (f == "tile_width") g_plan_overrides.tile_width = static_cast<int>(value);
    else if (f == "no_room_kernel") g_plan_overrides.no_room_kernel = value != 0;
    else return fail(PT_ERR_INVALID_ARGUMENT, "unknown mutation family " + f);
    return PT_OK;
}
#endif

}  // extern "C"
