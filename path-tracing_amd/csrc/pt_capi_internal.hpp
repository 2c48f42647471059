// What the translation units behind the C ABI share: the handles' types, the checks and the setter skeletons whose message every entry
// point shares, each stage's parameters into its launch arguments, the plane views of pt_device_mem.hpp -- the owners of everything held
// on a device -- into the same arguments, and the timed region of a one-shot entry point.
// Nothing here is part of the ABI.
#pragma once
#include "../../include/pt_hip.h"

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "pt_bloom.hpp"
#include "pt_colour.hpp"
#include "pt_denoise.hpp"
#include "pt_environment.hpp"
#include "pt_device_mem.hpp"
#include "pt_grade.hpp"
#include "pt_grain.hpp"
#include "pt_kernels.hpp"
#include "pt_linear.hpp"
#include "pt_local.hpp"
#include "pt_meter.hpp"
#include "pt_optics.hpp"
#include "pt_direct.hpp"
#include "pt_envdirect.hpp"
#include "pt_roulette.hpp"
#include "pt_rough.hpp"
#include "pt_scene.hpp"
#include "pt_sharpen.hpp"
#include "pt_smooth.hpp"
#include "pt_texture.hpp"
#include "pt_upsample.hpp"

// The host side of a scene: parsed model, its device-independent tables and the culling hierarchies built so far (one per
// eps).  Immutable once the scene is finished and shared by every per-device copy of it (pt_scene_clone_to_device, pt_frame):
// the OBJ is parsed once and the hierarchy built once per (scene, eps), however many devices render it.
struct pt_scene_host {
    pt::HostScene host;
    pt::DeviceTables tables;
    std::mutex cull_mutex;
    std::vector<std::shared_ptr<const pt::CullTables>> cull_cache;   // most recent last; a handful of eps values at most
    double load_seconds = 0;                                         // parsing + per-triangle tables
    double cull_build_seconds = 0;                                   // host time spent in build_cull_tables (pt_render -TIMING)
    double vertex_extent = 0;                                        // largest |vertex coordinate| (the cull envelope's key)
};

// Skybox texels (B,G,R; top-down rows; no padding).  A skybox belongs to a pt_scene handle, not to the shared model: a per-device
// copy inherits the one of the handle it was made FROM (the pointer is copied; texels are immutable once set).
struct pt_sky_texels {
    std::vector<uint8_t> texels;
    int w = 0, h = 0;
};

// The environment of a handle (pt_hip.h: pt_environment_*): the octahedral map, n x n x 3 floats as given or converted.  Belongs to
// the handle as the skybox does; immutable once set.
struct pt_env_map {
    std::vector<float> rgb;
    int n = 0;
};

// The dielectrics of a handle (pt_hip.h: pt_dielectric): the list as given and the per-material table the kernels read
// (pt_kernels.hpp: GlassRec, one per material of the scene).  Belongs to the handle as the environment does; immutable once set.
struct pt_glass_list {
    std::vector<pt_dielectric> list;
    std::vector<pt::GlassRec> table;
};

// The textures of a handle (pt_hip.h: pt_texture): the list as given (with its texels) and what the kernels read -- the per-material
// table (pt_texture.hpp: TexRec, one per material of the scene) and the pool of all the list's texels.  Belongs to the handle as the
// dielectrics do; immutable once set.  The handle's texture coordinates (6 floats per triangle) are a vector of their own, shared likewise.
struct pt_texture_list {
    struct Entry {
        int32_t material, width, height, filter;
        std::vector<float> rgb;
    };
    std::vector<Entry> list;
    std::vector<pt::TexRec> recs;
    std::vector<pt::TexTexel> pool;
};

// The roughness list of a handle (pt_hip.h: rough specular): the list as given and the per-material table the kernels read (one alpha
// per material of the scene, 0 = the mirror).  Belongs to the handle as the dielectrics do; immutable once set.
struct pt_rough_list {
    std::vector<pt_rough> list;
    std::vector<float> table;
};

// The light table of a handle with direct lighting on (pt_hip.h: direct lighting): the lights in the original triangle order and the
// total area A.  Belongs to the handle as the roughness list does; immutable once built (a handle's triangles and materials never change).
struct pt_light_table {
    std::vector<pt::LightRec> lights;
    float area = 0.0f;
};

// The environment sampling of a handle with that switch on (pt_hip.h: environment sampling): the alias table of the handle's environment,
// the share in use, what the setter was given, and the scene's light table (empty: no emitters, share 1).  Immutable once built; a new
// environment makes a new one.
struct pt_env_sampler {
    std::vector<pt::EnvAliasRec> records;
    int cells = 0;                    // S
    float share = 1.0f;
    pt_env_sampling given{};
    double phi_env = 0.0;
    std::shared_ptr<const pt_light_table> lights;
};

// The tables of a handle that the integrator reads only where a ray has hit a surface.  The host side: each
// nullptr = none, immutable once set, and a copy of the handle inherits all of them (a loaded scene has the OBJ's texcoords).
struct SurfaceTables {
    std::shared_ptr<const pt_glass_list> glass;              // dielectrics
    std::shared_ptr<const std::vector<float>> texcoords;     // 6 floats per triangle
    std::shared_ptr<const pt_texture_list> textures;         // only with texcoords
    std::shared_ptr<const std::vector<float>> smooth;        // shading normals, 9 floats per triangle
    std::shared_ptr<const pt_rough_list> rough;
    std::shared_ptr<const pt_light_table> direct;            // the light table: direct lighting is on
    std::shared_ptr<const pt_env_sampler> envdirect;         // the alias table: environment sampling is on
    // Russian roulette (pt_hip.h: Russian roulette): rr_start > 0 = on, only while direct or envdirect is set.  No table and nothing on
    // the device: the two numbers travel in the kernel arguments.
    int32_t rr_start = 0;
    float rr_floor = 0.0f;
};
// The same on the handle's device: one buffer per table that is set, and what stands in for the absent ones below the highest that is
// set (bind_surface) -- the barycentrics' record of every triangle (pt_texture.hpp: TexBary), which every unit from the texture
// kernels up reads, and all-zero tables: no material is a dielectric, none is textured, every Ns is N, every glossy lobe is the mirror.
// The stand-ins depend on the scene's immutable tables alone: each is uploaded once, when first needed, and never replaced.
struct DeviceSurface {
    ptc::DeviceBuffer glass, tex_recs, tex_uv, tex_texels, normals, alpha, lights;
    ptc::DeviceBuffer env_alias, env_lights;   // environment sampling: its table and its own copy of the light table (one all-zero record where the scene has no emitter)
    ptc::DeviceBuffer bary, no_glass, no_tex, no_normals, no_alpha;
};

// Device copy of one CullTables (they depend on eps and on the envelope the camera needs; a scene keeps the one of its last
// render).
struct DeviceCull {
    float eps = 0;
    double r_max = 0;   // CullTables::r_max
    bool valid = false;
    std::shared_ptr<const pt::CullTables> host;
    ptc::DeviceBuffer clusters, spheres, bary, bary_all, exact_slot, bvh;   // (bary_all, bvh: empty where the host table is)
};

// What one stream of launches needs besides the scene: the scheduler words of the integrator (ticket + per-tile chunk
// counters), the statistics block and the timing events.  Every pt_session owns one, so that sessions of ONE scene (row bands
// of a frame on one device) run concurrently; a scene has one of its own for pt_render_device / pt_render_host.
struct LaunchCtx {
    ptc::DeviceBuffer d_sched, d_stats;   // d_sched grows on demand
    ptc::DeviceEvent ev0, ev1, ev_done;
    bool has_prev = false;          // launches of one context are ordered on the device: they share its scheduler words
    hipStream_t prev_stream = nullptr;
    uint32_t last_chunks = 0;       // of the last launch enqueued (reported with its statistics)
    bool stats_pending = false;
    std::mutex mutex;               // one call at a time per context (enqueue + the optional wait for statistics)
};

struct pt_scene {
    std::shared_ptr<pt_scene_host> shared;
    int device = -1;
    DeviceCull cull;
    ptc::DeviceBuffer d_exact, d_mats;
    int cu_count = 256;            // compute units of the scene's device
    std::shared_ptr<const pt_sky_texels> sky;   // this handle's skybox (nullptr = none); copies made from it inherit it
    ptc::DeviceBuffer d_sky;       // the same texels on this copy's device
    int sky_w = 0, sky_h = 0;
    std::shared_ptr<const pt_env_map> env;      // this handle's environment (nullptr = none; never with a skybox); copies inherit it
    ptc::DeviceBuffer d_env;       // its (n + 2)^2 texels with the apron (pt_environment.hpp: EnvTexel) on this copy's device
    SurfaceTables surface;         // this handle's dielectrics, textures, shading normals, roughness list and light table; copies inherit them
    DeviceSurface d_surface;       // the same on this copy's device
    bool has_camera = false;       // this handle's camera (pt_scene_set_camera); copies made from it inherit it
    pt_camera camera{};
    bool has_lens = false;         // this handle's lens (pt_scene_set_lens; radius > 0); copies made from it inherit it
    pt_lens lens{};
    bool has_motion = false;       // this handle's camera motion (pt_scene_set_camera_motion): the END pose; copies inherit it
    pt_camera motion_end{};
    bool has_projection = false;   // this handle's projection (pt_scene_set_projection; a kind other than perspective); copies inherit it
    pt_projection projection{};
    // ensure_cull + the enqueue of a launch happen under launch_mutex (a concurrent render with another eps must not free
    // the tables in between); nothing waits for the device while holding it.
    std::mutex launch_mutex;
    LaunchCtx ctx;                 // pt_render_device / pt_render_host / pt_trace_rays_host
    // pt_render_host: device band kept between calls + the stream its kernel runs on (guarded by host_mutex)
    std::mutex host_mutex;
    ptc::DeviceBuffer d_host_band;
    ptc::DeviceStream host_stream;
    // Everything above is freed with the scene's device current; a scene without one holds nothing and makes no HIP call.
    ~pt_scene() {
        if (device >= 0) (void)hipSetDevice(device);
    }
};

// A row band's accumulators kept on the device between pass slices (pt_session_*).
struct pt_session {
    pt_scene *scene = nullptr;
    int32_t width = 0, height = 0, row_begin = 0, row_end = 0, row_stride = 1;
    size_t n = 0;                 // pixels of the band
    LaunchCtx ctx;
    ptc::DeviceBuffer d_band;     // owned: sum[3n] | sum2[3n] | count[n], each plane 256-byte aligned; empty if the planes are borrowed
    ptc::AccumPlanes planes;      // in d_band, or in the frame's planes
    ptc::DeviceStream stream;
    ~pt_session() {               // the stream drains, then it, the band and the context go, on the scene's device
        (void)hipSetDevice(scene->device);
        if (stream) (void)hipStreamSynchronize(stream.get());
    }
};

// A 3D LUT (pt_lut_create, pt_lut_load_cube): immutable once made.  No two LUTs of a process share a generation, so a display
// knows from the number alone whether its device copy is this one.
struct pt_lut {
    int32_t n = 0;
    uint64_t generation = 0;
    std::vector<pt::LutVertex> vertices;   // n^3, red index fastest
};

namespace ptc {

int fail(int code, const std::string &msg);
int hip_fail(hipError_t e, const char *what);
#define PT_HIP_TRY(expr)                                       \
    do {                                                       \
        hipError_t e_ = (expr);                                \
        if (e_ != hipSuccess) return ptc::hip_fail(e_, #expr); \
    } while (0)

// No exception may cross the C boundary: allocation failures and anything else become status codes.
template <class F>
int guarded(F &&f) noexcept {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return fail(PT_ERR_OUT_OF_MEMORY, "out of host memory");
    } catch (const std::exception &e) {
        return fail(PT_ERR_INVALID_ARGUMENT, std::string("internal error: ") + e.what());
    } catch (...) {
        return fail(PT_ERR_INVALID_ARGUMENT, "internal error");
    }
}

// A timed region of a one-shot entry point: the two events made, begin recorded on `stream`, what `enqueue` puts there (it answers
// a status; a failure is returned as it is, with no end recorded and no wait), end recorded, the wait, the milliseconds between.
// The events go with the call.  (The texts are those of the entry points that spelled this out, each on the null stream.)
template <class F>
int timed(hipStream_t stream, const char *what, float *ms, F &&enqueue) {
    DeviceTimer timer;
    int rc = timer.create(what);
    if (rc != PT_OK) return rc;
    if (const hipError_t e = timer.begin(stream)) return hip_fail(e, "timer.begin(nullptr)");
    if ((rc = enqueue()) != PT_OK) return rc;
    if (const hipError_t e = timer.end(stream)) return hip_fail(e, "timer.end(nullptr)");
    if (const hipError_t e = timer.wait_ms(ms)) return hip_fail(e, "timer.wait_ms(&ms)");
    return PT_OK;
}

// The two checks whose text every stage shares: `prefix` names the stage ("bloom: "), `tail` is what a handle's creation adds.
inline int check_image_size(int32_t width, int32_t height, const char *prefix = "") {
    if (static_cast<long long>(width) * height > 0x7fffffffLL / 4) return fail(PT_ERR_INVALID_ARGUMENT, std::string(prefix) + "image too large");
    return PT_OK;
}
inline int check_has_device(const pt_scene *scene, const char *tail = "") {
    if (scene->device < 0) return fail(PT_ERR_NO_DEVICE, std::string("scene was created without a device (device < 0)") + tail);
    return PT_OK;
}

int check_params(const pt_scene *scene, const pt_render_params *p);
// A session whose planes live in memory the caller owns (the root band of a frame renders straight into the frame's planes).
int session_create_on(pt_scene *scene, int32_t width, int32_t height, int32_t row_begin, int32_t row_end, const AccumPlanes *borrowed,
                      pt_session **out, int32_t row_stride = 1);
// rows the accumulator planes of a call hold (pt_band_rows)
int32_t band_rows(const pt_render_params *p);
// pt_session_render in two halves: enqueue the slice (never waits for the device), then -- if statistics were asked for --
// wait for it and read them.  A frame enqueues on every device before it waits on any.
int session_enqueue(pt_session *s, const pt_render_params *p, bool want_stats);
int session_collect(pt_session *s, pt_render_stats *stats);
// The camera primary rays are made from: the handle's, or the reference's fixed one.
const pt_camera &view_camera(const pt_scene *s);
// The scene part of the kernel arguments for `eps` (uploads the culling hierarchy on first use).  The scene's device is
// current and the caller holds scene->launch_mutex until its kernels are enqueued.
int scene_trace_args(pt_scene *scene, float eps, pt::RenderArgs &a);
// The view's first hits for `rows` rows from `row_begin`: centre rays through `camera`, the closest-hit search with `a`
// (scene_trace_args), the hit's features.  Enqueued on `stream`; the caller still holds scene->launch_mutex.
int enqueue_first_hits(pt_scene *scene, const pt::RenderArgs &a, const pt_camera &camera, int32_t width, int32_t height, int32_t row_begin,
                       int32_t rows, const FeaturePlanes &out, hipStream_t stream);
// Makes `device` current if it is an ordinal of a visible device; PT_ERR_NO_DEVICE otherwise (`stage` names the caller in the message).
int use_device(int device, const char *stage);
// pt_denoise_params as pt_denoise_host checks them, into the parameter fields of the launch arguments (zero = the default).
int denoise_params_to_args(const pt_denoise_params *prm, pt::DenoiseArgs &a);
// The planes a launch reads and writes, from their views: the one place each argument struct's pointers are spelled.
inline void bind_planes(pt::DenoiseArgs &a, const AccumPlanes &in, const FeaturePlanes &f, const DenoisePlanes &w) {
    a.sum = in.sum; a.sum2 = in.sum2; a.count = in.count;
    a.position = f.position; a.normal = f.normal; a.albedo = f.albedo; a.hit_index = f.hit;
    a.rec_a0 = w.rec_a0; a.rec_a1 = w.rec_a1; a.rec_b = w.rec_b; a.rec_c = w.rec_c;
    a.mean_rgb = w.out.rgb; a.count_out = w.out.count;
}
inline void bind_planes(pt::UpsampleArgs &a, const float *mean_lo, const int32_t *count_lo, const FeaturePlanes &f, const UpsamplePlanes &w,
                        const MeanPlanes &out) {
    a.mean_lo = mean_lo; a.count_lo = count_lo;
    a.position = f.position; a.normal = f.normal; a.albedo = f.albedo; a.hit_index = f.hit;
    a.rec_a = w.rec_a; a.rec_b = w.rec_b; a.rec_c = w.rec_c;
    a.mean_rgb = out.rgb; a.count_out = out.count;
}
// levels = 0 of pt_denoise_host: mean_rgb = sum / n (sum where n = 0), count_out = count (may be NULL), on the host.
void unfiltered_mean(size_t n, const float *sum, const int32_t *count, float *mean_rgb, int32_t *count_out);
// pt_upsample_params and the OUTPUT size as pt_upsample_host checks them (no device is touched), into the parameter fields of the
// launch arguments (zero = the default).
int upsample_params_to_args(const pt_upsample_params *prm, int32_t width, int32_t height, pt::UpsampleArgs &a);

// main.cpp:179-182 for one channel, and set_pixel's float -> unsigned char (bitmap_image.hpp:194-206): the ONE spelling of the
// two steps, shared by pt_resolve, pt_tonemap, pt_quantize and the display path, whose threshold table is made from them.
inline float tonemap_value(float mean, float gamma) { return std::pow(mean, gamma) * 255.0f; }
inline uint8_t quantize_value(float value) { return static_cast<uint8_t>(static_cast<int>(value)); }

// pt_grade_params as every entry point checks them (no device is touched), with the defaults filled in.
struct GradeSetup {
    int curve = pt::kCurveReference;
    bool automatic = false;
    float exposure = 1.0f;   // the manual e
    pt::ExposureRule rule{};
};
int grade_params_check(const pt_grade_params *g, GradeSetup &out);

// pt_bloom_params as every entry point checks them (no device is touched), with the defaults filled in (pt_bloom_capi.cpp).
struct BloomSetup {
    bool on = false;          // strength > 0: the stage runs
    float threshold = 1.0f;   // T
    int levels = 5;           // L
    float weight = 0.0f;      // strength / (float)L
};
int bloom_params_check(const pt_bloom_params *b, BloomSetup &out);

// pt_local_params as every entry point checks them (no device is touched), with the defaults filled in (pt_local_capi.cpp).
struct LocalSetup {
    bool on = false;          // strength > 0: the stage runs
    float strength = 0.0f;    // c
    float pivot = 0.18f;
    int levels = 5;           // L
    float sigma = 0.5f;
};
int local_params_check(const pt_local_params *l, LocalSetup &out);

// pt_colour_params as every entry point checks them (no device is touched): M composed, and the LUT's vertices in host memory
// (pt_colour_capi.cpp).  `step.lut` points into *lut, which the caller of the entry point keeps alive.
struct ColourSetup {
    bool on = false;          // M is not the identity, or there is a LUT: the stage runs
    pt::ColourStep step{};
    const pt_lut *lut = nullptr;
};
int colour_params_check(const pt_colour_params *c, ColourSetup &out);

// pt_optics_params as every entry point checks them (no device is touched), with the channels' magnifications composed
// (pt_optics_capi.cpp).
struct OpticsSetup {
    bool on = false;          // any field is not zero: the stage runs
    float k1 = 0.0f, k2 = 0.0f;
    float mag[3] = {1.0f, 1.0f, 1.0f};   // 1 - ca, 1, 1 + ca
    float vignette = 0.0f;
};
int optics_params_check(const pt_optics_params *o, OpticsSetup &out);

// pt_sharpen_params as every entry point checks them (no device is touched), with the default filled in (pt_sharpen_capi.cpp).
struct SharpenSetup {
    bool on = false;          // strength > 0: the stage runs
    float strength = 0.0f;
    float limit = pt::kSharpenMaxLimit;
};
int sharpen_params_check(const pt_sharpen_params *s, SharpenSetup &out);

// pt_grain_params as every entry point checks them (no device is touched), with the default pitch filled in (pt_grain_capi.cpp).
// `step.width` is the caller's to set.
struct GrainSetup {
    bool on = false;          // strength > 0 or dither > 0: the stage runs
    pt::GrainStep step{};
};
int grain_params_check(const pt_grain_params *n, GrainSetup &out);
// The threshold table of `gamma` (pt_display_capi.cpp: one per gamma, built on first use and kept).
struct DisplayTable;
std::shared_ptr<const DisplayTable> display_table(float gamma);
// The three bytes (r, g, b) of pixel (x, y) with samples from its g, the value behind matrix -> exposure -> curve -> LUT: grain, then
// per channel the dithered level of a value the table covers, and the host's own tone map and truncation of any other.
void grain_pixel_bytes(const pt::GrainStep &s, const DisplayTable &table, float gamma, uint32_t x, uint32_t y, const float *g, uint8_t *rgb);

// pt_linear_params as every entry point checks them (no device is touched) (pt_linear_capi.cpp).
struct LinearSetup {
    bool on = false;          // format != 0: the stage runs
    int format = 0;           // PT_LINEAR_PFM or PT_LINEAR_RGBE
    bool exposed = false;
};
int linear_params_check(const pt_linear_params *lin, LinearSetup &out);
// What pt_linear_encode and pt_linear_encode_device_host check, in the order pt_hip.h states: buffers and sizes, the image size, *lin
// (which must name a format), the exposure where it is used.
int linear_image_check(int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure, const pt_linear_params *lin,
                       const uint8_t *out, LinearSetup &setup);

// The image a chain has reached: planes on the device, sums still (divide) or means, and its size.
struct Image { const float *rgb; const int32_t *count; bool divide; int32_t width, height; };
// One image-space stage's launch arguments -- the only place each of these structs is filled: its checked parameters, the image it
// reads, the device scalar e where it has one, and where it writes (its view of pt_device_mem.hpp).
inline pt::OpticsArgs optics_args(const OpticsSetup &s, const Image &in, const MeanPlanes &out) {
    pt::OpticsArgs a;
    a.width = in.width; a.height = in.height; a.divide = in.divide ? 1 : 0; a.rgb = in.rgb; a.count = in.count;
    a.k1 = s.k1; a.k2 = s.k2; a.vignette = s.vignette; a.out_rgb = out.rgb; a.out_count = out.count;
    for (int k = 0; k < 3; ++k) a.mag[k] = s.mag[k];
    return a;
}
inline pt::MeterArgs meter_args(const Image &in, uint32_t *hist) {
    pt::MeterArgs a;
    a.n = in.width * in.height; a.divide = in.divide ? 1 : 0; a.rgb = in.rgb; a.count = in.count; a.hist = hist;
    return a;
}
inline pt::BloomArgs bloom_args(const BloomSetup &s, const Image &in, const float *exposure, const BloomPlanes &w) {
    pt::BloomArgs a;
    a.width = in.width; a.height = in.height; a.divide = in.divide ? 1 : 0; a.rgb = in.rgb; a.count = in.count; a.exposure = exposure;
    a.levels = s.levels; a.threshold = s.threshold; a.weight = s.weight; a.pyramid = w.pyramid; a.out_rgb = w.out_rgb;
    return a;
}
inline pt::LocalArgs local_args(const LocalSetup &s, const Image &in, const float *exposure, const LocalPlanes &w) {
    pt::LocalArgs a;
    a.width = in.width; a.height = in.height; a.divide = in.divide ? 1 : 0; a.rgb = in.rgb; a.count = in.count; a.exposure = exposure;
    a.levels = s.levels; a.strength = s.strength; a.pivot = s.pivot; a.sigma = s.sigma;
    a.base[0] = w.base[0]; a.base[1] = w.base[1]; a.out_rgb = w.out_rgb;
    return a;
}
// (out_rgb: the stage's own plane of means, or the plane `in` names, when that is one the caller may write)
inline pt::SharpenArgs sharpen_args(const SharpenSetup &s, const Image &in, const float *exposure, const SharpenPlanes &w, float *out_rgb) {
    pt::SharpenArgs a;
    a.width = in.width; a.height = in.height; a.divide = in.divide ? 1 : 0; a.rgb = in.rgb; a.count = in.count; a.exposure = exposure;
    a.strength = s.strength; a.limit = s.limit; a.luma = w.luma; a.out_rgb = out_rgb;
    return a;
}
inline pt::LinearArgs linear_args(const LinearSetup &s, const Image &in, const float *exposure, uint32_t *out) {
    pt::LinearArgs a;
    a.width = in.width; a.height = in.height; a.divide = in.divide ? 1 : 0; a.format = s.format; a.exposed = s.exposed ? 1 : 0;
    a.rgb = in.rgb; a.count = in.count; a.exposure = exposure; a.out = out;
    return a;
}

// pt_temporal_push_host in two halves, for a chain whose frame already lies on the device (pt_display_present).
// temporal_enqueue checks the parameters and enqueues features -> merge -> filter on `stream`, reading the frame's accumulators
// from `frame` in place; *out names the planes the chain writes (they belong to `t`).  The history is only read: it advances
// when the caller, once the chain has finished, calls temporal_commit -- or stays as it was if it never does.
struct TemporalPlanes {
    AccumPlanes merged;                  // sum_out, sum2_out, count_out
    const float *history_frames = nullptr;
    const float *mean = nullptr;         // with a filter (levels > 0) only
    const int32_t *mean_count = nullptr;
};
int temporal_enqueue(pt_temporal *t, const AccumPlanes &frame, const pt_temporal_params *prm, const pt_denoise_params *dn,
                     hipStream_t stream, TemporalPlanes *out);
void temporal_commit(pt_temporal *t);

// What a display needs of a frame: gathers if a band changed and waits, as pt_frame_read does; then the root device's copy of
// the scene, its full-frame planes and the root band's stream.
// Every device's copy of a frame's scene (owned by the frame), for the setters that live outside pt_frame.cpp.
const std::vector<pt_scene *> &frame_scenes(pt_frame *f);
int frame_root_planes(pt_frame *f, pt_scene **scene, AccumPlanes *planes, hipStream_t *stream, int32_t *width, int32_t *height);

// A setter on one handle or on every device's copy of a frame's scene, all or nothing: prepare() makes the host object once (and
// refuses what the handles do not allow), upload(i) puts it on copy i's device -- made current here -- into storage of its own, and
// only when every copy has it, and no launch in flight can still read the old one, does commit(i) change handle i.
template <class Prepare, class Upload, class Commit>
int set_on_copies(pt_scene *const *scenes, size_t n, Prepare &&prepare, Upload &&upload, Commit &&commit) {
    for (size_t i = 0; i < n; ++i)
        if (!scenes[i]) return fail(PT_ERR_INVALID_ARGUMENT, "null scene");
    int rc = prepare();
    if (rc != PT_OK) return rc;
    for (size_t i = 0; i < n; ++i) {
        if (scenes[i]->device < 0) continue;
        PT_HIP_TRY(hipSetDevice(scenes[i]->device));
        if ((rc = upload(i)) != PT_OK) return rc;
        PT_HIP_TRY(hipDeviceSynchronize());
    }
    for (size_t i = 0; i < n; ++i) commit(i);
    return PT_OK;
}
// A pt_frame_* entry point of those setters and of their getters: f(copies, count) on every device's copy of the frame's scene, or
// f(root) on the first.
template <class F>
int on_frame(pt_frame *frame, F &&f) {
    return guarded([&] {
        if (!frame) return fail(PT_ERR_INVALID_ARGUMENT, "null frame");
        const std::vector<pt_scene *> &sc = frame_scenes(frame);
        return f(sc.data(), sc.size());
    });
}
template <class F>
int on_frame_root(pt_frame *frame, F &&f) {
    return on_frame(frame, [&](pt_scene *const *sc, size_t) { return f(sc[0]); });
}

inline std::vector<pt::TexBary> texture_bary_records(const std::vector<pt::ExactRec> &exact) {
    std::vector<pt::TexBary> out(exact.size());
    for (size_t i = 0; i < exact.size(); ++i) out[i] = pt::tex_bary_record(exact[i].v0, exact[i].v1, exact[i].v2);
    return out;
}
// The one upload path of surface tables: every table `t` holds onto the current device, into `out`, and into `kept` those stand-ins
// that the highest of them reads and `kept` does not hold yet (no launch in flight reads a buffer this adds).  A setter gives its
// new table alone, storage of its own and the handle's `kept`; a new handle's upload gives all of its tables and its own buffers twice.
inline int upload_surface(const SurfaceTables &t, const pt::DeviceTables &tables, DeviceSurface &out, DeviceSurface &kept) {
    const int unit = t.envdirect ? pt::kEnvDirectUnit : t.direct ? pt::kDirectUnit : t.rough ? pt::kRoughUnit : t.smooth ? pt::kSmoothUnit : t.textures ? pt::kTextureUnit : pt::kNoSurfaceUnit;
    const size_t n_mat = tables.mats.size(), n_tri = tables.exact.size();
    int rc = PT_OK;
    const auto put = [&rc](ptc::DeviceBuffer &b, const auto &v, const char *what) {
        if (rc == PT_OK) rc = b.upload(v, what, 64);
    };
    if (unit >= pt::kTextureUnit && !kept.bary) put(kept.bary, texture_bary_records(tables.exact), "barycentric records");
    if (unit >= pt::kTextureUnit && !kept.no_glass) put(kept.no_glass, std::vector<pt::GlassRec>(n_mat, pt::GlassRec{}), "empty dielectric table");
    if (unit >= pt::kSmoothUnit && !kept.no_tex) put(kept.no_tex, std::vector<pt::TexRec>(n_mat, pt::TexRec{0, 0, 0, 0}), "empty texture table");
    if (unit >= pt::kRoughUnit && !kept.no_normals) put(kept.no_normals, std::vector<pt::SmoothCorner>(3 * n_tri, pt::SmoothCorner{0.0f, 0.0f, 0.0f, 0.0f}), "empty shading normals");
    if (unit >= pt::kDirectUnit && !kept.no_alpha) put(kept.no_alpha, std::vector<float>(n_mat, 0.0f), "empty roughness table");
    if (t.glass) put(out.glass, t.glass->table, "dielectric table");
    if (t.textures) {
        put(out.tex_recs, t.textures->recs, "texture table");
        put(out.tex_uv, *t.texcoords, "texture coordinates");
        put(out.tex_texels, t.textures->pool, "texels");
    }
    if (t.smooth) {
        std::vector<pt::SmoothCorner> corners(t.smooth->size() / 3);
        for (size_t i = 0; i < corners.size(); ++i) corners[i] = pt::SmoothCorner{(*t.smooth)[3 * i], (*t.smooth)[3 * i + 1], (*t.smooth)[3 * i + 2], 0.0f};
        put(out.normals, corners, "shading normals");
    }
    if (t.rough) put(out.alpha, t.rough->table, "roughness table");
    if (t.direct) put(out.lights, t.direct->lights, "light table");
    if (t.envdirect) {
        put(out.env_alias, t.envdirect->records, "environment sampling table");
        put(out.env_lights, t.envdirect->lights->lights.empty() ? std::vector<pt::LightRec>(1, pt::LightRec{}) : t.envdirect->lights->lights, "light table");
    }
    return rc;
}
// Whether material `m` is what the light table takes its lights from: the single emissive lobe.
inline bool material_is_light(const pt::MatRec &m) { return m.n_lobes == 1 && m.kind0 == 0; }
// The light table of a scene (pt_direct_capi.cpp; pt_hip.h: THE LIGHT TABLE).
std::shared_ptr<pt_light_table> light_table_of(const pt::DeviceTables &tables);
// Environment sampling's sampler and its rebuild (pt_hip.h: environment sampling), inline here: the environment's setters
// (pt_environment_capi.cpp) rebuild the table of a switched-on handle and must not need another translation unit for it.
// Phi_em of a light table (pt_hip.h: SHARE): areas as the table builder forms them, in double from the float edges.
inline double envdirect_emitted_power(const pt_light_table &t) {
    double sum = 0.0;
    for (const pt::LightRec &l : t.lights) {
        const double ax = l.e1[0], ay = l.e1[1], az = l.e1[2], bx = l.e2[0], by = l.e2[1], bz = l.e2[2];
        const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        const double area = 0.5 * std::sqrt((cx * cx + cy * cy) + cz * cz);
        sum += area * pt::envdirect_lum(l.le[0], l.le[1], l.le[2]);
    }
    return 3.14159265358979323846 * sum;
}

// The sampler of `map` for a scene with light table `lights` and the setter's `given`; refuses a black map and a share out of range.
inline int envdirect_sampler(const pt_env_map &map, std::shared_ptr<const pt_light_table> lights, const pt_env_sampling &given,
                  std::shared_ptr<const pt_env_sampler> &out) {
    auto s = std::make_shared<pt_env_sampler>();
    s->given = given;
    s->lights = std::move(lights);
    s->cells = pt::envdirect_cells(map.n);
    const bool emitters = !s->lights->lights.empty() && s->lights->area > 0.0f && std::isfinite(s->lights->area);
    const float g = given.share;
    if (emitters ? !(g == 0.0f || (g > 0.0f && g < 1.0f)) : !(g == 0.0f || g == 1.0f))
        return fail(PT_ERR_INVALID_ARGUMENT, emitters ? "environment sampling: the share must lie strictly between 0 and 1 (0 = the default): either end leaves a source unsampled"
                               : "environment sampling: a scene without emitters has share 1 (give 0 or 1)");
    if (!pt::envdirect_build(map.n, pt::env_with_apron(map.n, map.rgb.data()), s->records, s->phi_env))
        return fail(PT_ERR_INVALID_ARGUMENT, "environment sampling: the environment is black or not finite: there is nothing to sample");
    if (!emitters) {
        auto none = std::make_shared<pt_light_table>();
        s->lights = none;
        s->share = 1.0f;
    } else if (g != 0.0f) {
        s->share = g;
    } else {
        const float d = static_cast<float>(s->phi_env / (s->phi_env + envdirect_emitted_power(*s->lights)));
        s->share = d < 0.125f ? 0.125f : d > 0.875f ? 0.875f : d;
        if (!(s->share == s->share)) s->share = 0.875f;   // (an infinite Phi_em)
    }
    out = std::move(s);
    return PT_OK;
}

// Environment sampling on handles whose environment is being replaced by `map`: the new table of those copies that have the switch, built
// once and uploaded to each copy's device; envdirect_commit(i) then swaps copy i's.  Copies without the switch are left alone.  A map the
// table refuses fails here, before any handle has changed.
struct EnvSamplingRebuild {
    std::shared_ptr<const pt_env_sampler> table;
    std::vector<DeviceSurface> fresh;
};
inline int envdirect_prepare(pt_scene *const *scenes, size_t n, const pt_env_map &map, EnvSamplingRebuild &out) {
    const pt_env_sampler *old = nullptr;
    for (size_t i = 0; i < n && !old; ++i) old = scenes[i]->surface.envdirect.get();
    if (!old) return PT_OK;
    int rc = envdirect_sampler(map, old->lights, old->given, out.table);
    if (rc != PT_OK) return rc;
    SurfaceTables made;
    made.envdirect = out.table;
    out.fresh.resize(n);
    for (size_t i = 0; i < n; ++i) {
        if (!scenes[i]->surface.envdirect || scenes[i]->device < 0) continue;
        PT_HIP_TRY(hipSetDevice(scenes[i]->device));
        if ((rc = upload_surface(made, scenes[i]->shared->tables, out.fresh[i], scenes[i]->d_surface)) != PT_OK) return rc;
    }
    return PT_OK;
}
inline void envdirect_commit(pt_scene *scene, size_t i, EnvSamplingRebuild &r) {
    if (!scene->surface.envdirect || !r.table) return;
    scene->d_surface.env_alias = std::move(r.fresh[i].env_alias);
    scene->d_surface.env_lights = std::move(r.fresh[i].env_lights);
    scene->surface.envdirect = r.table;
}

}  // namespace ptc
