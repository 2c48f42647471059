// Host side of the temporal accumulation stage (include/pt_hip.h: pt_temporal_*): argument checks, the device-resident history,
// the chain features -> merge -> a-trous on one stream.
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstring>

#include "pt_temporal.hpp"

using ptc::fail;
using ptc::guarded;
using ptc::hip_fail;

struct pt_temporal {
    pt_scene *scene = nullptr;
    int32_t width = 0, height = 0;
    float eps = 0;
    size_t n = 0;
    std::mutex mutex;             // one push / reset at a time
    char *d_all = nullptr;        // everything below but the denoiser's planes
    float *d_sum = nullptr, *d_sum2 = nullptr, *d_origins = nullptr, *d_directions = nullptr, *d_position = nullptr, *d_normal = nullptr,
          *d_albedo = nullptr, *d_hit_t = nullptr, *d_sum_out = nullptr, *d_sum2_out = nullptr, *d_frames = nullptr;
    int32_t *d_count = nullptr, *d_hit = nullptr, *d_count_out = nullptr;
    pt::TemporalRecords rec[2];   // ping-pong; rec[cur] holds the history
    int cur = 0;
    bool has_history = false;
    pt_camera camera{};           // of the history
    float inverse[9] = {};        // rows of the inverse of [right up forward] of that camera
    char *d_denoise = nullptr;    // allocated by the first push that filters: records A0, A1, B, C, mean, count
    void *dn_a0 = nullptr, *dn_a1 = nullptr, *dn_b = nullptr, *dn_c = nullptr;
    float *d_mean = nullptr;
    int32_t *d_mean_count = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

namespace {

size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// Rows of the inverse of the matrix whose columns are right, up, forward: cross products over the determinant, in double,
// rounded to float once (pt_hip.h states the order).
void camera_inverse(const pt_camera &c, float out[9]) {
    const double r[3] = {c.right[0], c.right[1], c.right[2]}, u[3] = {c.up[0], c.up[1], c.up[2]}, f[3] = {c.forward[0], c.forward[1], c.forward[2]};
    auto cross = [](const double *a, const double *b, double *o) {
        o[0] = a[1] * b[2] - a[2] * b[1];
        o[1] = a[2] * b[0] - a[0] * b[2];
        o[2] = a[0] * b[1] - a[1] * b[0];
    };
    double uf[3], fr[3], ru[3];
    cross(u, f, uf);
    cross(f, r, fr);
    cross(r, u, ru);
    const double det = (r[0] * uf[0] + r[1] * uf[1]) + r[2] * uf[2];
    for (int k = 0; k < 3; ++k) {
        out[k] = static_cast<float>(uf[k] / det);
        out[3 + k] = static_cast<float>(fr[k] / det);
        out[6 + k] = static_cast<float>(ru[k] / det);
    }
}

void temporal_free(pt_temporal *t) {
    if (t->scene && t->scene->device >= 0) (void)hipSetDevice(t->scene->device);
    if (t->ev0) (void)hipEventDestroy(t->ev0);
    if (t->ev1) (void)hipEventDestroy(t->ev1);
    if (t->d_denoise) (void)hipFree(t->d_denoise);
    if (t->d_all) (void)hipFree(t->d_all);
    delete t;
}

int temporal_create_impl(pt_scene *scene, int32_t width, int32_t height, float eps, pt_temporal **out) {
    if (!scene || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null scene or output pointer");
    *out = nullptr;
    if (width <= 0 || height <= 0) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive");
    if (static_cast<long long>(width) * height > 0x7fffffffLL / 4) return fail(PT_ERR_INVALID_ARGUMENT, "image too large");
    if (std::isnan(eps)) return fail(PT_ERR_INVALID_ARGUMENT, "eps is not a number");
    if (scene->device < 0) return fail(PT_ERR_NO_DEVICE, "scene was created without a device (device < 0); there is no CPU fallback");
    PT_HIP_TRY(hipSetDevice(scene->device));
    pt_temporal *t = new pt_temporal;
    t->scene = scene; t->width = width; t->height = height; t->eps = eps;
    const size_t n = t->n = static_cast<size_t>(width) * height;
    const size_t b12 = up256(12 * n), b4 = up256(4 * n), b16 = up256(16 * n);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&t->d_all), 9 * b12 + 5 * b4 + 8 * b16);
    if (e == hipSuccess) e = hipEventCreate(&t->ev0);
    if (e == hipSuccess) e = hipEventCreate(&t->ev1);
    if (e != hipSuccess) {
        temporal_free(t);
        return hip_fail(e, "pt_temporal_create");
    }
    char *at = t->d_all;
    auto take = [&](size_t b) { char *r = at; at += b; return r; };
    auto f = [&](size_t b) { return reinterpret_cast<float *>(take(b)); };
    auto i = [&](size_t b) { return reinterpret_cast<int32_t *>(take(b)); };
    t->d_sum = f(b12); t->d_sum2 = f(b12); t->d_origins = f(b12); t->d_directions = f(b12); t->d_position = f(b12);
    t->d_normal = f(b12); t->d_albedo = f(b12); t->d_sum_out = f(b12); t->d_sum2_out = f(b12);
    t->d_count = i(b4); t->d_hit = i(b4); t->d_count_out = i(b4); t->d_hit_t = f(b4); t->d_frames = f(b4);
    for (auto &r : t->rec) { r.sum_n = take(b16); r.sum2_age = take(b16); r.normal = take(b16); r.position = take(b16); }
    *out = t;
    return PT_OK;
}

int temporal_push_impl(pt_temporal *t, const float *sum, const float *sum2, const int32_t *count, const pt_temporal_params *prm,
                       const pt_denoise_params *dn, float *sum_out, float *sum2_out, int32_t *count_out, float *history_frames,
                       float *mean_rgb, int32_t *mean_count, float *kernel_ms) {
    if (!t || !sum || !sum2 || !count || !prm) return fail(PT_ERR_INVALID_ARGUMENT, "null handle, accumulator buffer or params");
    if (std::isnan(prm->max_frames) || prm->max_frames < 0.0f) return fail(PT_ERR_INVALID_ARGUMENT, "temporal: max_frames must not be negative (0 = the default)");
    if (!std::isfinite(prm->sigma_plane) || prm->sigma_plane < 0.0f)
        return fail(PT_ERR_INVALID_ARGUMENT, "temporal: sigma_plane must be finite and not negative (0 = the default)");
    if (!std::isfinite(prm->min_normal_dot) || prm->min_normal_dot < 0.0f || prm->min_normal_dot > 1.0f)
        return fail(PT_ERR_INVALID_ARGUMENT, "temporal: min_normal_dot must lie in 0 .. 1 (0 = the default)");
    pt::DenoiseArgs da;
    da.levels = 0;
    if (dn) {
        const int rc = ptc::denoise_params_to_args(dn, da);
        if (rc != PT_OK) return rc;
    }
    pt_scene *scene = t->scene;
    const size_t n = t->n;
    if (kernel_ms) *kernel_ms = 0.0f;
    PT_HIP_TRY(hipSetDevice(scene->device));
    std::lock_guard<std::mutex> push_lock(t->mutex);
    if (da.levels > 0 && !t->d_denoise) {
        const size_t b12 = up256(12 * n), b4 = up256(4 * n), b16 = up256(16 * n);
        PT_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&t->d_denoise), 4 * b16 + b12 + b4));
        char *at = t->d_denoise;
        t->dn_a0 = at; t->dn_a1 = at + b16; t->dn_b = at + 2 * b16; t->dn_c = at + 3 * b16;
        t->d_mean = reinterpret_cast<float *>(at + 4 * b16);
        t->d_mean_count = reinterpret_cast<int32_t *>(at + 4 * b16 + b12);
    }
    const pt_camera cam = ptc::view_camera(scene);
    pt::TemporalArgs a;
    a.width = t->width; a.height = t->height;
    a.mode = !t->has_history ? pt::kTemporalFirstFrame
             : std::memcmp(&cam, &t->camera, sizeof cam) == 0 ? pt::kTemporalStatic : pt::kTemporalReproject;
    a.max_frames = prm->max_frames > 0.0f ? prm->max_frames : pt::kTemporalMaxFrames;
    a.sigma_plane = prm->sigma_plane > 0.0f ? prm->sigma_plane : pt::kTemporalSigmaPlane;
    a.min_normal_dot = prm->min_normal_dot > 0.0f ? prm->min_normal_dot : pt::kTemporalMinNormalDot;
    std::memcpy(a.cam, &cam, sizeof a.cam);
    std::memcpy(a.prev_origin, t->camera.origin, sizeof a.prev_origin);
    std::memcpy(a.prev_inverse, t->inverse, sizeof a.prev_inverse);
    a.sum = t->d_sum; a.sum2 = t->d_sum2; a.count = t->d_count;
    a.position = t->d_position; a.normal = t->d_normal; a.hit_index = t->d_hit;
    a.prev = t->rec[t->cur]; a.next = t->rec[t->cur ^ 1];
    a.sum_out = t->d_sum_out; a.sum2_out = t->d_sum2_out; a.count_out = t->d_count_out; a.history_frames = t->d_frames;
    da.width = t->width; da.height = t->height;
    da.sum = t->d_sum_out; da.sum2 = t->d_sum2_out; da.count = t->d_count_out;
    da.position = t->d_position; da.normal = t->d_normal; da.albedo = t->d_albedo; da.hit_index = t->d_hit;
    da.rec_a0 = t->dn_a0; da.rec_a1 = t->dn_a1; da.rec_b = t->dn_b; da.rec_c = t->dn_c;
    da.mean_rgb = t->d_mean; da.count_out = t->d_mean_count;

    hipError_t e = hipMemcpy(t->d_sum, sum, 12 * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t->d_sum2, sum2, 12 * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t->d_count, count, 4 * n, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "pt_temporal_push_host");
    {   // the chain: the view's first hits, the merge, the filter -- one stream, no host synchronisation in between
        std::lock_guard<std::mutex> launch_lock(scene->launch_mutex);
        pt::RenderArgs ra;
        const int crc = ptc::scene_trace_args(scene, t->eps, ra);
        if (crc != PT_OK) return crc;
        pt::FeatureCamera fc;
        std::memcpy(fc.v, &cam, sizeof fc.v);
        const int ni = static_cast<int>(n);
        e = hipEventRecord(t->ev0, nullptr);
        if (e == hipSuccess) e = pt::launch_feature_rays(fc, t->width, t->height, 0, t->height, t->d_origins, t->d_directions, nullptr);
        if (e == hipSuccess) e = pt::launch_trace_rays(ra, t->d_origins, t->d_directions, ni, t->d_hit, t->d_hit_t, nullptr);
        if (e == hipSuccess)
            e = pt::launch_feature_gather(scene->d_exact, scene->d_mats, t->d_origins, t->d_directions, t->d_hit, t->d_hit_t, ni, t->d_position,
                                          t->d_normal, t->d_albedo, nullptr);
        if (e == hipSuccess) e = pt::launch_temporal_merge(a, nullptr);
        if (e == hipSuccess && da.levels > 0) e = pt::launch_denoise(da, nullptr);
        if (e == hipSuccess) e = hipEventRecord(t->ev1, nullptr);
    }
    if (e == hipSuccess) e = hipEventSynchronize(t->ev1);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, t->ev0, t->ev1);
    if (e == hipSuccess && sum_out) e = hipMemcpy(sum_out, t->d_sum_out, 12 * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess && sum2_out) e = hipMemcpy(sum2_out, t->d_sum2_out, 12 * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess && count_out) e = hipMemcpy(count_out, t->d_count_out, 4 * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess && history_frames) e = hipMemcpy(history_frames, t->d_frames, 4 * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess && dn && da.levels > 0) {
        if (mean_rgb) e = hipMemcpy(mean_rgb, t->d_mean, 12 * n, hipMemcpyDeviceToHost);
        if (e == hipSuccess && mean_count) e = hipMemcpy(mean_count, t->d_mean_count, 4 * n, hipMemcpyDeviceToHost);
    } else if (e == hipSuccess && dn && mean_rgb) {   // levels = 0: the unfiltered mean of the merged accumulators, on the host
        std::vector<float> s(3 * n);
        std::vector<int32_t> c(n);
        e = hipMemcpy(s.data(), t->d_sum_out, 12 * n, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(c.data(), t->d_count_out, 4 * n, hipMemcpyDeviceToHost);
        if (e == hipSuccess) ptc::unfiltered_mean(n, s.data(), c.data(), mean_rgb, mean_count);
    }
    if (e != hipSuccess) return hip_fail(e, "pt_temporal_push_host");   // the history is still the previous one: rec[cur] was only read
    t->cur ^= 1;
    t->has_history = true;
    t->camera = cam;
    camera_inverse(cam, t->inverse);
    if (kernel_ms) *kernel_ms = ms;
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_temporal_create(pt_scene *scene, int32_t width, int32_t height, float eps, pt_temporal **out) {
    return guarded([&] { return temporal_create_impl(scene, width, height, eps, out); });
}

int pt_temporal_push_host(pt_temporal *t, const float *sum, const float *sum2, const int32_t *count, const pt_temporal_params *params,
                          const pt_denoise_params *denoise, float *sum_out, float *sum2_out, int32_t *count_out, float *history_frames,
                          float *mean_rgb, int32_t *mean_count, float *kernel_ms) {
    return guarded([&] {
        return temporal_push_impl(t, sum, sum2, count, params, denoise, sum_out, sum2_out, count_out, history_frames, mean_rgb, mean_count,
                                  kernel_ms);
    });
}

int pt_temporal_reset(pt_temporal *t) {
    return guarded([&] {
        if (!t) return fail(PT_ERR_INVALID_ARGUMENT, "null handle");
        std::lock_guard<std::mutex> lock(t->mutex);
        t->has_history = false;
        return static_cast<int>(PT_OK);
    });
}

void pt_temporal_destroy(pt_temporal *t) {
    if (t) temporal_free(t);
}

}  // extern "C"
