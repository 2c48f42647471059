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
    ptc::DeviceBuffer d_all;      // everything below but the denoiser's planes
    ptc::AccumPlanes in, out;     // the frame pushed, the merged accumulators
    ptc::FeaturePlanes features;  // the first hits of the view the frame was rendered from
    float *d_frames = nullptr;
    pt::TemporalRecords rec[2];   // ping-pong; rec[cur] holds the history
    int cur = 0;
    bool has_history = false;
    pt_camera camera{};           // of the history
    pt_camera pending_camera{};   // of the chain enqueued last: the history's once that chain is committed
    float inverse[9] = {};        // rows of the inverse of [right up forward] of that camera
    ptc::DeviceBuffer d_denoise;  // allocated by the first push that filters
    ptc::DenoisePlanes denoise;
    ptc::DeviceTimer timer;
    ~pt_temporal() { (void)hipSetDevice(scene->device); }   // (a handle exists only over a scene with a device)
};

namespace {

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

int temporal_create_impl(pt_scene *scene, int32_t width, int32_t height, float eps, pt_temporal **out) {
    if (!scene || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null scene or output pointer");
    *out = nullptr;
    if (width <= 0 || height <= 0) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive");
    int rc = ptc::check_image_size(width, height);
    if (rc != PT_OK) return rc;
    if (std::isnan(eps)) return fail(PT_ERR_INVALID_ARGUMENT, "eps is not a number");
    if ((rc = ptc::check_has_device(scene, "; there is no CPU fallback")) != PT_OK) return rc;
    PT_HIP_TRY(hipSetDevice(scene->device));
    std::unique_ptr<pt_temporal> t(new pt_temporal);
    t->scene = scene; t->width = width; t->height = height; t->eps = eps;
    const size_t n = t->n = static_cast<size_t>(width) * height;
    // one allocation: the two accumulator triples, the features, the frame counts, the two sets of four records of 16 n
    ptc::PlaneLayout l;
    t->in = ptc::AccumPlanes::in(l, n);
    t->out = ptc::AccumPlanes::in(l, n);
    t->features = ptc::FeaturePlanes::in(l, n);
    const size_t o_frames = l.add(4 * n);
    size_t o_rec[8];
    for (size_t &o : o_rec) o = l.add(16 * n);
    if ((rc = t->d_all.alloc(l, "pt_temporal_create")) != PT_OK || (rc = t->timer.create("pt_temporal_create")) != PT_OK) return rc;
    const ptc::DeviceBuffer &d = t->d_all;
    t->in.bind(d); t->out.bind(d); t->features.bind(d);
    t->d_frames = d.at<float>(o_frames);
    for (int k = 0; k < 2; ++k)
        t->rec[k] = {d.at<void>(o_rec[4 * k]), d.at<void>(o_rec[4 * k + 1]), d.at<void>(o_rec[4 * k + 2]), d.at<void>(o_rec[4 * k + 3])};
    *out = t.release();
    return PT_OK;
}

int check_temporal_params(const pt_temporal_params *prm) {
    if (std::isnan(prm->max_frames) || prm->max_frames < 0.0f) return fail(PT_ERR_INVALID_ARGUMENT, "temporal: max_frames must not be negative (0 = the default)");
    if (!std::isfinite(prm->sigma_plane) || prm->sigma_plane < 0.0f)
        return fail(PT_ERR_INVALID_ARGUMENT, "temporal: sigma_plane must be finite and not negative (0 = the default)");
    if (!std::isfinite(prm->min_normal_dot) || prm->min_normal_dot < 0.0f || prm->min_normal_dot > 1.0f)
        return fail(PT_ERR_INVALID_ARGUMENT, "temporal: min_normal_dot must lie in 0 .. 1 (0 = the default)");
    return PT_OK;
}

// The chain of a push on `stream`, from accumulators that lie on the device (`frame`: the handle's own upload planes, or a
// session's): the view's first hits, the merge, the filter -- no host synchronisation in between.  The caller holds t->mutex and
// has made the scene's device current.  `timer` (NULL: none) times the kernels.  The history is only read.
int enqueue_chain(pt_temporal *t, const ptc::AccumPlanes &frame, const pt_temporal_params *prm, const pt_denoise_params *dn,
                  hipStream_t stream, const ptc::DeviceTimer *timer, int *levels) {
    int rc = check_temporal_params(prm);
    if (rc != PT_OK) return rc;
    // (the reprojection inverts a pinhole: pt_hip.h, pt_projection)
    if (t->scene->has_projection) return fail(PT_ERR_UNSUPPORTED, "temporal: the scene handle has a non-perspective projection, which the reprojection does not invert");
    pt::DenoiseArgs da;
    da.levels = 0;
    if (dn && (rc = ptc::denoise_params_to_args(dn, da)) != PT_OK) return rc;
    *levels = da.levels;
    pt_scene *scene = t->scene;
    if (da.levels > 0 && !t->d_denoise) {
        ptc::PlaneLayout l;
        t->denoise = ptc::DenoisePlanes::in(l, t->n);
        if ((rc = t->d_denoise.alloc(l, "pt_temporal_push_host")) != PT_OK) return rc;
        t->denoise.bind(t->d_denoise);
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
    a.prev = t->rec[t->cur]; a.next = t->rec[t->cur ^ 1];
    a.sum = frame.sum; a.sum2 = frame.sum2; a.count = frame.count;
    a.position = t->features.position; a.normal = t->features.normal; a.hit_index = t->features.hit;
    a.sum_out = t->out.sum; a.sum2_out = t->out.sum2; a.count_out = t->out.count; a.history_frames = t->d_frames;
    da.width = t->width; da.height = t->height;
    ptc::bind_planes(da, t->out, t->features, t->denoise);

    std::lock_guard<std::mutex> launch_lock(scene->launch_mutex);
    pt::RenderArgs ra;
    if ((rc = ptc::scene_trace_args(scene, t->eps, ra)) != PT_OK) return rc;
    if (timer) PT_HIP_TRY(timer->begin(stream));
    if ((rc = ptc::enqueue_first_hits(scene, ra, cam, t->width, t->height, 0, t->height, t->features, stream)) != PT_OK) return rc;
    PT_HIP_TRY(pt::launch_temporal_merge(a, stream));
    if (da.levels > 0) PT_HIP_TRY(pt::launch_denoise(da, stream));
    if (timer) PT_HIP_TRY(timer->end(stream));
    t->pending_camera = cam;
    return PT_OK;
}

// The chain has finished: the records it wrote are the history now.
void commit_chain(pt_temporal *t) {
    t->cur ^= 1;
    t->has_history = true;
    t->camera = t->pending_camera;
    camera_inverse(t->camera, t->inverse);
}

int temporal_push_impl(pt_temporal *t, const float *sum, const float *sum2, const int32_t *count, const pt_temporal_params *prm,
                       const pt_denoise_params *dn, float *sum_out, float *sum2_out, int32_t *count_out, float *history_frames,
                       float *mean_rgb, int32_t *mean_count, float *kernel_ms) {
    if (!t || !sum || !sum2 || !count || !prm) return fail(PT_ERR_INVALID_ARGUMENT, "null handle, accumulator buffer or params");
    int rc = check_temporal_params(prm);
    if (rc != PT_OK) return rc;
    pt::DenoiseArgs checked;
    if (dn && (rc = ptc::denoise_params_to_args(dn, checked)) != PT_OK) return rc;
    const size_t n = t->n;
    if (kernel_ms) *kernel_ms = 0.0f;
    PT_HIP_TRY(hipSetDevice(t->scene->device));
    std::lock_guard<std::mutex> push_lock(t->mutex);
    if ((rc = t->in.upload(sum, sum2, count)) != PT_OK) return rc;
    int levels = 0;
    if ((rc = enqueue_chain(t, t->in, prm, dn, nullptr, &t->timer, &levels)) != PT_OK) return rc;
    // (an error return from here on leaves the history the previous one: rec[cur] was only read)
    float ms = 0.0f;
    PT_HIP_TRY(t->timer.wait_ms(&ms));
    if ((rc = t->out.download(sum_out, sum2_out, count_out)) != PT_OK) return rc;
    if (history_frames) PT_HIP_TRY(hipMemcpy(history_frames, t->d_frames, 4 * n, hipMemcpyDeviceToHost));
    if (dn && levels > 0) {
        if ((rc = t->denoise.out.download(mean_rgb, mean_count)) != PT_OK) return rc;
    } else if (dn && mean_rgb) {   // levels = 0: the unfiltered mean of the merged accumulators, on the host
        std::vector<float> s(3 * n);
        std::vector<int32_t> c(n);
        if ((rc = t->out.download(s.data(), nullptr, c.data())) != PT_OK) return rc;
        ptc::unfiltered_mean(n, s.data(), c.data(), mean_rgb, mean_count);
    }
    commit_chain(t);
    if (kernel_ms) *kernel_ms = ms;
    return PT_OK;
}

}  // namespace

int ptc::temporal_enqueue(pt_temporal *t, const AccumPlanes &frame, const pt_temporal_params *prm, const pt_denoise_params *dn,
                          hipStream_t stream, TemporalPlanes *out) {
    if (!t || !prm || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null handle, params or output");
    if (frame.n != t->n) return fail(PT_ERR_INVALID_ARGUMENT, "temporal: the frame's planes do not hold width x height pixels");
    PT_HIP_TRY(hipSetDevice(t->scene->device));
    std::lock_guard<std::mutex> push_lock(t->mutex);
    int levels = 0;
    const int rc = enqueue_chain(t, frame, prm, dn, stream, nullptr, &levels);
    if (rc != PT_OK) return rc;
    out->merged = t->out;
    out->history_frames = t->d_frames;
    out->mean = levels > 0 ? t->denoise.out.rgb : nullptr;
    out->mean_count = levels > 0 ? t->denoise.out.count : nullptr;
    return PT_OK;
}

void ptc::temporal_commit(pt_temporal *t) {
    std::lock_guard<std::mutex> push_lock(t->mutex);
    commit_chain(t);
}

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
    delete t;   // (~pt_temporal makes the scene's device current for its owners)
}

}  // extern "C"
