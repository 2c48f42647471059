// Host side of the first-hit feature buffers and of the denoiser (include/pt_hip.h: pt_render_features_host, pt_denoise_host):
// argument checks, device buffers, the launches of pt_denoise.hip.
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstring>

#include "pt_denoise.hpp"

using ptc::fail;
using ptc::guarded;
using ptc::hip_fail;

int ptc::enqueue_first_hits(pt_scene *scene, const pt::RenderArgs &a, const pt_camera &camera, int32_t width, int32_t height, int32_t row_begin,
                            int32_t rows, float *origins, float *directions, int32_t *hit, float *hit_t, float *position, float *normal,
                            float *albedo, hipStream_t stream) {
    pt::FeatureCamera cam;
    std::memcpy(cam.v, &camera, sizeof cam.v);
    const int n = rows * width;
    PT_HIP_TRY(pt::launch_feature_rays(cam, width, height, row_begin, rows, origins, directions, stream));
    PT_HIP_TRY(pt::launch_trace_rays(a, origins, directions, n, hit, hit_t, stream));
    PT_HIP_TRY(pt::launch_feature_gather(scene->d_exact.get<pt::ExactRec>(), scene->d_mats.get<pt::MatRec>(), origins, directions, hit, hit_t, n, position,
                                         normal, albedo, stream));
    return PT_OK;
}

// pt_render_features_host: centre rays on the device, the unchanged closest-hit search, then the hit's features.
static int render_features_host_impl(pt_scene *scene, const pt_render_params *p, int32_t *hit_index, float *hit_t, float *position,
                                     float *normal, float *albedo) {
    if (!scene || !p) return fail(PT_ERR_INVALID_ARGUMENT, "null scene or params");
    if (p->width <= 0 || p->height <= 0) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive");
    if (p->row_begin < 0 || p->row_end > p->height || p->row_begin > p->row_end)
        return fail(PT_ERR_INVALID_ARGUMENT, "row band outside the image");
    if (p->row_stride < 0) return fail(PT_ERR_INVALID_ARGUMENT, "negative row_stride");
    if (p->row_stride > 1) return fail(PT_ERR_UNSUPPORTED, "feature buffers are rendered for contiguous rows only (row_stride 0 / 1)");
    if (static_cast<long long>(p->width) * p->height > 0x7fffffffLL) return fail(PT_ERR_INVALID_ARGUMENT, "image has more than 2^31 pixels");
    if (scene->device < 0) return fail(PT_ERR_NO_DEVICE, "scene was created without a device (device < 0)");
    const int rows = p->row_end - p->row_begin;
    const size_t n = static_cast<size_t>(rows) * p->width;
    if (n == 0) return PT_OK;
    PT_HIP_TRY(hipSetDevice(scene->device));
    std::lock_guard<std::mutex> launch_lock(scene->launch_mutex);
    pt::RenderArgs a;
    int rc = ptc::scene_trace_args(scene, p->eps, a);
    if (rc != PT_OK) return rc;
    // one allocation: origins | directions | position | normal | albedo (3 floats per pixel each) | hit_t | hit_index
    ptc::DeviceBuffer d_all;
    if ((rc = d_all.alloc(n * 17 * sizeof(float), "pt_render_features_host")) != PT_OK) return rc;
    float *d_o = d_all.get<float>(), *d_d = d_o + 3 * n, *d_p = d_d + 3 * n, *d_n = d_p + 3 * n, *d_a = d_n + 3 * n, *d_t = d_a + 3 * n;
    int32_t *d_i = reinterpret_cast<int32_t *>(d_t + n);
    rc = ptc::enqueue_first_hits(scene, a, ptc::view_camera(scene), p->width, p->height, p->row_begin, rows, d_o, d_d, d_i, d_t, d_p, d_n, d_a, nullptr);
    if (rc != PT_OK) return rc;
    PT_HIP_TRY(hipDeviceSynchronize());
    if (hit_index) PT_HIP_TRY(hipMemcpy(hit_index, d_i, n * 4, hipMemcpyDeviceToHost));
    if (hit_t) PT_HIP_TRY(hipMemcpy(hit_t, d_t, n * 4, hipMemcpyDeviceToHost));
    if (position) PT_HIP_TRY(hipMemcpy(position, d_p, n * 12, hipMemcpyDeviceToHost));
    if (normal) PT_HIP_TRY(hipMemcpy(normal, d_n, n * 12, hipMemcpyDeviceToHost));
    if (albedo) PT_HIP_TRY(hipMemcpy(albedo, d_a, n * 12, hipMemcpyDeviceToHost));
    return PT_OK;
}


static_assert(PT_DENOISE_MAX_LEVELS == pt::kDenoiseMaxLevels, "the ABI header states the denoiser's level limit");

namespace ptc {

int denoise_params_to_args(const pt_denoise_params *prm, pt::DenoiseArgs &a) {
    if (prm->levels < 0 || prm->levels > PT_DENOISE_MAX_LEVELS) return fail(PT_ERR_INVALID_ARGUMENT, "denoise: levels must lie in 0 .. 8");
    if (!std::isfinite(prm->sigma_luminance) || !std::isfinite(prm->sigma_plane) || prm->sigma_luminance < 0.0f || prm->sigma_plane < 0.0f)
        return fail(PT_ERR_INVALID_ARGUMENT, "denoise: sigmas must be finite and not negative (0 = the default)");
    if (prm->normal_power_log2 < 0 || prm->normal_power_log2 > pt::kDenoiseMaxNormalPowerLog2)
        return fail(PT_ERR_INVALID_ARGUMENT, "denoise: normal_power_log2 must lie in 0 .. 16 (0 = the default)");
    a.levels = prm->levels;
    a.sigma_luminance = prm->sigma_luminance > 0.0f ? prm->sigma_luminance : pt::kDenoiseSigmaLuminance;
    a.sigma_plane = prm->sigma_plane > 0.0f ? prm->sigma_plane : pt::kDenoiseSigmaPlane;
    a.normal_power_log2 = prm->normal_power_log2 > 0 ? prm->normal_power_log2 : pt::kDenoiseNormalPowerLog2;
    a.demodulate = prm->demodulate_albedo >= 0 ? 1 : 0;
    return PT_OK;
}

void unfiltered_mean(size_t n, const float *sum, const int32_t *count, float *mean_rgb, int32_t *count_out) {
    for (size_t p = 0; p < n; ++p) {
        const float cn = static_cast<float>(count[p]);
        for (int k = 0; k < 3; ++k) mean_rgb[3 * p + k] = count[p] ? sum[3 * p + k] / cn : sum[3 * p + k];
        if (count_out) count_out[p] = count[p];
    }
}

}  // namespace ptc

static int denoise_host_impl(int device, int32_t width, int32_t height, const float *sum, const float *sum2, const int32_t *count,
                             const float *position, const float *normal, const float *albedo, const int32_t *hit_index,
                             const pt_denoise_params *prm, float *mean_rgb, int32_t *count_out, float *kernel_ms) {
    if (width <= 0 || height <= 0 || !sum || !sum2 || !count || !prm || !mean_rgb) return fail(PT_ERR_INVALID_ARGUMENT, "null buffer or empty image");
    if (static_cast<long long>(width) * height > 0x7fffffffLL / 4) return fail(PT_ERR_INVALID_ARGUMENT, "image too large");
    pt::DenoiseArgs a;
    const int prc = ptc::denoise_params_to_args(prm, a);
    if (prc != PT_OK) return prc;
    const size_t n = static_cast<size_t>(width) * height;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (prm->levels == 0) {   // the unfiltered mean, on the host
        ptc::unfiltered_mean(n, sum, count, mean_rgb, count_out);
        return PT_OK;
    }
    if (!position || !normal || !albedo || !hit_index) return fail(PT_ERR_INVALID_ARGUMENT, "denoise: null feature buffer");
    int rc = ptc::use_device(device, "denoiser");
    if (rc != PT_OK) return rc;
    // one allocation, every plane 256-byte aligned: sum, sum2, position, normal, albedo, mean (12 n), count, hit, count_out (4 n),
    // records A0, A1, B, C (16 n)
    ptc::PlaneLayout l;
    const size_t o_sum = l.add(12 * n), o_sum2 = l.add(12 * n), o_pos = l.add(12 * n), o_nrm = l.add(12 * n), o_alb = l.add(12 * n), o_mean = l.add(12 * n);
    const size_t o_cnt = l.add(4 * n), o_hit = l.add(4 * n), o_cnt_out = l.add(4 * n);
    const size_t o_a0 = l.add(16 * n), o_a1 = l.add(16 * n), o_b = l.add(16 * n), o_c = l.add(16 * n);
    ptc::DeviceBuffer d;
    if ((rc = d.alloc(l, "pt_denoise_host")) != PT_OK) return rc;
    const ptc::AccumPlanes acc = {d.at<float>(o_sum), d.at<float>(o_sum2), d.at<int32_t>(o_cnt), n};
    a.width = width; a.height = height;
    a.sum = acc.sum; a.sum2 = acc.sum2; a.count = acc.count;
    a.position = d.at<float>(o_pos); a.normal = d.at<float>(o_nrm); a.albedo = d.at<float>(o_alb); a.hit_index = d.at<int32_t>(o_hit);
    a.rec_a0 = d.at<void>(o_a0); a.rec_a1 = d.at<void>(o_a1); a.rec_b = d.at<void>(o_b); a.rec_c = d.at<void>(o_c);
    a.mean_rgb = d.at<float>(o_mean); a.count_out = d.at<int32_t>(o_cnt_out);
    if ((rc = acc.upload(sum, sum2, count)) != PT_OK) return rc;
    PT_HIP_TRY(hipMemcpy(d.at<void>(o_pos), position, 12 * n, hipMemcpyHostToDevice));
    PT_HIP_TRY(hipMemcpy(d.at<void>(o_nrm), normal, 12 * n, hipMemcpyHostToDevice));
    PT_HIP_TRY(hipMemcpy(d.at<void>(o_alb), albedo, 12 * n, hipMemcpyHostToDevice));
    PT_HIP_TRY(hipMemcpy(d.at<void>(o_hit), hit_index, 4 * n, hipMemcpyHostToDevice));
    ptc::DeviceEvent ev0, ev1;
    if ((rc = ev0.create("pt_denoise_host")) != PT_OK || (rc = ev1.create("pt_denoise_host")) != PT_OK) return rc;
    PT_HIP_TRY(hipEventRecord(ev0.get(), nullptr));
    PT_HIP_TRY(pt::launch_denoise(a, nullptr));
    PT_HIP_TRY(hipEventRecord(ev1.get(), nullptr));
    PT_HIP_TRY(hipEventSynchronize(ev1.get()));
    float ms = 0.0f;
    PT_HIP_TRY(hipEventElapsedTime(&ms, ev0.get(), ev1.get()));
    PT_HIP_TRY(hipMemcpy(mean_rgb, a.mean_rgb, 12 * n, hipMemcpyDeviceToHost));
    if (count_out) PT_HIP_TRY(hipMemcpy(count_out, a.count_out, 4 * n, hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = ms;
    return PT_OK;
}


extern "C" {

int pt_render_features_host(pt_scene *scene, const pt_render_params *params, int32_t *hit_index, float *hit_t, float *position,
                            float *normal, float *albedo) {
    return guarded([&] { return render_features_host_impl(scene, params, hit_index, hit_t, position, normal, albedo); });
}

int pt_denoise_host(int device, int32_t width, int32_t height, const float *sum, const float *sum2, const int32_t *count,
                    const float *position, const float *normal, const float *albedo, const int32_t *hit_index,
                    const pt_denoise_params *params, float *mean_rgb, int32_t *count_out, float *kernel_ms) {
    return guarded([&] {
        return denoise_host_impl(device, width, height, sum, sum2, count, position, normal, albedo, hit_index, params, mean_rgb, count_out, kernel_ms);
    });
}

}  // extern "C"
