// Host side of the first-hit feature buffers and of the denoiser (include/pt_hip.h: pt_render_features_host, pt_denoise_host):
// argument checks, device buffers, the launches of pt_denoise.hip.
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstring>

#include "pt_denoise.hpp"

using ptc::fail;
using ptc::guarded;
using ptc::hip_fail;

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
    const int crc = ptc::scene_trace_args(scene, p->eps, a);
    if (crc != PT_OK) return crc;
    pt::FeatureCamera cam;
    std::memcpy(cam.v, &ptc::view_camera(scene), sizeof cam.v);
    // one allocation: origins | directions | position | normal | albedo (3 floats per pixel each) | hit_t | hit_index
    float *d_all = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_all), n * 17 * sizeof(float));
    if (e != hipSuccess) return hip_fail(e, "pt_render_features_host");
    float *d_o = d_all, *d_d = d_o + 3 * n, *d_p = d_d + 3 * n, *d_n = d_p + 3 * n, *d_a = d_n + 3 * n, *d_t = d_a + 3 * n;
    int32_t *d_i = reinterpret_cast<int32_t *>(d_t + n);
    const int ni = static_cast<int>(n);
    e = pt::launch_feature_rays(cam, p->width, p->height, p->row_begin, rows, d_o, d_d, nullptr);
    if (e == hipSuccess) e = pt::launch_trace_rays(a, d_o, d_d, ni, d_i, d_t, nullptr);
    if (e == hipSuccess) e = pt::launch_feature_gather(scene->d_exact, scene->d_mats, d_o, d_d, d_i, d_t, ni, d_p, d_n, d_a, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && hit_index) e = hipMemcpy(hit_index, d_i, n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && hit_t) e = hipMemcpy(hit_t, d_t, n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && position) e = hipMemcpy(position, d_p, n * 12, hipMemcpyDeviceToHost);
    if (e == hipSuccess && normal) e = hipMemcpy(normal, d_n, n * 12, hipMemcpyDeviceToHost);
    if (e == hipSuccess && albedo) e = hipMemcpy(albedo, d_a, n * 12, hipMemcpyDeviceToHost);
    (void)hipFree(d_all);
    return e == hipSuccess ? static_cast<int>(PT_OK) : hip_fail(e, "pt_render_features_host");
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
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || device < 0 || device >= n_dev)
        return fail(PT_ERR_NO_DEVICE, "no usable HIP device for the denoiser (there is no CPU fallback)");
    PT_HIP_TRY(hipSetDevice(device));
    // one allocation, every plane 256-byte aligned: sum, sum2, position, normal, albedo, mean (12 n), count, hit, count_out (4 n),
    // records A0, A1, B, C (16 n)
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b12 = up(12 * n), b4 = up(4 * n), b16 = up(16 * n);
    char *d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d), 6 * b12 + 3 * b4 + 4 * b16);
    if (e != hipSuccess) return hip_fail(e, "pt_denoise_host");
    char *at = d;
    auto take = [&](size_t b) { char *r = at; at += b; return r; };
    float *d_sum = reinterpret_cast<float *>(take(b12)), *d_sum2 = reinterpret_cast<float *>(take(b12));
    float *d_pos = reinterpret_cast<float *>(take(b12)), *d_nrm = reinterpret_cast<float *>(take(b12));
    float *d_alb = reinterpret_cast<float *>(take(b12)), *d_mean = reinterpret_cast<float *>(take(b12));
    int32_t *d_cnt = reinterpret_cast<int32_t *>(take(b4)), *d_hit = reinterpret_cast<int32_t *>(take(b4));
    int32_t *d_cnt_out = reinterpret_cast<int32_t *>(take(b4));
    a.width = width; a.height = height;
    a.sum = d_sum; a.sum2 = d_sum2; a.count = d_cnt; a.position = d_pos; a.normal = d_nrm; a.albedo = d_alb; a.hit_index = d_hit;
    a.rec_a0 = take(b16); a.rec_a1 = take(b16); a.rec_b = take(b16); a.rec_c = take(b16);
    a.mean_rgb = d_mean; a.count_out = d_cnt_out;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    e = hipMemcpy(d_sum, sum, 12 * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_sum2, sum2, 12 * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_cnt, count, 4 * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_pos, position, 12 * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_nrm, normal, 12 * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_alb, albedo, 12 * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_hit, hit_index, 4 * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreate(&ev0);
    if (e == hipSuccess) e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipEventRecord(ev0, nullptr);
    if (e == hipSuccess) e = pt::launch_denoise(a, nullptr);
    if (e == hipSuccess) e = hipEventRecord(ev1, nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(ev1);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev0, ev1);
    if (e == hipSuccess) e = hipMemcpy(mean_rgb, d_mean, 12 * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess && count_out) e = hipMemcpy(count_out, d_cnt_out, 4 * n, hipMemcpyDeviceToHost);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    (void)hipFree(d);
    if (e != hipSuccess) return hip_fail(e, "pt_denoise_host");
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
