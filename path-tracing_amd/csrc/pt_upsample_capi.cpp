// Host side of the feature-guided upsampler (include/pt_hip.h: pt_upsample_host): argument checks -- all of them before the device
// is looked at --, device buffers, the launches of pt_upsample.hip.
#include "pt_capi_internal.hpp"

#include <cmath>

#include "pt_upsample.hpp"

using ptc::fail;
using ptc::guarded;
using ptc::hip_fail;

static_assert(PT_UPSAMPLE_MAX_SCALE == pt::kUpsampleMaxScale, "the ABI header states the upsampler's largest scale");

int ptc::upsample_params_to_args(const pt_upsample_params *prm, int32_t width, int32_t height, pt::UpsampleArgs &a) {
    if (!prm) return fail(PT_ERR_INVALID_ARGUMENT, "upsample: null params");
    if (width <= 0 || height <= 0) return fail(PT_ERR_INVALID_ARGUMENT, "upsample: empty image");
    if (prm->scale < pt::kUpsampleMinScale || prm->scale > pt::kUpsampleMaxScale) return fail(PT_ERR_INVALID_ARGUMENT, "upsample: scale must be 2, 3 or 4");
    if (width % prm->scale || height % prm->scale) return fail(PT_ERR_INVALID_ARGUMENT, "upsample: width and height must be multiples of scale");
    if (static_cast<long long>(width) * height > 0x7fffffffLL / 4) return fail(PT_ERR_INVALID_ARGUMENT, "upsample: image too large");
    if (!std::isfinite(prm->sigma_plane) || prm->sigma_plane < 0.0f)
        return fail(PT_ERR_INVALID_ARGUMENT, "upsample: sigma_plane must be finite and not negative (0 = the default)");
    if (prm->normal_power_log2 < 0 || prm->normal_power_log2 > pt::kDenoiseMaxNormalPowerLog2)
        return fail(PT_ERR_INVALID_ARGUMENT, "upsample: normal_power_log2 must lie in 0 .. 16 (0 = the default)");
    a.width = width; a.height = height; a.scale = prm->scale;
    a.sigma_plane = prm->sigma_plane > 0.0f ? prm->sigma_plane : pt::kDenoiseSigmaPlane;
    a.normal_power_log2 = prm->normal_power_log2 > 0 ? prm->normal_power_log2 : pt::kDenoiseNormalPowerLog2;
    a.demodulate = prm->demodulate_albedo >= 0 ? 1 : 0;
    return PT_OK;
}

static int upsample_host_impl(int device, int32_t width, int32_t height, const float *mean_lo, const int32_t *count_lo, const float *position,
                              const float *normal, const float *albedo, const int32_t *hit_index, const pt_upsample_params *prm,
                              float *mean_rgb, int32_t *count_out, float *kernel_ms) {
    if (!mean_lo || !count_lo || !position || !normal || !albedo || !hit_index || !prm || !mean_rgb)
        return fail(PT_ERR_INVALID_ARGUMENT, "upsample: null buffer");
    pt::UpsampleArgs a;
    int rc = ptc::upsample_params_to_args(prm, width, height, a);
    if (rc != PT_OK) return rc;
    if (kernel_ms) *kernel_ms = 0.0f;
    if ((rc = ptc::use_device(device, "upsampler")) != PT_OK) return rc;
    const size_t n = static_cast<size_t>(width) * height, n_lo = n / (static_cast<size_t>(a.scale) * a.scale);
    // one allocation, every plane 256-byte aligned: the low mean and count, the output image's features, mean and count, the
    // three records per low pixel
    ptc::PlaneLayout l;
    const size_t o_mlo = l.add(12 * n_lo), o_clo = l.add(4 * n_lo);
    const size_t o_pos = l.add(12 * n), o_nrm = l.add(12 * n), o_alb = l.add(12 * n), o_hit = l.add(4 * n), o_mean = l.add(12 * n), o_cnt = l.add(4 * n);
    const size_t o_a = l.add(16 * n_lo), o_b = l.add(16 * n_lo), o_c = l.add(16 * n_lo);
    ptc::DeviceBuffer d;
    if ((rc = d.alloc(l, "pt_upsample_host")) != PT_OK) return rc;
    a.mean_lo = d.at<float>(o_mlo); a.count_lo = d.at<int32_t>(o_clo);
    a.position = d.at<float>(o_pos); a.normal = d.at<float>(o_nrm); a.albedo = d.at<float>(o_alb); a.hit_index = d.at<int32_t>(o_hit);
    a.rec_a = d.at<void>(o_a); a.rec_b = d.at<void>(o_b); a.rec_c = d.at<void>(o_c);
    a.mean_rgb = d.at<float>(o_mean); a.count_out = d.at<int32_t>(o_cnt);
    PT_HIP_TRY(hipMemcpy(d.at<void>(o_mlo), mean_lo, 12 * n_lo, hipMemcpyHostToDevice));
    PT_HIP_TRY(hipMemcpy(d.at<void>(o_clo), count_lo, 4 * n_lo, hipMemcpyHostToDevice));
    PT_HIP_TRY(hipMemcpy(d.at<void>(o_pos), position, 12 * n, hipMemcpyHostToDevice));
    PT_HIP_TRY(hipMemcpy(d.at<void>(o_nrm), normal, 12 * n, hipMemcpyHostToDevice));
    PT_HIP_TRY(hipMemcpy(d.at<void>(o_alb), albedo, 12 * n, hipMemcpyHostToDevice));
    PT_HIP_TRY(hipMemcpy(d.at<void>(o_hit), hit_index, 4 * n, hipMemcpyHostToDevice));
    ptc::DeviceEvent ev0, ev1;
    if ((rc = ev0.create("pt_upsample_host")) != PT_OK || (rc = ev1.create("pt_upsample_host")) != PT_OK) return rc;
    PT_HIP_TRY(hipEventRecord(ev0.get(), nullptr));
    PT_HIP_TRY(pt::launch_upsample(a, nullptr));
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

int pt_upsample_host(int device, int32_t width, int32_t height, const float *mean_lo, const int32_t *count_lo, const float *position,
                     const float *normal, const float *albedo, const int32_t *hit_index, const pt_upsample_params *params,
                     float *mean_rgb, int32_t *count_out, float *kernel_ms) {
    return guarded([&] {
        return upsample_host_impl(device, width, height, mean_lo, count_lo, position, normal, albedo, hit_index, params, mean_rgb, count_out,
                                  kernel_ms);
    });
}

}  // extern "C"
