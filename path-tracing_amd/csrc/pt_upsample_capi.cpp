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
    if (const int rc = check_image_size(width, height, "upsample: ")) return rc;
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
    // one allocation: the low image, the output image's features, mean and count, the upsampler's records
    ptc::PlaneLayout l;
    ptc::MeanPlanes lo = ptc::MeanPlanes::in(l, n_lo);
    ptc::FeaturePlanes f = ptc::FeaturePlanes::uploaded_in(l, n);
    ptc::MeanPlanes out = ptc::MeanPlanes::in(l, n);
    ptc::UpsamplePlanes work = ptc::UpsamplePlanes::in(l, n_lo, false);
    ptc::DeviceBuffer d;
    if ((rc = d.alloc(l, "pt_upsample_host")) != PT_OK) return rc;
    lo.bind(d); f.bind(d); out.bind(d); work.bind(d);
    ptc::bind_planes(a, lo.rgb, lo.count, f, work, out);
    if ((rc = lo.upload(mean_lo, count_lo)) != PT_OK || (rc = f.upload(position, normal, albedo, hit_index)) != PT_OK) return rc;
    float ms = 0.0f;
    if ((rc = ptc::timed(nullptr, "pt_upsample_host", &ms, [&]() -> int { PT_HIP_TRY(pt::launch_upsample(a, nullptr)); return PT_OK; })) != PT_OK) return rc;
    if ((rc = out.download(mean_rgb, count_out)) != PT_OK) return rc;
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
