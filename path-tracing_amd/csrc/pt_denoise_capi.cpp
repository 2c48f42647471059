// Host side of the first-hit feature buffers and of the denoiser (include/pt_hip.h: pt_render_features_host, pt_denoise_host):
// argument checks, device buffers, the launches of pt_denoise.hip.
#include "pt_capi_internal.hpp"

#include <cmath>
#include <cstring>

#include "pt_denoise.hpp"
#include "pt_smooth_features.hpp"
#include "pt_texture_features.hpp"

using ptc::fail;
using ptc::guarded;
using ptc::hip_fail;

int ptc::enqueue_first_hits(pt_scene *scene, const pt::RenderArgs &a, const pt_camera &camera, int32_t width, int32_t height, int32_t row_begin,
                            int32_t rows, const FeaturePlanes &out, hipStream_t stream) {
    pt::FeatureCamera cam;
    std::memcpy(cam.v, &camera, sizeof cam.v);
    const int n = rows * width;
    // (a.projection != 0: the handle's non-perspective projection, of the handle's own camera -- the one spelling of its ray,
    // pt_projection.hpp, which the integrator traced; the temporal stage, the one caller with another camera, refuses such a handle)
    if (a.projection != 0) PT_HIP_TRY(pt::launch_projection_rays(a, width, height, row_begin, rows, out.origins, out.directions, stream));
    else PT_HIP_TRY(pt::launch_feature_rays(cam, width, height, row_begin, rows, out.origins, out.directions, stream));
    PT_HIP_TRY(pt::launch_trace_rays(a, out.origins, out.directions, n, out.hit, out.hit_t, stream));
    if (a.smooth_normals != nullptr)   // the handle's shading normals: normal = Ns, and the textured albedo as below (pt_smooth_features.hip)
        PT_HIP_TRY(pt::launch_feature_gather_smooth(scene->d_exact.get<pt::ExactRec>(), scene->d_mats.get<pt::MatRec>(), a.tex_recs, a.tex_uv, a.tex_texels, a.tex_bary,
                                                    a.smooth_normals, out.origins, out.directions, out.hit, out.hit_t, n, out.position, out.normal, out.albedo, stream));
    else if (a.tex_recs != nullptr)   // the handle's textures: the gather's twin, albedo = Kd x texel (pt_texture_features.hip)
        PT_HIP_TRY(pt::launch_feature_gather_textured(scene->d_exact.get<pt::ExactRec>(), scene->d_mats.get<pt::MatRec>(), a.tex_recs, a.tex_uv, a.tex_texels, a.tex_bary,
                                                      out.origins, out.directions, out.hit, out.hit_t, n, out.position, out.normal, out.albedo, stream));
    else
    PT_HIP_TRY(pt::launch_feature_gather(scene->d_exact.get<pt::ExactRec>(), scene->d_mats.get<pt::MatRec>(), out.origins, out.directions, out.hit,
                                         out.hit_t, n, out.position, out.normal, out.albedo, stream));
    return PT_OK;
}

// pt_render_features_host: centre rays on the device, the unchanged closest-hit search, then the hit's features.
// (`host`: where the caller wants the planes, NULL for those it does not.)
static int render_features_host_impl(pt_scene *scene, const pt_render_params *p, const ptc::FeaturePlanes &host) {
    if (!scene || !p) return fail(PT_ERR_INVALID_ARGUMENT, "null scene or params");
    if (p->width <= 0 || p->height <= 0) return fail(PT_ERR_INVALID_ARGUMENT, "width and height must be positive");
    if (p->row_begin < 0 || p->row_end > p->height || p->row_begin > p->row_end)
        return fail(PT_ERR_INVALID_ARGUMENT, "row band outside the image");
    if (p->row_stride < 0) return fail(PT_ERR_INVALID_ARGUMENT, "negative row_stride");
    if (p->row_stride > 1) return fail(PT_ERR_UNSUPPORTED, "feature buffers are rendered for contiguous rows only (row_stride 0 / 1)");
    if (static_cast<long long>(p->width) * p->height > 0x7fffffffLL) return fail(PT_ERR_INVALID_ARGUMENT, "image has more than 2^31 pixels");
    int rc = ptc::check_has_device(scene);
    if (rc != PT_OK) return rc;
    const int rows = p->row_end - p->row_begin;
    const size_t n = static_cast<size_t>(rows) * p->width;
    if (n == 0) return PT_OK;
    PT_HIP_TRY(hipSetDevice(scene->device));
    std::lock_guard<std::mutex> launch_lock(scene->launch_mutex);
    pt::RenderArgs a;
    if ((rc = ptc::scene_trace_args(scene, p->eps, a)) != PT_OK) return rc;
    ptc::PlaneLayout l;
    ptc::FeaturePlanes f = ptc::FeaturePlanes::in(l, n);
    ptc::DeviceBuffer d_all;
    if ((rc = d_all.alloc(l, "pt_render_features_host")) != PT_OK) return rc;
    f.bind(d_all);
    if ((rc = ptc::enqueue_first_hits(scene, a, ptc::view_camera(scene), p->width, p->height, p->row_begin, rows, f, nullptr)) != PT_OK) return rc;
    PT_HIP_TRY(hipDeviceSynchronize());
    return f.download(host);
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
    int rc = ptc::check_image_size(width, height);
    if (rc != PT_OK) return rc;
    pt::DenoiseArgs a;
    if ((rc = ptc::denoise_params_to_args(prm, a)) != PT_OK) return rc;
    const size_t n = static_cast<size_t>(width) * height;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (prm->levels == 0) {   // the unfiltered mean, on the host
        ptc::unfiltered_mean(n, sum, count, mean_rgb, count_out);
        return PT_OK;
    }
    if (!position || !normal || !albedo || !hit_index) return fail(PT_ERR_INVALID_ARGUMENT, "denoise: null feature buffer");
    if ((rc = ptc::use_device(device, "denoiser")) != PT_OK) return rc;
    // one allocation: the accumulators, the features, the denoiser's own planes
    ptc::PlaneLayout l;
    ptc::AccumPlanes acc = ptc::AccumPlanes::in(l, n);
    ptc::FeaturePlanes f = ptc::FeaturePlanes::uploaded_in(l, n);
    ptc::DenoisePlanes work = ptc::DenoisePlanes::in(l, n);
    ptc::DeviceBuffer d;
    if ((rc = d.alloc(l, "pt_denoise_host")) != PT_OK) return rc;
    acc.bind(d); f.bind(d); work.bind(d);
    a.width = width; a.height = height;
    ptc::bind_planes(a, acc, f, work);
    if ((rc = acc.upload(sum, sum2, count)) != PT_OK || (rc = f.upload(position, normal, albedo, hit_index)) != PT_OK) return rc;
    float ms = 0.0f;
    if ((rc = ptc::timed(nullptr, "pt_denoise_host", &ms, [&]() -> int { PT_HIP_TRY(pt::launch_denoise(a, nullptr)); return PT_OK; })) != PT_OK) return rc;
    if ((rc = work.out.download(mean_rgb, count_out)) != PT_OK) return rc;
    if (kernel_ms) *kernel_ms = ms;
    return PT_OK;
}


extern "C" {

int pt_render_features_host(pt_scene *scene, const pt_render_params *params, int32_t *hit_index, float *hit_t, float *position,
                            float *normal, float *albedo) {
    return guarded([&] {
        ptc::FeaturePlanes host;
        host.hit = hit_index; host.hit_t = hit_t; host.position = position; host.normal = normal; host.albedo = albedo;
        return render_features_host_impl(scene, params, host);
    });
}

int pt_denoise_host(int device, int32_t width, int32_t height, const float *sum, const float *sum2, const int32_t *count,
                    const float *position, const float *normal, const float *albedo, const int32_t *hit_index,
                    const pt_denoise_params *params, float *mean_rgb, int32_t *count_out, float *kernel_ms) {
    return guarded([&] {
        return denoise_host_impl(device, width, height, sum, sum2, count, position, normal, albedo, hit_index, params, mean_rgb, count_out, kernel_ms);
    });
}

}  // extern "C"
