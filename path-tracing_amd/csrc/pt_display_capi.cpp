// Host side of the device-resident display path (include/pt_hip.h: pt_display_*): the threshold table made from the host's own
// tone map, the chain features -> temporal merge -> a-trous -> (upsample ->) bytes on the stream of the session it displays, and the few
// pixels the kernel leaves to the host.  With grading (pt_display_present_graded): the meter and the exposure kernel before the
// display kernel, the exposure in a device scalar, and deferred pixels finished through pt_grade.hpp.  With bloom
// (pt_display_present_bloom): the bloom kernels between the exposure and the display kernel, which then reads the bloomed means.
#include "pt_capi_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "pt_bloom.hpp"
#include "pt_display.hpp"
#include "pt_display_table.hpp"
#include "pt_meter.hpp"

using ptc::fail;
using ptc::guarded;
using ptc::hip_fail;

namespace {

using ptc::DisplayTable;
static_assert(ptc::kDisplayMaxLevels == pt::kDisplayTableSize, "the kernel searches a table of the builder's length");

int check_gamma(float gamma) {
    if (!std::isfinite(gamma) || !(gamma > 0.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "display: gamma must be finite and > 0");
    return PT_OK;
}

// One table per gamma (its bit pattern), built on first use: about 650 000 calls of powf.
std::shared_ptr<const DisplayTable> display_table(float gamma) {
    static std::mutex mutex;
    static std::vector<std::shared_ptr<const DisplayTable>> cache;   // most recent last; a handful of gammas at most
    std::lock_guard<std::mutex> lock(mutex);
    for (const auto &t : cache)
        if (std::memcmp(&t->gamma, &gamma, sizeof gamma) == 0) return t;
    auto t = std::make_shared<DisplayTable>();
    t->gamma = gamma;
    ptc::build_display_table([gamma](float m, int k) { return ptc::tonemap_value(m, gamma) >= static_cast<float>(k); }, *t);
    if (cache.size() >= 8) cache.erase(cache.begin());
    cache.push_back(t);
    return t;
}

// What the kernel would have written for a pixel it deferred: the host's own two steps.
void finish_on_host(const std::vector<pt::DisplayDeferred> &list, float gamma, uint8_t *bgr) {
    for (const pt::DisplayDeferred &d : list) {
        const size_t p = static_cast<size_t>(d.pixel);
        bgr[3 * p + 0] = ptc::quantize_value(ptc::tonemap_value(d.mean[2], gamma));
        bgr[3 * p + 1] = ptc::quantize_value(ptc::tonemap_value(d.mean[1], gamma));
        bgr[3 * p + 2] = ptc::quantize_value(ptc::tonemap_value(d.mean[0], gamma));
    }
}
// The same for a graded image: the list carries the ungraded mean, the grade is the host chain's own (pt_grade.hpp).
void finish_on_host_graded(const std::vector<pt::DisplayDeferred> &list, float gamma, int curve, float e, uint8_t *bgr) {
    for (const pt::DisplayDeferred &d : list) {
        const size_t p = static_cast<size_t>(d.pixel);
        for (int k = 0; k < 3; ++k)
            bgr[3 * p + k] = ptc::quantize_value(ptc::tonemap_value(pt::grade_value(curve, d.mean[2 - k], e), gamma));
    }
}

// What a graded present is asked for: the checked parameters, and the display's previous metered exposure.
struct GradeRequest {
    ptc::GradeSetup setup;
    bool has_prev = false;
    float e_prev = 0.0f;
    ptc::BloomSetup bloom;   // on: the bloom kernels run between the exposure and the display kernel
    int32_t width = 0, height = 0;   // of the image the display kernel reads (bloom needs its shape)
};

// ---- what one image needs on its device -------------------------------------------------------------------------------
// The table of the gamma used last, the output bytes, the deferred list and its length.
struct DisplayDevice {
    static constexpr size_t kExposureAt = (4 * pt::kMeterEntries + 15) / 16 * 16, kGradeBytes = kExposureAt + sizeof(pt::ExposureOut);
    size_t n = 0;
    ptc::DeviceBuffer d_table, d_out;
    float *table = nullptr, *band_lo = nullptr, *band_hi = nullptr;
    uint32_t *bgr = nullptr, *n_deferred = nullptr;
    pt::DisplayDeferred *deferred = nullptr;
    uint32_t *hist = nullptr;               // grading: the meter's histogram and, behind it, what the exposure kernel writes --
    pt::ExposureOut *exposure = nullptr;    // cleared together on the stream of every graded present
    std::shared_ptr<const DisplayTable> host;   // what d_table holds
    size_t band_room = 0;
    // bloom: the deepest pyramid of the image and the plane of bloomed means, allocated by the first bloomed present
    ptc::DeviceBuffer d_bloom;
    void *pyramid = nullptr;
    float *bloomed = nullptr;

    int alloc(size_t pixels, const char *what) {
        n = pixels;
        d_bloom.reset();   // (of another size's image)
        ptc::PlaneLayout l;
        const size_t o_bgr = l.add((n + 3) / 4 * 12), o_list = l.add(16 * n), o_len = l.add(4);
        const size_t o_grade = l.add(kGradeBytes);
        const int rc = d_out.alloc(l, what);
        if (rc != PT_OK) return rc;
        hist = d_out.at<uint32_t>(o_grade);
        exposure = d_out.at<pt::ExposureOut>(o_grade + kExposureAt);
        bgr = d_out.at<uint32_t>(o_bgr);
        deferred = d_out.at<pt::DisplayDeferred>(o_list);
        n_deferred = d_out.at<uint32_t>(o_len);
        return PT_OK;
    }
    int ensure_bloom(int32_t width, int32_t height, const char *what) {
        if (d_bloom) return PT_OK;
        ptc::PlaneLayout l;
        const size_t o_out = l.add(12 * n), o_pyr = l.add(16 * pt::bloom_pyramid_records(width, height, pt::kBloomMaxLevels));
        const int rc = d_bloom.alloc(l, what);
        if (rc != PT_OK) return rc;
        bloomed = d_bloom.at<float>(o_out); pyramid = d_bloom.at<void>(o_pyr);
        return PT_OK;
    }
    // (no kernel of this object is in flight: every call that launches one waits for it)
    int use_table(const std::shared_ptr<const DisplayTable> &t, const char *what) {
        if (host == t) return PT_OK;
        host.reset();
        const size_t bands = t->band_lo.size();
        if (!d_table || bands > band_room) {
            ptc::PlaneLayout l;
            const size_t o_t = l.add(4 * pt::kDisplayTableSize), o_lo = l.add(4 * std::max<size_t>(bands, 1)), o_hi = l.add(4 * std::max<size_t>(bands, 1));
            const int rc = d_table.alloc(l, what);
            if (rc != PT_OK) return rc;
            table = d_table.at<float>(o_t); band_lo = d_table.at<float>(o_lo); band_hi = d_table.at<float>(o_hi);
            band_room = std::max<size_t>(bands, 1);
        }
        std::vector<float> padded(pt::kDisplayTableSize, INFINITY);
        std::copy(t->thresholds.begin(), t->thresholds.end(), padded.begin());
        PT_HIP_TRY(hipMemcpy(table, padded.data(), 4 * padded.size(), hipMemcpyHostToDevice));
        if (bands) {
            PT_HIP_TRY(hipMemcpy(band_lo, t->band_lo.data(), 4 * bands, hipMemcpyHostToDevice));
            PT_HIP_TRY(hipMemcpy(band_hi, t->band_hi.data(), 4 * bands, hipMemcpyHostToDevice));
        }
        host = t;
        return PT_OK;
    }
    // Zero the list's length and launch the kernel on `stream`; with `grade`, the exposure first -- metered from the image the
    // kernel is about to read, or the manual one written into the device scalar -- and then the graded kernel.
    int enqueue(const float *rgb, const int32_t *count, bool divide, hipStream_t stream, const GradeRequest *grade = nullptr) {
        pt::DisplayArgs a;
        a.n = static_cast<int>(n);
        a.divide = divide ? 1 : 0;
        a.rgb = rgb; a.count = count;
        a.table = table;
        a.last = host->thresholds.empty() ? 0.0f : host->thresholds.back();   // (no level at all: everything is the host's)
        a.n_bands = static_cast<int>(host->band_lo.size());
        a.band_lo = band_lo; a.band_hi = band_hi;
        a.bgr = bgr; a.deferred = deferred; a.n_deferred = n_deferred;
        PT_HIP_TRY(hipMemsetAsync(n_deferred, 0, 4, stream));
        if (!grade) {
            PT_HIP_TRY(pt::launch_display(a, stream));
            return PT_OK;
        }
        PT_HIP_TRY(hipMemsetAsync(hist, 0, kGradeBytes, stream));
        if (grade->setup.automatic) {
            pt::MeterArgs m;
            m.n = a.n; m.divide = a.divide; m.rgb = rgb; m.count = count; m.hist = hist;
            PT_HIP_TRY(pt::launch_meter(m, stream));
            PT_HIP_TRY(pt::launch_exposure(hist, grade->setup.rule, grade->has_prev, grade->e_prev, exposure, stream));
        } else {
            uint32_t bits;
            std::memcpy(&bits, &grade->setup.exposure, sizeof bits);
            PT_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&exposure->exposure), static_cast<int>(bits), 1, stream));
        }
        if (grade->bloom.on) {   // the display kernel reads m + A * weight, a plane of means, with the chain's count
            pt::BloomArgs b;
            b.width = grade->width; b.height = grade->height; b.levels = grade->bloom.levels; b.divide = a.divide;
            b.rgb = rgb; b.count = count; b.exposure = &exposure->exposure;
            b.threshold = grade->bloom.threshold; b.weight = grade->bloom.weight;
            b.pyramid = pyramid; b.out_rgb = bloomed;
            PT_HIP_TRY(pt::launch_bloom(b, stream));
            a.rgb = bloomed; a.divide = 0;
        }
        PT_HIP_TRY(pt::launch_display_graded(a, grade->setup.curve, &exposure->exposure, stream));
        return PT_OK;
    }
    // The kernel has finished: 3 bytes per pixel and the deferred list come to the host, which finishes the list's pixels.
    int collect(float gamma, uint8_t *out, int32_t *n_deferred_out, const GradeRequest *grade = nullptr, pt_grade_info *used = nullptr) {
        PT_HIP_TRY(hipMemcpy(out, bgr, 3 * n, hipMemcpyDeviceToHost));
        if (grade) {
            pt::ExposureOut o;
            PT_HIP_TRY(hipMemcpy(&o, exposure, sizeof o, hipMemcpyDeviceToHost));
            used->exposure = o.exposure;
            used->target = grade->setup.automatic ? o.target : o.exposure;
            used->metered = o.metered; used->dark = o.dark;
        }
        uint32_t len = 0;
        PT_HIP_TRY(hipMemcpy(&len, n_deferred, 4, hipMemcpyDeviceToHost));
        if (len > n) return fail(PT_ERR_HIP, "display: the deferred list is longer than the image");
        if (len) {
            std::vector<pt::DisplayDeferred> list(len);
            PT_HIP_TRY(hipMemcpy(list.data(), deferred, sizeof(pt::DisplayDeferred) * len, hipMemcpyDeviceToHost));
            for (const pt::DisplayDeferred &d : list)
                if (d.pixel < 0 || static_cast<size_t>(d.pixel) >= n) return fail(PT_ERR_HIP, "display: a deferred pixel lies outside the image");
            if (grade) finish_on_host_graded(list, gamma, grade->setup.curve, used->exposure, out);
            else finish_on_host(list, gamma, out);
        }
        *n_deferred_out = static_cast<int32_t>(len);
        return PT_OK;
    }
    void fill(pt_display_info *info, float ms, int32_t n_def) const {
        if (!info) return;
        info->kernel_ms = ms;
        info->deferred_pixels = n_def;
        info->table_levels = static_cast<int32_t>(host->thresholds.size());
        info->doubt_bands = static_cast<int32_t>(host->band_lo.size());
    }
};

static_assert(sizeof(pt::DisplayDeferred) == 16, "a deferred entry is one 16-byte store");

}  // namespace

struct pt_display {
    pt_session *session = nullptr;   // one of the two
    pt_frame *frame = nullptr;
    pt_scene *scene = nullptr;       // the session's, or the root copy of the frame's
    int32_t width = 0, height = 0;
    float eps = 0;
    size_t n = 0;
    std::mutex mutex;                // one present / reset at a time
    DisplayDevice dev;
    pt_temporal *history = nullptr;  // created by the first present with a temporal stage
    // a filter without a temporal stage: the view's features and the denoiser's planes, allocated by the first such present
    ptc::DeviceBuffer d_filter;
    float *d_origins = nullptr, *d_directions = nullptr, *d_position = nullptr, *d_normal = nullptr, *d_albedo = nullptr, *d_hit_t = nullptr, *d_mean = nullptr;
    int32_t *d_hit = nullptr, *d_mean_count = nullptr;
    void *dn_a0 = nullptr, *dn_a1 = nullptr, *dn_b = nullptr, *dn_c = nullptr;
    // a scaled present: the output image's features, mean and count, the low mean and the upsampler's records, and the output's
    // bytes and deferred list -- allocated by the first scaled present, again when the scale changes
    int32_t up_scale = 0;
    ptc::DeviceBuffer d_up;
    DisplayDevice dev_up;
    float *up_origins = nullptr, *up_directions = nullptr, *up_position = nullptr, *up_normal = nullptr, *up_albedo = nullptr, *up_hit_t = nullptr,
          *up_mean = nullptr, *up_mean_lo = nullptr;
    int32_t *up_hit = nullptr, *up_count = nullptr;
    void *up_a = nullptr, *up_b = nullptr, *up_c = nullptr;
    ptc::DeviceEvent ev0, ev1;
    bool has_exposure = false;       // the e of the last metered present (pt_display_present_graded), until a reset
    float exposure = 0.0f;
    ~pt_display() {
        (void)hipSetDevice(scene->device);
        pt_temporal_destroy(history);
    }
};

namespace {

int display_create_impl(pt_scene *scene, int32_t width, int32_t height, float eps, std::unique_ptr<pt_display> &d) {
    if (static_cast<long long>(width) * height > 0x7fffffffLL / 4) return fail(PT_ERR_INVALID_ARGUMENT, "image too large");
    if (std::isnan(eps)) return fail(PT_ERR_INVALID_ARGUMENT, "eps is not a number");
    if (scene->device < 0) return fail(PT_ERR_NO_DEVICE, "scene was created without a device (device < 0); there is no CPU fallback");
    PT_HIP_TRY(hipSetDevice(scene->device));
    d.reset(new pt_display);
    d->scene = scene; d->width = width; d->height = height; d->eps = eps;
    d->n = static_cast<size_t>(width) * height;
    int rc;
    if ((rc = d->dev.alloc(d->n, "pt_display_create")) != PT_OK || (rc = d->ev0.create("pt_display_create")) != PT_OK ||
        (rc = d->ev1.create("pt_display_create")) != PT_OK)
        return rc;
    return PT_OK;
}

// What a scaled present needs on the device for scale s (the caller holds d->mutex and has made the device current).
int ensure_scaled(pt_display *d, int32_t s) {
    if (d->up_scale == s) return PT_OK;
    d->up_scale = 0;
    const size_t n_lo = d->n, n = n_lo * static_cast<size_t>(s) * s;
    ptc::PlaneLayout l;
    const size_t o_org = l.add(12 * n), o_dir = l.add(12 * n), o_pos = l.add(12 * n), o_nrm = l.add(12 * n), o_alb = l.add(12 * n), o_mean = l.add(12 * n);
    const size_t o_hit = l.add(4 * n), o_hit_t = l.add(4 * n), o_cnt = l.add(4 * n);
    const size_t o_mlo = l.add(12 * n_lo), o_a = l.add(16 * n_lo), o_b = l.add(16 * n_lo), o_c = l.add(16 * n_lo);
    int rc;
    if ((rc = d->d_up.alloc(l, "pt_display_present_scaled")) != PT_OK || (rc = d->dev_up.alloc(n, "pt_display_present_scaled")) != PT_OK) return rc;
    d->dev_up.host.reset();   // (a new allocation holds no table yet)
    const ptc::DeviceBuffer &b = d->d_up;
    d->up_origins = b.at<float>(o_org); d->up_directions = b.at<float>(o_dir); d->up_position = b.at<float>(o_pos);
    d->up_normal = b.at<float>(o_nrm); d->up_albedo = b.at<float>(o_alb); d->up_mean = b.at<float>(o_mean);
    d->up_hit = b.at<int32_t>(o_hit); d->up_hit_t = b.at<float>(o_hit_t); d->up_count = b.at<int32_t>(o_cnt);
    d->up_mean_lo = b.at<float>(o_mlo);
    d->up_a = b.at<void>(o_a); d->up_b = b.at<void>(o_b); d->up_c = b.at<void>(o_c);
    d->up_scale = s;
    return PT_OK;
}

// `u` = NULL: pt_display_present.  Else the scaled present: the same chain at the display's size, then the upsample to s times it.
// `g` = NULL: no grading.  Else pt_display_present_graded: the exposure and the graded kernel in place of the display kernel.
// `b` (with `g` only): pt_display_present_bloom.
int display_present_impl(pt_display *d, const pt_display_params *p, const pt_upsample_params *u, bool scaled, uint8_t *bgr, pt_display_info *info,
                         const pt_grade_params *g = nullptr, bool graded = false, pt_grade_info *grade_info = nullptr,
                         const pt_bloom_params *b = nullptr, bool bloomed = false) {
    if (!d || !p || !bgr || (scaled && !u) || (graded && !g) || (bloomed && !b)) return fail(PT_ERR_INVALID_ARGUMENT, "null handle, params or image");
    int rc = check_gamma(p->gamma);
    if (rc != PT_OK) return rc;
    GradeRequest grade;
    if (graded && (rc = ptc::grade_params_check(g, grade.setup)) != PT_OK) return rc;
    if (bloomed && (rc = ptc::bloom_params_check(b, grade.bloom)) != PT_OK) return rc;
    pt::UpsampleArgs ua;
    if (scaled) {
        if (u->scale < pt::kUpsampleMinScale || u->scale > pt::kUpsampleMaxScale) return fail(PT_ERR_INVALID_ARGUMENT, "upsample: scale must be 2, 3 or 4");
        if ((rc = ptc::upsample_params_to_args(u, d->width * u->scale, d->height * u->scale, ua)) != PT_OK) return rc;
    }
    pt::DenoiseArgs da;
    if ((rc = ptc::denoise_params_to_args(&p->denoise, da)) != PT_OK) return rc;
    const bool temporal = p->temporal != 0, filter = da.levels > 0;
    std::lock_guard<std::mutex> present_lock(d->mutex);
    grade.has_prev = d->has_exposure; grade.e_prev = d->exposure;
    const std::shared_ptr<const DisplayTable> table = display_table(p->gamma);
    const size_t n = d->n;
    // the accumulators, where they lie, and the stream their slices were enqueued on: the chain goes behind them
    ptc::AccumPlanes planes;
    hipStream_t stream = nullptr;
    if (d->frame) {
        pt_scene *root = nullptr;
        int32_t w = 0, h = 0;
        if ((rc = ptc::frame_root_planes(d->frame, &root, &planes, &stream, &w, &h)) != PT_OK) return rc;
    } else {
        planes = d->session->planes;
        stream = d->session->stream.get();
    }
    pt_scene *scene = d->scene;
    PT_HIP_TRY(hipSetDevice(scene->device));
    DisplayDevice &dev = scaled ? d->dev_up : d->dev;
    if (scaled && (rc = ensure_scaled(d, ua.scale)) != PT_OK) return rc;
    if ((rc = dev.use_table(table, "pt_display_present")) != PT_OK) return rc;
    grade.width = scaled ? ua.width : d->width; grade.height = scaled ? ua.height : d->height;
    if (grade.bloom.on && (rc = dev.ensure_bloom(grade.width, grade.height, "pt_display_present_bloom")) != PT_OK) return rc;
    if (temporal && !d->history && (rc = pt_temporal_create(scene, d->width, d->height, d->eps, &d->history)) != PT_OK) return rc;
    if (filter && !temporal && !d->d_filter) {
        ptc::PlaneLayout l;
        const size_t o_org = l.add(12 * n), o_dir = l.add(12 * n), o_pos = l.add(12 * n), o_nrm = l.add(12 * n), o_alb = l.add(12 * n), o_mean = l.add(12 * n);
        const size_t o_hit = l.add(4 * n), o_hit_t = l.add(4 * n), o_cnt = l.add(4 * n);
        const size_t o_a0 = l.add(16 * n), o_a1 = l.add(16 * n), o_b = l.add(16 * n), o_c = l.add(16 * n);
        if ((rc = d->d_filter.alloc(l, "pt_display_present")) != PT_OK) return rc;
        const ptc::DeviceBuffer &b = d->d_filter;
        d->d_origins = b.at<float>(o_org); d->d_directions = b.at<float>(o_dir); d->d_position = b.at<float>(o_pos);
        d->d_normal = b.at<float>(o_nrm); d->d_albedo = b.at<float>(o_alb); d->d_mean = b.at<float>(o_mean);
        d->d_hit = b.at<int32_t>(o_hit); d->d_hit_t = b.at<float>(o_hit_t); d->d_mean_count = b.at<int32_t>(o_cnt);
        d->dn_a0 = b.at<void>(o_a0); d->dn_a1 = b.at<void>(o_a1); d->dn_b = b.at<void>(o_b); d->dn_c = b.at<void>(o_c);
    }
    {   // the chain, behind every slice enqueued so far: no host synchronisation until its last kernel is in the queue
        std::unique_lock<std::mutex> ctx_lock;
        if (d->session) ctx_lock = std::unique_lock<std::mutex>(d->session->ctx.mutex);
        PT_HIP_TRY(hipEventRecord(d->ev0.get(), stream));
        const float *rgb = planes.sum;
        const int32_t *count = planes.count;
        bool divide = true;
        if (temporal) {
            ptc::TemporalPlanes merged;
            if ((rc = ptc::temporal_enqueue(d->history, planes, &p->temporal_params, filter ? &p->denoise : nullptr, stream, &merged)) != PT_OK) return rc;
            rgb = filter ? merged.mean : merged.merged.sum;
            count = filter ? merged.mean_count : merged.merged.count;
            divide = !filter;
        } else if (filter) {
            std::lock_guard<std::mutex> launch_lock(scene->launch_mutex);
            pt::RenderArgs ra;
            if ((rc = ptc::scene_trace_args(scene, d->eps, ra)) != PT_OK) return rc;
            rc = ptc::enqueue_first_hits(scene, ra, ptc::view_camera(scene), d->width, d->height, 0, d->height, d->d_origins, d->d_directions, d->d_hit,
                                         d->d_hit_t, d->d_position, d->d_normal, d->d_albedo, stream);
            if (rc != PT_OK) return rc;
            da.width = d->width; da.height = d->height;
            da.sum = planes.sum; da.sum2 = planes.sum2; da.count = planes.count;
            da.position = d->d_position; da.normal = d->d_normal; da.albedo = d->d_albedo; da.hit_index = d->d_hit;
            da.rec_a0 = d->dn_a0; da.rec_a1 = d->dn_a1; da.rec_b = d->dn_b; da.rec_c = d->dn_c;
            da.mean_rgb = d->d_mean; da.count_out = d->d_mean_count;
            PT_HIP_TRY(pt::launch_denoise(da, stream));
            rgb = d->d_mean; count = d->d_mean_count;
            divide = false;
        }
        if (scaled) {
            // the low mean (levels = 0: sum / n of the accumulators as they are, or merged), the output image's features from the
            // same camera, the upsample; the bytes are then made from its mean and count
            if (divide) {
                PT_HIP_TRY(pt::launch_upsample_mean(rgb, count, static_cast<int>(n), d->up_mean_lo, stream));
                rgb = d->up_mean_lo;
            }
            {
                std::lock_guard<std::mutex> launch_lock(scene->launch_mutex);
                pt::RenderArgs ra;
                if ((rc = ptc::scene_trace_args(scene, d->eps, ra)) != PT_OK) return rc;
                rc = ptc::enqueue_first_hits(scene, ra, ptc::view_camera(scene), ua.width, ua.height, 0, ua.height, d->up_origins, d->up_directions,
                                             d->up_hit, d->up_hit_t, d->up_position, d->up_normal, d->up_albedo, stream);
                if (rc != PT_OK) return rc;
            }
            ua.mean_lo = rgb; ua.count_lo = count;
            ua.position = d->up_position; ua.normal = d->up_normal; ua.albedo = d->up_albedo; ua.hit_index = d->up_hit;
            ua.rec_a = d->up_a; ua.rec_b = d->up_b; ua.rec_c = d->up_c;
            ua.mean_rgb = d->up_mean; ua.count_out = d->up_count;
            PT_HIP_TRY(pt::launch_upsample(ua, stream));
            rgb = d->up_mean; count = d->up_count;
            divide = false;
        }
        if ((rc = dev.enqueue(rgb, count, divide, stream, graded ? &grade : nullptr)) != PT_OK) return rc;
        PT_HIP_TRY(hipEventRecord(d->ev1.get(), stream));
    }
    // (an error return from here on leaves the history and the metered exposure as they were: they were only read)
    PT_HIP_TRY(hipEventSynchronize(d->ev1.get()));
    float ms = 0.0f;
    PT_HIP_TRY(hipEventElapsedTime(&ms, d->ev0.get(), d->ev1.get()));
    int32_t n_deferred = 0;
    pt_grade_info used{};
    if ((rc = dev.collect(p->gamma, bgr, &n_deferred, graded ? &grade : nullptr, &used)) != PT_OK) return rc;
    if (temporal) ptc::temporal_commit(d->history);
    if (graded && grade.setup.automatic) {
        d->has_exposure = true;
        d->exposure = used.exposure;
    }
    if (graded && grade_info) *grade_info = used;
    dev.fill(info, ms, n_deferred);
    return PT_OK;
}

// `g` = NULL: pt_display_bytes_host.  Else pt_display_bytes_graded_host.
int display_bytes_host_impl(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float gamma,
                            uint8_t *bgr, pt_display_info *info, const pt_grade_params *g = nullptr, bool graded = false, bool has_prev = false,
                            float e_prev = 0.0f, pt_grade_info *grade_info = nullptr) {
    if (width <= 0 || height <= 0 || !mean_rgb || !count || !bgr || (graded && !g)) return fail(PT_ERR_INVALID_ARGUMENT, "null buffer or empty image");
    if (static_cast<long long>(width) * height > 0x7fffffffLL / 4) return fail(PT_ERR_INVALID_ARGUMENT, "image too large");
    int rc = check_gamma(gamma);
    if (rc != PT_OK) return rc;
    GradeRequest grade;
    if (graded && (rc = ptc::grade_params_check(g, grade.setup)) != PT_OK) return rc;
    grade.has_prev = has_prev; grade.e_prev = e_prev;
    if ((rc = ptc::use_device(device, "display")) != PT_OK) return rc;
    const size_t n = static_cast<size_t>(width) * height;
    const std::shared_ptr<const DisplayTable> table = display_table(gamma);
    DisplayDevice dev;
    ptc::PlaneLayout l;
    const size_t o_mean = l.add(12 * n), o_cnt = l.add(4 * n);
    ptc::DeviceBuffer d_in;
    ptc::DeviceEvent ev0, ev1;
    if ((rc = d_in.alloc(l, "pt_display_bytes_host")) != PT_OK || (rc = dev.alloc(n, "pt_display_bytes_host")) != PT_OK ||
        (rc = dev.use_table(table, "pt_display_bytes_host")) != PT_OK || (rc = ev0.create("pt_display_bytes_host")) != PT_OK ||
        (rc = ev1.create("pt_display_bytes_host")) != PT_OK)
        return rc;
    PT_HIP_TRY(hipMemcpy(d_in.at<void>(o_mean), mean_rgb, 12 * n, hipMemcpyHostToDevice));
    PT_HIP_TRY(hipMemcpy(d_in.at<void>(o_cnt), count, 4 * n, hipMemcpyHostToDevice));
    PT_HIP_TRY(hipEventRecord(ev0.get(), nullptr));
    if ((rc = dev.enqueue(d_in.at<float>(o_mean), d_in.at<int32_t>(o_cnt), false, nullptr, graded ? &grade : nullptr)) != PT_OK) return rc;
    PT_HIP_TRY(hipEventRecord(ev1.get(), nullptr));
    PT_HIP_TRY(hipEventSynchronize(ev1.get()));
    float ms = 0.0f;
    PT_HIP_TRY(hipEventElapsedTime(&ms, ev0.get(), ev1.get()));
    int32_t n_deferred = 0;
    pt_grade_info used{};
    if ((rc = dev.collect(gamma, bgr, &n_deferred, graded ? &grade : nullptr, &used)) != PT_OK) return rc;
    if (graded && grade_info) *grade_info = used;
    dev.fill(info, ms, n_deferred);
    return PT_OK;
}

int display_table_impl(float gamma, int32_t *levels, float *thresholds, float *doubt_lo, float *doubt_hi) {
    if (!levels) return fail(PT_ERR_INVALID_ARGUMENT, "null levels");
    const int rc = check_gamma(gamma);
    if (rc != PT_OK) return rc;
    const std::shared_ptr<const DisplayTable> t = display_table(gamma);
    const size_t k = t->thresholds.size();
    *levels = static_cast<int32_t>(k);
    if (thresholds) std::copy(t->thresholds.begin(), t->thresholds.end(), thresholds);
    if (doubt_lo) std::copy(t->doubt_lo.begin(), t->doubt_lo.end(), doubt_lo);
    if (doubt_hi) std::copy(t->doubt_hi.begin(), t->doubt_hi.end(), doubt_hi);
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_display_create(pt_session *session, float eps, pt_display **out) {
    return guarded([&] {
        if (!out) return fail(PT_ERR_INVALID_ARGUMENT, "null output pointer");
        *out = nullptr;
        if (!session) return fail(PT_ERR_INVALID_ARGUMENT, "null session");
        if (session->row_begin != 0 || session->row_end != session->height || session->row_stride > 1)
            return fail(PT_ERR_UNSUPPORTED, "a display shows a whole image: the session must cover rows 0 .. height with row_stride 0 / 1 "
                                            "(a pt_frame displays an image rendered in bands)");
        std::unique_ptr<pt_display> d;
        const int rc = display_create_impl(session->scene, session->width, session->height, eps, d);
        if (rc != PT_OK) return rc;
        d->session = session;
        *out = d.release();
        return static_cast<int>(PT_OK);
    });
}

int pt_display_create_frame(pt_frame *frame, float eps, pt_display **out) {
    return guarded([&] {
        if (!out) return fail(PT_ERR_INVALID_ARGUMENT, "null output pointer");
        *out = nullptr;
        if (!frame) return fail(PT_ERR_INVALID_ARGUMENT, "null frame");
        pt_scene *root = nullptr;
        ptc::AccumPlanes planes;
        hipStream_t stream = nullptr;
        int32_t w = 0, h = 0;
        int rc = ptc::frame_root_planes(frame, &root, &planes, &stream, &w, &h);
        if (rc != PT_OK) return rc;
        std::unique_ptr<pt_display> d;
        if ((rc = display_create_impl(root, w, h, eps, d)) != PT_OK) return rc;
        d->frame = frame;
        *out = d.release();
        return static_cast<int>(PT_OK);
    });
}

int pt_display_present(pt_display *d, const pt_display_params *p, uint8_t *bgr, pt_display_info *info) {
    return guarded([&] { return display_present_impl(d, p, nullptr, false, bgr, info); });
}

int pt_display_present_scaled(pt_display *d, const pt_display_params *p, const pt_upsample_params *u, uint8_t *bgr, pt_display_info *info) {
    return guarded([&] { return display_present_impl(d, p, u, true, bgr, info); });
}

int pt_display_present_graded(pt_display *d, const pt_display_params *p, const pt_upsample_params *u, const pt_grade_params *g, uint8_t *bgr,
                              pt_display_info *info, pt_grade_info *grade_info) {
    return guarded([&] { return display_present_impl(d, p, u, u != nullptr, bgr, info, g, true, grade_info); });
}

int pt_display_present_bloom(pt_display *d, const pt_display_params *p, const pt_upsample_params *u, const pt_grade_params *g,
                             const pt_bloom_params *b, uint8_t *bgr, pt_display_info *info, pt_grade_info *grade_info) {
    return guarded([&] { return display_present_impl(d, p, u, u != nullptr, bgr, info, g, true, grade_info, b, true); });
}

int pt_display_reset(pt_display *d) {
    return guarded([&] {
        if (!d) return fail(PT_ERR_INVALID_ARGUMENT, "null handle");
        std::lock_guard<std::mutex> lock(d->mutex);
        const int rc = d->history ? pt_temporal_reset(d->history) : static_cast<int>(PT_OK);
        if (rc == PT_OK) d->has_exposure = false;   // the next metered present is a first one
        return rc;
    });
}

void pt_display_destroy(pt_display *d) {
    delete d;   // (~pt_display makes the scene's device current for its owners)
}

int pt_display_bytes_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float gamma,
                          uint8_t *bgr, pt_display_info *info) {
    return guarded([&] { return display_bytes_host_impl(device, width, height, mean_rgb, count, gamma, bgr, info); });
}

int pt_display_bytes_graded_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float gamma,
                                 const pt_grade_params *g, int32_t has_prev, float e_prev, uint8_t *bgr, pt_display_info *info,
                                 pt_grade_info *grade_info) {
    return guarded([&] {
        return display_bytes_host_impl(device, width, height, mean_rgb, count, gamma, bgr, info, g, true, has_prev != 0, e_prev, grade_info);
    });
}

int pt_display_table(float gamma, int32_t *levels, float *thresholds, float *doubt_lo, float *doubt_hi) {
    return guarded([&] { return display_table_impl(gamma, levels, thresholds, doubt_lo, doubt_hi); });
}

}  // extern "C"
