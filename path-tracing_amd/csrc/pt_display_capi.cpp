// Host side of the device-resident display path (include/pt_hip.h: pt_display_*): the threshold table made from the host's own
// tone map, the chain features -> temporal merge -> a-trous -> (upsample ->) bytes on the stream of the session it displays, and the few
// pixels the kernel leaves to the host.  With grading (pt_display_present_graded): the meter and the exposure kernel before the
// display kernel, the exposure in a device scalar, and deferred pixels finished through pt_grade.hpp.  With bloom
// (pt_display_present_bloom): the bloom kernels between the exposure and the display kernel, which then reads the bloomed means.
// With local exposure (pt_display_present_local): its kernels behind bloom's, on the plane of means bloom wrote or on the chain's image.
// With colour grading (pt_display_present_colour): the colour display kernel in the graded one's place, its LUT in device memory of the
// display's, uploaded when the generation of the pt_lut given differs from the one held.
// With lens optics (pt_display_present_optics): its kernel ahead of all of these, from the chain's image into a mean image of the
// display's, which the meter and every later stage read in the chain's place.
// With sharpening (pt_display_present_sharpen): its two kernels behind local exposure's, immediately ahead of the graded or the colour
// kernel, in place on the plane of means a stage of the display's wrote, or from the chain's image into a plane of the display's.
// With grain or dither (pt_display_present_grain): the grain display kernel in the graded or the colour one's place, and deferred pixels
// finished with pt_grain.hpp from their index, the seed and the frame.
// With scene-linear output (pt_display_present_linear): the encode kernel (pt_linear.hip) immediately ahead of the display kernel, on the
// image that one reads, into a buffer of the display's that one more copy brings to the host.
#include "pt_capi_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "pt_display.hpp"
#include "pt_display_table.hpp"

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

}  // namespace

// One table per gamma (its bit pattern), built on first use: about 650 000 calls of powf.
std::shared_ptr<const ptc::DisplayTable> ptc::display_table(float gamma) {
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

namespace {

using ptc::display_table;

// What a graded present is asked for: the checked parameters, and the display's previous metered exposure.
struct GradeRequest {
    ptc::GradeSetup setup;
    bool has_prev = false;
    float e_prev = 0.0f;
    ptc::BloomSetup bloom;   // on: the bloom kernels run between the exposure and the display kernel
    ptc::LocalSetup local;   // on: the local exposure kernels run behind them
    ptc::ColourSetup colour; // on: the colour display kernel takes the graded one's place
    ptc::OpticsSetup optics; // on: the optics kernel runs ahead of the meter, and everything behind it reads what it wrote
    ptc::SharpenSetup sharpen;   // on: the sharpening kernels run last before the graded or the colour kernel
    ptc::GrainSetup grain;   // on: the grain display kernel takes the graded or the colour one's place
    // the image the chain hands to the stages is no plane of the display's: no stage ahead of sharpening writes one it may overwrite
    bool sharpen_own_mean() const { return !optics.on && !bloom.on && !local.on; }
};

// What the tone map gets for a pixel the kernel deferred, from the mean its entry carries: the mean itself (no exposure is
// multiplied in), the host chain's own grade of it (pt_grade.hpp), or matrix -> exposure -> curve -> LUT (pt_colour.hpp, on the
// host's LUT).  Three computations, none made of another: NaN payloads and -0 come out as each kernel's.
void deferred_value(const float *mean, const GradeRequest *grade, float e, float *v) {
    for (int k = 0; k < 3; ++k) v[k] = mean[k];
    if (!grade) return;
    if (grade->colour.on) pt::colour_pixel(grade->colour.step, grade->setup.curve, e, v[0], v[1], v[2]);
    else for (int k = 0; k < 3; ++k) v[k] = pt::grade_value(grade->setup.curve, mean[k], e);
}
// What the kernel would have written for the pixels it deferred: the host's own two steps on that value -- or, with grain or dither,
// pt_grain.hpp's on it and the table's or the host's on each channel of the result.
void finish_on_host(const std::vector<pt::DisplayDeferred> &list, float gamma, const DisplayTable &table, const GradeRequest *grade, float e,
                    uint8_t *bgr) {
    for (const pt::DisplayDeferred &d : list) {
        const size_t p = static_cast<size_t>(d.pixel);
        float v[3];
        deferred_value(d.mean, grade, e, v);
        if (grade && grade->grain.on) {
            const uint32_t width = static_cast<uint32_t>(grade->grain.step.width), pixel = static_cast<uint32_t>(d.pixel);
            uint8_t rgb[3];
            ptc::grain_pixel_bytes(grade->grain.step, table, gamma, pixel % width, pixel / width, v, rgb);
            for (int k = 0; k < 3; ++k) bgr[3 * p + k] = rgb[2 - k];
            continue;
        }
        for (int k = 0; k < 3; ++k) bgr[3 * p + k] = ptc::quantize_value(ptc::tonemap_value(v[2 - k], gamma));
    }
}
// Where scene-linear output goes on the device: the body, padded to the whole 16-byte groups the kernel writes (PFM's 12 bytes per pixel
// hold either format).
struct LinearPlane {
    uint32_t *out = nullptr;
    size_t offset = 0;
    static LinearPlane in(ptc::PlaneLayout &l, size_t n) {
        LinearPlane w;
        w.offset = l.add(pt::linear_room(n, pt::kLinearPfm));
        return w;
    }
    void bind(const ptc::DeviceBuffer &b) { out = b.at<uint32_t>(offset); }
};
// What collect brings back besides the bytes (used: of a graded image).
struct Presented { int32_t n_deferred = 0; pt_grade_info used{}; };

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
    ptc::BloomPlanes bloom;
    // local exposure: the two planes of the base and the plane of locally exposed means, allocated by the first present with the stage
    ptc::DeviceBuffer d_local;
    ptc::LocalPlanes local;
    // colour grading: the LUT of the last present with one, and the generation of the pt_lut it was copied from (0: none)
    ptc::DeviceBuffer d_lut;
    uint64_t lut_generation = 0;
    size_t lut_room = 0;
    // lens optics: the mean image the stage writes, allocated by the first present with it
    ptc::DeviceBuffer d_optics;
    ptc::MeanPlanes optics_out;
    // sharpening: the plane of compressed luminance and, for a chain in which no stage before it writes a plane of the display's, the
    // plane of sharpened means; allocated by the first present with the stage
    ptc::DeviceBuffer d_sharpen;
    ptc::SharpenPlanes sharpen;
    // scene-linear output: the encoded body, allocated by the first present with the stage
    ptc::DeviceBuffer d_linear;
    LinearPlane linear;

    int alloc(size_t pixels, const char *what) {
        n = pixels;
        d_bloom.reset();   // (of another size's image)
        d_local.reset();
        d_optics.reset();
        d_sharpen.reset();
        d_linear.reset();
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
    // A lazily made plane set: laid out, allocated and bound by the first present that needs it.
    template <class View, class... Sizes>
    static int ensure(ptc::DeviceBuffer &buffer, View &view, const char *what, Sizes... sizes) {
        if (buffer) return PT_OK;
        ptc::PlaneLayout l;
        view = View::in(l, sizes...);
        const int rc = buffer.alloc(l, what);
        if (rc == PT_OK) view.bind(buffer);
        return rc;
    }
    int ensure_bloom(int32_t width, int32_t height, const char *what) {
        return ensure(d_bloom, bloom, what, n, pt::bloom_pyramid_records(width, height, pt::kBloomMaxLevels));
    }
    int ensure_local(const char *what) { return ensure(d_local, local, what, n); }
    int ensure_optics(const char *what) { return ensure(d_optics, optics_out, what, n); }
    int ensure_sharpen(bool own_mean, const char *what) {
        if (d_sharpen && own_mean && !sharpen.own_mean) d_sharpen.reset();   // (made by a chain that needed the luminance alone)
        return ensure(d_sharpen, sharpen, what, n, own_mean);
    }
    int ensure_linear(const char *what) { return ensure(d_linear, linear, what, n); }
    // (no kernel of this object is in flight: every call that launches one waits for it)
    int use_lut(const pt_lut *lut, const char *what) {
        if (lut_generation == lut->generation) return PT_OK;
        lut_generation = 0;
        const size_t bytes = sizeof(pt::LutVertex) * lut->vertices.size();
        if (!d_lut || bytes > lut_room) {
            ptc::PlaneLayout l;
            l.add(bytes);
            const int rc = d_lut.alloc(l, what);
            if (rc != PT_OK) return rc;
            lut_room = bytes;
        }
        PT_HIP_TRY(hipMemcpy(d_lut.at<void>(0), lut->vertices.data(), bytes, hipMemcpyHostToDevice));
        lut_generation = lut->generation;
        return PT_OK;
    }
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
    // Zero the list's length and launch the kernel on `stream`; with `grade`, the stages ahead of the graded or the colour kernel first, each
    // on the image the one before it left: the lens, the exposure (metered from the image, or the manual one), bloom, local exposure,
    // sharpening.  With `lin` on, the encode of the image these leave goes immediately ahead of the display kernel; without `want_bgr`
    // that one is left out.
    int enqueue(ptc::Image image, hipStream_t stream, const GradeRequest *grade, const ptc::LinearSetup *lin = nullptr, bool want_bgr = true) {
        PT_HIP_TRY(hipMemsetAsync(n_deferred, 0, 4, stream));
        if (grade && grade->optics.on) {   // the meter and everything behind it read mean' and count'
            const auto o = ptc::optics_args(grade->optics, image, optics_out);
            PT_HIP_TRY(pt::launch_optics(o, stream));
            image.rgb = optics_out.rgb; image.count = optics_out.count; image.divide = false;
        }
        if (grade) PT_HIP_TRY(hipMemsetAsync(hist, 0, kGradeBytes, stream));
        if (grade && grade->setup.automatic) {
            const auto m = ptc::meter_args(image, hist);
            PT_HIP_TRY(pt::launch_meter(m, stream));
            PT_HIP_TRY(pt::launch_exposure(hist, grade->setup.rule, grade->has_prev, grade->e_prev, exposure, stream));
        } else if (grade) {
            uint32_t bits;
            std::memcpy(&bits, &grade->setup.exposure, sizeof bits);
            PT_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&exposure->exposure), static_cast<int>(bits), 1, stream));
        }
        if (grade && grade->bloom.on) {   // m + A * weight, a plane of means, with the count as it is
            const auto b = ptc::bloom_args(grade->bloom, image, &exposure->exposure, bloom);
            PT_HIP_TRY(pt::launch_bloom(b, stream));
            image.rgb = bloom.out_rgb; image.divide = false;
        }
        if (grade && grade->local.on) {   // ... and then m * g of that plane, or of the image so far
            const auto l = ptc::local_args(grade->local, image, &exposure->exposure, local);
            PT_HIP_TRY(pt::launch_local(l, stream));
            image.rgb = local.out_rgb; image.divide = false;
        }
        if (grade && grade->sharpen.on) {   // ... and then m * g of that: where it lies if a stage above wrote it, else into the stage's own plane
            float *out = grade->sharpen_own_mean() ? sharpen.out_rgb : const_cast<float *>(image.rgb);
            const auto s = ptc::sharpen_args(grade->sharpen, image, &exposure->exposure, sharpen, out);
            PT_HIP_TRY(pt::launch_sharpen(s, stream));
            image.rgb = out; image.divide = false;
        }
        if (lin && lin->on) {   // (without a grade nothing wrote an exposure, and `exposed` was refused)
            const auto e = ptc::linear_args(*lin, image, grade ? &exposure->exposure : nullptr, linear.out);
            PT_HIP_TRY(pt::launch_linear_encode(e, stream));
        }
        if (!want_bgr) return PT_OK;
        pt::DisplayArgs a;
        a.n = static_cast<int>(n);
        a.divide = image.divide ? 1 : 0;
        a.rgb = image.rgb; a.count = image.count;
        a.table = table;
        a.last = host->thresholds.empty() ? 0.0f : host->thresholds.back();   // (no level at all: everything is the host's)
        a.n_bands = static_cast<int>(host->band_lo.size());
        a.band_lo = band_lo; a.band_hi = band_hi;
        a.bgr = bgr; a.deferred = deferred; a.n_deferred = n_deferred;
        if (!grade) PT_HIP_TRY(pt::launch_display(a, stream));
        else if (grade->grain.on) {   // (the colour step of a request without one is the identity and no LUT)
            pt::ColourStep step = grade->colour.step;
            step.lut = step.lut_n ? d_lut.at<pt::LutVertex>(0) : nullptr;
            pt::GrainStep grain = grade->grain.step;
            grain.width = image.width;
            PT_HIP_TRY(pt::launch_display_grain(a, grade->setup.curve, &exposure->exposure, step, grain, stream));
        } else if (!grade->colour.on) PT_HIP_TRY(pt::launch_display_graded(a, grade->setup.curve, &exposure->exposure, stream));
        else {   // (use_lut has brought the LUT of this request to the device)
            pt::ColourStep step = grade->colour.step;
            step.lut = step.lut_n ? d_lut.at<pt::LutVertex>(0) : nullptr;
            PT_HIP_TRY(pt::launch_display_colour(a, grade->setup.curve, &exposure->exposure, step, stream));
        }
        return PT_OK;
    }
    // The kernel has finished: 3 bytes per pixel and the deferred list come to the host, which finishes the list's pixels.
    // `out` NULL: no display kernel ran.  With `lin` on, the encoded body comes to `linear_out` as it stands.
    int collect(float gamma, uint8_t *out, const GradeRequest *grade, Presented &got, const ptc::LinearSetup *lin = nullptr, uint8_t *linear_out = nullptr) {
        if (lin && lin->on) PT_HIP_TRY(hipMemcpy(linear_out, linear.out, (lin->format == pt::kLinearPfm ? 12 : 4) * n, hipMemcpyDeviceToHost));
        if (out) PT_HIP_TRY(hipMemcpy(out, bgr, 3 * n, hipMemcpyDeviceToHost));
        if (grade) {
            pt::ExposureOut o;
            PT_HIP_TRY(hipMemcpy(&o, exposure, sizeof o, hipMemcpyDeviceToHost));
            got.used.exposure = o.exposure;
            got.used.target = grade->setup.automatic ? o.target : o.exposure;
            got.used.metered = o.metered; got.used.dark = o.dark;
        }
        if (!out) return PT_OK;
        uint32_t len = 0;
        PT_HIP_TRY(hipMemcpy(&len, n_deferred, 4, hipMemcpyDeviceToHost));
        if (len > n) return fail(PT_ERR_HIP, "display: the deferred list is longer than the image");
        if (len) {
            std::vector<pt::DisplayDeferred> list(len);
            PT_HIP_TRY(hipMemcpy(list.data(), deferred, sizeof(pt::DisplayDeferred) * len, hipMemcpyDeviceToHost));
            for (const pt::DisplayDeferred &d : list)
                if (d.pixel < 0 || static_cast<size_t>(d.pixel) >= n) return fail(PT_ERR_HIP, "display: a deferred pixel lies outside the image");
            finish_on_host(list, gamma, *host, grade, got.used.exposure, out);
        }
        got.n_deferred = static_cast<int32_t>(len);
        return PT_OK;
    }
    void fill(pt_display_info *info, float ms, const Presented &got) const {
        if (!info) return;
        info->kernel_ms = ms;
        info->deferred_pixels = got.n_deferred;
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
    ptc::FeaturePlanes features;
    ptc::DenoisePlanes denoise;
    // a scaled present: the output image's features, mean and count, the low mean and the upsampler's records, and the output's
    // bytes and deferred list -- allocated by the first scaled present, again when the scale changes
    int32_t up_scale = 0;
    ptc::DeviceBuffer d_up;
    DisplayDevice dev_up;
    ptc::FeaturePlanes up_features;
    ptc::MeanPlanes up_out;
    ptc::UpsamplePlanes up_work;
    ptc::DeviceTimer timer;
    bool has_exposure = false;       // the e of the last metered present (pt_display_present_graded), until a reset
    float exposure = 0.0f;
    ~pt_display() {
        (void)hipSetDevice(scene->device);
        pt_temporal_destroy(history);
    }
};

namespace {

int display_create_impl(pt_scene *scene, int32_t width, int32_t height, float eps, std::unique_ptr<pt_display> &d) {
    int rc = ptc::check_image_size(width, height);
    if (rc != PT_OK) return rc;
    if (std::isnan(eps)) return fail(PT_ERR_INVALID_ARGUMENT, "eps is not a number");
    if ((rc = ptc::check_has_device(scene, "; there is no CPU fallback")) != PT_OK) return rc;
    PT_HIP_TRY(hipSetDevice(scene->device));
    d.reset(new pt_display);
    d->scene = scene; d->width = width; d->height = height; d->eps = eps;
    d->n = static_cast<size_t>(width) * height;
    if ((rc = d->dev.alloc(d->n, "pt_display_create")) != PT_OK) return rc;
    return d->timer.create("pt_display_create");
}

// What a filtered present without a temporal stage needs on the device (the caller holds d->mutex and has made the device current).
int ensure_filter(pt_display *d) {
    if (d->d_filter) return PT_OK;
    ptc::PlaneLayout l;
    d->features = ptc::FeaturePlanes::in(l, d->n);
    d->denoise = ptc::DenoisePlanes::in(l, d->n);
    const int rc = d->d_filter.alloc(l, "pt_display_present");
    if (rc != PT_OK) return rc;
    d->features.bind(d->d_filter); d->denoise.bind(d->d_filter);
    return PT_OK;
}

// What a scaled present needs on the device for scale s (the caller holds d->mutex and has made the device current).
int ensure_scaled(pt_display *d, int32_t s) {
    if (d->up_scale == s) return PT_OK;
    d->up_scale = 0;
    const size_t n_lo = d->n, n = n_lo * static_cast<size_t>(s) * s;
    ptc::PlaneLayout l;
    d->up_features = ptc::FeaturePlanes::in(l, n);
    d->up_out = ptc::MeanPlanes::in(l, n);
    d->up_work = ptc::UpsamplePlanes::in(l, n_lo, true);
    int rc;
    if ((rc = d->d_up.alloc(l, "pt_display_present_scaled")) != PT_OK || (rc = d->dev_up.alloc(n, "pt_display_present_scaled")) != PT_OK) return rc;
    d->dev_up.host.reset();   // (a new allocation holds no table yet)
    d->up_features.bind(d->d_up); d->up_out.bind(d->d_up); d->up_work.bind(d->d_up);
    d->up_scale = s;
    return PT_OK;
}

// The first hits of the whole view through the scene's camera at width x height, on `stream`.  The caller holds
// scene->launch_mutex, and keeps it for whatever else its launches need of the scene.
int enqueue_view_first_hits(pt_scene *scene, float eps, int32_t width, int32_t height, const ptc::FeaturePlanes &out, hipStream_t stream) {
    pt::RenderArgs ra;
    const int rc = ptc::scene_trace_args(scene, eps, ra);
    if (rc != PT_OK) return rc;
    return ptc::enqueue_first_hits(scene, ra, ptc::view_camera(scene), width, height, 0, height, out, stream);
}

int null_argument() { return fail(PT_ERR_INVALID_ARGUMENT, "null handle, params or image"); }

// What one present is asked for.  A NULL stage is off: the entry point that requires one has refused its absence already.
struct PresentRequest {
    const pt_display_params *display = nullptr;
    const pt_upsample_params *upsample = nullptr;   // the same chain at the display's size, then the upsample to scale times it
    const pt_grade_params *grade = nullptr;         // the exposure and the graded kernel in place of the display kernel
    pt_grade_info *grade_info = nullptr;            // with grade only; may be NULL
    const pt_bloom_params *bloom = nullptr;         // with grade only, and so are the stages below
    const pt_local_params *local = nullptr;
    const pt_colour_params *colour = nullptr;
    const pt_optics_params *optics = nullptr;
    const pt_sharpen_params *sharpen = nullptr;
    const pt_grain_params *grain = nullptr;
    const pt_linear_params *linear = nullptr;       // with or without grade; its body goes to linear_out
    uint8_t *linear_out = nullptr;
};

int display_present_impl(pt_display *d, const PresentRequest &rq, uint8_t *bgr, pt_display_info *info) {
    const pt_display_params *p = rq.display;
    const pt_upsample_params *u = rq.upsample;
    if (!d || !p) return null_argument();
    const bool scaled = u != nullptr, graded = rq.grade != nullptr;
    int rc = check_gamma(p->gamma);
    if (rc != PT_OK) return rc;
    GradeRequest grade;
    if (graded && (rc = ptc::grade_params_check(rq.grade, grade.setup)) != PT_OK) return rc;
    if (rq.bloom && (rc = ptc::bloom_params_check(rq.bloom, grade.bloom)) != PT_OK) return rc;
    if (rq.local && (rc = ptc::local_params_check(rq.local, grade.local)) != PT_OK) return rc;
    if (rq.colour && (rc = ptc::colour_params_check(rq.colour, grade.colour)) != PT_OK) return rc;
    if (rq.optics && (rc = ptc::optics_params_check(rq.optics, grade.optics)) != PT_OK) return rc;
    if (rq.sharpen && (rc = ptc::sharpen_params_check(rq.sharpen, grade.sharpen)) != PT_OK) return rc;
    if (rq.grain && (rc = ptc::grain_params_check(rq.grain, grade.grain)) != PT_OK) return rc;
    ptc::LinearSetup lin;
    if (rq.linear && (rc = ptc::linear_params_check(rq.linear, lin)) != PT_OK) return rc;
    if (lin.exposed && !graded) return fail(PT_ERR_INVALID_ARGUMENT, "linear: exposed needs a grade: a chain without one has no exposure");
    if (lin.on ? !rq.linear_out : !bgr) return null_argument();   // (bgr may be NULL where there is a linear body to make)
    pt::UpsampleArgs ua;
    if (scaled) {
        if (u->scale < pt::kUpsampleMinScale || u->scale > pt::kUpsampleMaxScale) return fail(PT_ERR_INVALID_ARGUMENT, "upsample: scale must be 2, 3 or 4");
        if ((rc = ptc::upsample_params_to_args(u, d->width * u->scale, d->height * u->scale, ua)) != PT_OK) return rc;
    }
    pt::DenoiseArgs da;
    if ((rc = ptc::denoise_params_to_args(&p->denoise, da)) != PT_OK) return rc;
    const bool temporal = p->temporal != 0, filter = da.levels > 0;
    grade.grain.step.width = scaled ? ua.width : d->width;   // (of the image the bytes are made of)
    std::lock_guard<std::mutex> present_lock(d->mutex);
    grade.has_prev = d->has_exposure; grade.e_prev = d->exposure;
    const std::shared_ptr<const DisplayTable> table = display_table(p->gamma);
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
    if (temporal && scene->has_projection)   // (the reprojection inverts a pinhole: pt_hip.h, pt_projection)
        return fail(PT_ERR_UNSUPPORTED, "temporal: the scene handle has a non-perspective projection, which the reprojection does not invert");
    PT_HIP_TRY(hipSetDevice(scene->device));
    DisplayDevice &dev = scaled ? d->dev_up : d->dev;
    if (scaled && (rc = ensure_scaled(d, ua.scale)) != PT_OK) return rc;
    if ((rc = dev.use_table(table, "pt_display_present")) != PT_OK) return rc;
    if (grade.bloom.on && (rc = dev.ensure_bloom(scaled ? ua.width : d->width, scaled ? ua.height : d->height, "pt_display_present_bloom")) != PT_OK) return rc;
    if (grade.local.on && (rc = dev.ensure_local("pt_display_present_local")) != PT_OK) return rc;
    if (grade.colour.lut && (rc = dev.use_lut(grade.colour.lut, "pt_display_present_colour")) != PT_OK) return rc;
    if (grade.optics.on && (rc = dev.ensure_optics("pt_display_present_optics")) != PT_OK) return rc;
    if (grade.sharpen.on && (rc = dev.ensure_sharpen(grade.sharpen_own_mean(), "pt_display_present_sharpen")) != PT_OK) return rc;
    if (lin.on && (rc = dev.ensure_linear("pt_display_present_linear")) != PT_OK) return rc;
    if (temporal && !d->history && (rc = pt_temporal_create(scene, d->width, d->height, d->eps, &d->history)) != PT_OK) return rc;
    if (filter && !temporal && (rc = ensure_filter(d)) != PT_OK) return rc;
    {   // the chain, behind every slice enqueued so far: no host synchronisation until its last kernel is in the queue
        std::unique_lock<std::mutex> ctx_lock;
        if (d->session) ctx_lock = std::unique_lock<std::mutex>(d->session->ctx.mutex);
        PT_HIP_TRY(d->timer.begin(stream));
        ptc::Image image = {planes.sum, planes.count, true, d->width, d->height};
        if (temporal) {
            ptc::TemporalPlanes merged;
            if ((rc = ptc::temporal_enqueue(d->history, planes, &p->temporal_params, filter ? &p->denoise : nullptr, stream, &merged)) != PT_OK) return rc;
            if (filter) image.rgb = merged.mean, image.count = merged.mean_count, image.divide = false;
            else image.rgb = merged.merged.sum, image.count = merged.merged.count;
        } else if (filter) {
            std::lock_guard<std::mutex> launch_lock(scene->launch_mutex);
            if ((rc = enqueue_view_first_hits(scene, d->eps, d->width, d->height, d->features, stream)) != PT_OK) return rc;
            da.width = d->width; da.height = d->height;
            ptc::bind_planes(da, planes, d->features, d->denoise);
            PT_HIP_TRY(pt::launch_denoise(da, stream));
            image.rgb = d->denoise.out.rgb; image.count = d->denoise.out.count; image.divide = false;
        }
        if (scaled) {
            // the low mean (levels = 0: sum / n of the accumulators as they are, or merged), the output image's features from the
            // same camera, the upsample; the bytes are then made from its mean and count
            if (image.divide) {
                PT_HIP_TRY(pt::launch_upsample_mean(image.rgb, image.count, static_cast<int>(d->n), d->up_work.mean_lo, stream));
                image.rgb = d->up_work.mean_lo;
            }
            {
                std::lock_guard<std::mutex> launch_lock(scene->launch_mutex);
                if ((rc = enqueue_view_first_hits(scene, d->eps, ua.width, ua.height, d->up_features, stream)) != PT_OK) return rc;
            }
            ptc::bind_planes(ua, image.rgb, image.count, d->up_features, d->up_work, d->up_out);
            PT_HIP_TRY(pt::launch_upsample(ua, stream));
            image = {d->up_out.rgb, d->up_out.count, false, ua.width, ua.height};
        }
        if ((rc = dev.enqueue(image, stream, graded ? &grade : nullptr, &lin, bgr != nullptr)) != PT_OK) return rc;
        PT_HIP_TRY(d->timer.end(stream));
    }
    // (an error return from here on leaves the history and the metered exposure as they were: they were only read)
    float ms = 0.0f;
    PT_HIP_TRY(d->timer.wait_ms(&ms));
    Presented got;
    if ((rc = dev.collect(p->gamma, bgr, graded ? &grade : nullptr, got, &lin, rq.linear_out)) != PT_OK) return rc;
    if (temporal) ptc::temporal_commit(d->history);
    if (graded && grade.setup.automatic) {
        d->has_exposure = true;
        d->exposure = got.used.exposure;
    }
    if (graded && rq.grade_info) *rq.grade_info = got.used;
    dev.fill(info, ms, got);
    return PT_OK;
}

// An entry point's present: `complete` is its own condition, that no stage its signature requires is NULL.
int present(pt_display *d, bool complete, const PresentRequest &rq, uint8_t *bgr, pt_display_info *info) {
    return guarded([&] { return complete ? display_present_impl(d, rq, bgr, info) : null_argument(); });
}

// A mean image in host memory, and how it is to be graded (pt_display_bytes_graded_host).
struct HostImage { int device; int32_t width, height; const float *mean_rgb; const int32_t *count; };
struct HostGrade {   // (info, colour, grain may be NULL)
    const pt_grade_params *params; bool has_prev; float e_prev; pt_grade_info *info; const pt_colour_params *colour; const pt_grain_params *grain;
};

// `g` = NULL: pt_display_bytes_host.
int display_bytes_host_impl(const HostImage &image, float gamma, const HostGrade *g, uint8_t *bgr, pt_display_info *info) {
    if (image.width <= 0 || image.height <= 0 || !image.mean_rgb || !image.count || !bgr || (g && !g->params))
        return fail(PT_ERR_INVALID_ARGUMENT, "null buffer or empty image");
    int rc = ptc::check_image_size(image.width, image.height);
    if (rc != PT_OK || (rc = check_gamma(gamma)) != PT_OK) return rc;
    GradeRequest grade;
    if (g && (rc = ptc::grade_params_check(g->params, grade.setup)) != PT_OK) return rc;
    if (g) grade.has_prev = g->has_prev, grade.e_prev = g->e_prev;
    if (g && g->colour && (rc = ptc::colour_params_check(g->colour, grade.colour)) != PT_OK) return rc;
    if (g && g->grain && (rc = ptc::grain_params_check(g->grain, grade.grain)) != PT_OK) return rc;
    grade.grain.step.width = image.width;
    if ((rc = ptc::use_device(image.device, "display")) != PT_OK) return rc;
    const size_t n = static_cast<size_t>(image.width) * image.height;
    const std::shared_ptr<const DisplayTable> table = display_table(gamma);
    DisplayDevice dev;
    ptc::PlaneLayout l;
    ptc::MeanPlanes in = ptc::MeanPlanes::in(l, n);
    ptc::DeviceBuffer d_in;
    if ((rc = d_in.alloc(l, "pt_display_bytes_host")) != PT_OK || (rc = dev.alloc(n, "pt_display_bytes_host")) != PT_OK ||
        (rc = dev.use_table(table, "pt_display_bytes_host")) != PT_OK)
        return rc;
    if (grade.colour.lut && (rc = dev.use_lut(grade.colour.lut, "pt_display_bytes_colour_host")) != PT_OK) return rc;
    in.bind(d_in);
    if ((rc = in.upload(image.mean_rgb, image.count)) != PT_OK) return rc;
    float ms = 0.0f;
    rc = ptc::timed(nullptr, "pt_display_bytes_host", &ms, [&] { return dev.enqueue({in.rgb, in.count, false, image.width, image.height}, nullptr, g ? &grade : nullptr); });
    if (rc != PT_OK) return rc;
    Presented got;
    if ((rc = dev.collect(gamma, bgr, g ? &grade : nullptr, got)) != PT_OK) return rc;
    if (g && g->info) *g->info = got.used;
    dev.fill(info, ms, got);
    return PT_OK;
}

// The encode kernel alone on a host image (pt_linear_encode_device_host).
int linear_encode_device_host_impl(const HostImage &image, float exposure, const pt_linear_params *lin, uint8_t *out, pt_display_info *info) {
    ptc::LinearSetup setup;
    int rc = ptc::linear_image_check(image.width, image.height, image.mean_rgb, image.count, exposure, lin, out, setup);
    if (rc != PT_OK || (rc = ptc::use_device(image.device, "linear")) != PT_OK) return rc;
    const size_t n = static_cast<size_t>(image.width) * image.height;
    ptc::PlaneLayout l;
    ptc::MeanPlanes in = ptc::MeanPlanes::in(l, n);
    LinearPlane body = LinearPlane::in(l, n);
    const size_t o_e = l.add(4);
    ptc::DeviceBuffer d_in;
    if ((rc = d_in.alloc(l, "pt_linear_encode_device_host")) != PT_OK) return rc;
    in.bind(d_in); body.bind(d_in);
    float *e = d_in.at<float>(o_e);
    if ((rc = in.upload(image.mean_rgb, image.count)) != PT_OK) return rc;
    PT_HIP_TRY(hipMemcpy(e, &exposure, 4, hipMemcpyHostToDevice));
    float ms = 0.0f;
    rc = ptc::timed(nullptr, "pt_linear_encode_device_host", &ms, [&] {
        const auto a = ptc::linear_args(setup, {in.rgb, in.count, false, image.width, image.height}, e, body.out);
        PT_HIP_TRY(pt::launch_linear_encode(a, nullptr));
        return static_cast<int>(PT_OK);
    });
    if (rc != PT_OK) return rc;
    PT_HIP_TRY(hipMemcpy(out, body.out, pt_linear_bytes(image.width, image.height, setup.format), hipMemcpyDeviceToHost));
    if (info) {
        *info = pt_display_info{};
        info->kernel_ms = ms;   // (no pixel is deferred, and the kernel searches no table)
    }
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
    PresentRequest rq;
    rq.display = p;
    return present(d, true, rq, bgr, info);
}

int pt_display_present_scaled(pt_display *d, const pt_display_params *p, const pt_upsample_params *u, uint8_t *bgr, pt_display_info *info) {
    PresentRequest rq;
    rq.display = p; rq.upsample = u;
    return present(d, u != nullptr, rq, bgr, info);
}

int pt_display_present_graded(pt_display *d, const pt_display_params *p, const pt_upsample_params *u, const pt_grade_params *g, uint8_t *bgr,
                              pt_display_info *info, pt_grade_info *grade_info) {
    PresentRequest rq;
    rq.display = p; rq.upsample = u; rq.grade = g; rq.grade_info = grade_info;
    return present(d, g != nullptr, rq, bgr, info);
}

int pt_display_present_bloom(pt_display *d, const pt_display_params *p, const pt_upsample_params *u, const pt_grade_params *g,
                             const pt_bloom_params *b, uint8_t *bgr, pt_display_info *info, pt_grade_info *grade_info) {
    PresentRequest rq;
    rq.display = p; rq.upsample = u; rq.grade = g; rq.grade_info = grade_info; rq.bloom = b;
    return present(d, g && b, rq, bgr, info);
}

int pt_display_present_local(pt_display *d, const pt_display_params *p, const pt_upsample_params *u, const pt_grade_params *g,
                             const pt_bloom_params *b, const pt_local_params *l, uint8_t *bgr, pt_display_info *info, pt_grade_info *grade_info) {
    PresentRequest rq;
    rq.display = p; rq.upsample = u; rq.grade = g; rq.grade_info = grade_info; rq.bloom = b; rq.local = l;
    return present(d, g && b && l, rq, bgr, info);
}

int pt_display_present_colour(pt_display *d, const pt_display_params *p, const pt_upsample_params *u, const pt_grade_params *g,
                              const pt_bloom_params *b, const pt_local_params *l, const pt_colour_params *c, uint8_t *bgr, pt_display_info *info,
                              pt_grade_info *grade_info) {
    PresentRequest rq;
    rq.display = p; rq.upsample = u; rq.grade = g; rq.grade_info = grade_info; rq.bloom = b; rq.local = l; rq.colour = c;
    return present(d, g && b && l && c, rq, bgr, info);
}

int pt_display_present_optics(pt_display *d, const pt_display_params *p, const pt_upsample_params *u, const pt_grade_params *g,
                              const pt_bloom_params *b, const pt_local_params *l, const pt_colour_params *c, const pt_optics_params *o,
                              uint8_t *bgr, pt_display_info *info, pt_grade_info *grade_info) {
    PresentRequest rq;
    rq.display = p; rq.upsample = u; rq.grade = g; rq.grade_info = grade_info; rq.bloom = b; rq.local = l; rq.colour = c; rq.optics = o;
    return present(d, g && b && l && c && o, rq, bgr, info);
}

int pt_display_present_sharpen(pt_display *d, const pt_display_params *p, const pt_upsample_params *u, const pt_grade_params *g,
                               const pt_bloom_params *b, const pt_local_params *l, const pt_colour_params *c, const pt_optics_params *o,
                               const pt_sharpen_params *s, uint8_t *bgr, pt_display_info *info, pt_grade_info *grade_info) {
    PresentRequest rq;
    rq.display = p; rq.upsample = u; rq.grade = g; rq.grade_info = grade_info; rq.bloom = b; rq.local = l; rq.colour = c; rq.optics = o;
    rq.sharpen = s;
    return present(d, g && b && l && c && o && s, rq, bgr, info);
}

int pt_display_present_grain(pt_display *d, const pt_display_params *p, const pt_upsample_params *u, const pt_grade_params *g,
                             const pt_bloom_params *b, const pt_local_params *l, const pt_colour_params *c, const pt_optics_params *o,
                             const pt_sharpen_params *s, const pt_grain_params *n, uint8_t *bgr, pt_display_info *info, pt_grade_info *grade_info) {
    PresentRequest rq;
    rq.display = p; rq.upsample = u; rq.grade = g; rq.grade_info = grade_info; rq.bloom = b; rq.local = l; rq.colour = c; rq.optics = o;
    rq.sharpen = s; rq.grain = n;
    return present(d, g && b && l && c && o && s && n, rq, bgr, info);
}

int pt_display_present_linear(pt_display *d, const pt_display_params *p, const pt_upsample_params *u, const pt_grade_params *g,
                              const pt_bloom_params *b, const pt_local_params *l, const pt_colour_params *c, const pt_optics_params *o,
                              const pt_sharpen_params *s, const pt_grain_params *n, const pt_linear_params *lin, uint8_t *bgr, uint8_t *linear,
                              pt_display_info *info, pt_grade_info *grade_info) {
    PresentRequest rq;
    rq.display = p; rq.upsample = u; rq.grade = g; rq.grade_info = grade_info; rq.bloom = b; rq.local = l; rq.colour = c; rq.optics = o;
    rq.sharpen = s; rq.grain = n; rq.linear = lin; rq.linear_out = linear;
    // every stage of the graded chain, or -- a chain with no grade at all -- none of them
    const bool complete = lin && (g ? b && l && c && o && s && n : !b && !l && !c && !o && !s && !n);
    return present(d, complete, rq, bgr, info);
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
    return guarded([&] { return display_bytes_host_impl({device, width, height, mean_rgb, count}, gamma, nullptr, bgr, info); });
}

int pt_display_bytes_graded_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float gamma,
                                 const pt_grade_params *g, int32_t has_prev, float e_prev, uint8_t *bgr, pt_display_info *info,
                                 pt_grade_info *grade_info) {
    return guarded([&] {
        const HostGrade grade = {g, has_prev != 0, e_prev, grade_info, nullptr, nullptr};
        return display_bytes_host_impl({device, width, height, mean_rgb, count}, gamma, &grade, bgr, info);
    });
}

int pt_display_bytes_colour_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float gamma,
                                 const pt_grade_params *g, const pt_colour_params *c, int32_t has_prev, float e_prev, uint8_t *bgr,
                                 pt_display_info *info, pt_grade_info *grade_info) {
    return guarded([&] {
        if (!c) return null_argument();
        const HostGrade grade = {g, has_prev != 0, e_prev, grade_info, c, nullptr};
        return display_bytes_host_impl({device, width, height, mean_rgb, count}, gamma, &grade, bgr, info);
    });
}

int pt_display_bytes_grain_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float gamma,
                                const pt_grade_params *g, const pt_colour_params *c, const pt_grain_params *n, int32_t has_prev, float e_prev,
                                uint8_t *bgr, pt_display_info *info, pt_grade_info *grade_info) {
    return guarded([&] {
        if (!c || !n) return null_argument();
        const HostGrade grade = {g, has_prev != 0, e_prev, grade_info, c, n};
        return display_bytes_host_impl({device, width, height, mean_rgb, count}, gamma, &grade, bgr, info);
    });
}

int pt_linear_encode_device_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure,
                                 const pt_linear_params *lin, uint8_t *out, pt_display_info *info) {
    return guarded([&] { return linear_encode_device_host_impl({device, width, height, mean_rgb, count}, exposure, lin, out, info); });
}

int pt_display_table(float gamma, int32_t *levels, float *thresholds, float *doubt_lo, float *doubt_hi) {
    return guarded([&] { return display_table_impl(gamma, levels, thresholds, doubt_lo, doubt_hi); });
}

}  // extern "C"
