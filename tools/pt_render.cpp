// pt_render -- command-line front end with the reference's flag set (config.h:35-99) on top of libpt_hip.so.
//
// It plays the part of the reference's main() (main.cpp:87-215): parse flags, load the model, run the passes, write
// previews every `-UPDATE` passes, stop at the `-TL` time limit, print the per-pass progress lines, then resolve,
// and write "<date>  <ms>   <n> of <rpp>  max_disp .. min_disp .. aver_disp ...bmp" plus "../result.bmp".
// The passes themselves run on the GPU through the C ABI; nothing here computes radiance.
//
// The accumulators stay on the device for the whole frame (pt_session): they cross PCIe only when a preview or the final
// image needs them.  With -TL the pass slices are kept to about 75 ms (from the measured time per pass, never less than
// one pass), so the time limit is checked at the reference's granularity -- before a pass starts (main.cpp:111-114) --
// whatever -UPDATE is.
//
// Several GPUs: the reference splits the image's rows over its OpenMP threads inside the pass loop (main.cpp:115,132,141);
// `-GPUS N` splits them over the first N devices of the node (or `-DEVICES 0,2,5`) through pt_frame_*: N row bands, every
// pass slice enqueued on all devices before anything waits, the bands' accumulators gathered to the first device by one RCCL
// group of sends / receives, then the unmodified resolve.  The image is bit-identical for any N.  On a box with fewer
// devices `-REHEARSE 1` runs the N-band code path anyway, several bands per device, with device-to-device copies in place of
// the collective -- and says so on stderr; without it such a request is refused.
//
// Extra flags (not in the reference): -OUT <file> writes only that file instead of the two reference outputs,
// -DEVICE <n> selects the HIP device (one GPU), -GPUS / -DEVICES / -REHEARSE as above, -QUIET 1 drops the per-pass lines,
// -TIMING 1 prints one JSON line with the seconds spent in each phase (HIP start-up, load, render, read-back, resolve, BMP
// write) on stderr, -BENCH_STEPS k [-BENCH_WARMUP w] times k whole frames (clear, all passes on all devices, gather, wait)
// after w untimed ones and prints one JSON line on stdout instead of writing an image, -SELFCOLL 1 (test aid, one GPU)
// routes the band through an RCCL send / receive to self, -FASTEXIT 1 leaves with _Exit once the files are written (skips the
// runtime's teardown).
// A camera (pt_camera_look_at, not in the reference): -EYE x,y,z (default 0,0,-20), -LOOKAT x,y,z (default 0,0,0), -UP x,y,z
// (default 0,1,0), -FOV <vertical degrees> (default 53.13010235415598 = 2 atan(0.5)), -ASPECT <width / height> (default 0: both image
// axes span -FOV, the reference's mapping).  Without any of them no camera is set and the reference's view is rendered as before;
// with the defaults spelled out the camera is the reference's and the image is the same.  PT_RENDER_PRINT_CAMERA=1 prints the
// camera the flags resolve to ("camera none" without one) and exits.
// A thin lens (pt_scene_set_lens, not in the reference): -APERTURE <radius> (default 0: no lens, a pinhole), -FOCUS <distance of
// the focal plane> (default |LOOKAT - EYE|, 20 for the reference's camera).  PT_RENDER_PRINT_CAMERA=1 then also prints
// "lens <radius> <focus distance>".
// The denoiser (pt_denoise_host, not in the reference): -DENOISE <levels> (default 0: off; 5 is the usual choice) filters the final
// image's linear mean with the feature-guided a-trous filter before the tone map, -DN_SIGMA_L / -DN_SIGMA_P set its luminance and
// plane-distance widths (default 0: the library's).  The order is resolve (so the dispersion numbers and the file name are those
// of the undenoised frame) -> feature buffers -> denoise -> tone map -> -GAUSS / -MEDIAN -> quantize -> BMP, on the first device
// of the frame.  Previews (-UPDATE) stay undenoised.  Without the flag nothing changes.
// A sequence (pt_temporal_*, not in the reference): -FRAMES n (default 1) renders n frames, frame i with passes [i RPP, (i + 1) RPP)
// of the same seed, and writes each as frame_%04d.bmp in the working directory; the last frame also takes the usual outputs (the
// named file and ../result.bmp, or -OUT).  -EYE_END x,y,z and -LOOKAT_END x,y,z (default: -EYE and -LOOKAT) move the camera: frame
// i looks from start + (end - start) i / (n - 1), computed in double, through pt_camera_look_at.  -TEMPORAL m (default 0: off)
// merges every frame with the reprojected history of the earlier ones before it is resolved, m being the cap of the history's age
// in frames (32 is the usual choice); with -DENOISE the filter then runs on the merged frame, in the same chain on the device.
// A sequence writes no previews and prints no -TIMING line, and -TL with -FRAMES > 1 is refused.  Without -FRAMES and -TEMPORAL
// nothing changes.
// The device-resident display path (pt_display_*, not in the reference): -DEVICE_RESOLVE 1 (default 0) makes the images' bytes on
// the first device of the frame, where the accumulators lie -- temporal merge, denoiser, tone map and quantization in one chain,
// 3 bytes per pixel to the host -- instead of reading 28 bytes per pixel back and tone-mapping on the host.  The files are
// byte-identical with and without it.  In a sequence only the last frame is also read back, for the dispersion figures in the
// output name.  -GAUSS / -MEDIAN act on the tone-mapped float image and stay on the host path: with either of them, or with a
// -GAMMA that is not a finite positive number, the flag is ignored with a message on stderr.
// Reduced-resolution rendering (pt_upsample_host, not in the reference): -RENDER_SCALE s (default 1: off; 2, 3 or 4) traces the
// frame at (W / s) x (H / s) and writes it at --W x --H: the low frame's linear mean (denoised with -DENOISE, merged with -TEMPORAL,
// all at the traced size) is reconstructed at the written size by the feature-guided upsampler from first-hit features rendered
// at the written size, then tone-mapped, filtered (-GAUSS / -MEDIAN, at the written size) and quantized.  --W and --H must be
// multiples of s: otherwise, or with s outside 1 .. 4, a message goes to stderr and the exit status is 1.  The dispersion numbers
// in the file name are those of the low-resolution accumulators; previews (-UPDATE) show the traced frame at its own size.  With
// -DEVICE_RESOLVE 1 the chain runs on the device (pt_display_present_scaled); the files are byte-identical either way.  With
// -RENDER_SCALE 1 nothing changes.
// Display grading (pt_grade_host, pt_display_present_graded, not in the reference): -TONE reference|clamp|reinhard|aces (default
// reference: the reference's wrapping conversion) applies a tone curve and -EXPOSURE <stops> (default 0) an exposure e = 2^stops to
// the linear mean before the tone map; -AUTO_EXPOSURE 1 meters e from the image instead (a luminance histogram on the device),
// with -KEY <the luminance the percentile is brought to, default 0.18>, -PERCENTILE <1 .. 100, default 50> and -ADAPT <rate, default
// 1: no smoothing> -- in a sequence frame i starts from frame i - 1's exposure.  The order is ... -> linear mean -> meter -> grade ->
// tone map -> -GAUSS / -MEDIAN -> quantize; previews (-UPDATE) stay ungraded.  It works on the host path and with
// -DEVICE_RESOLVE 1, with byte-identical files, and with -RENDER_SCALE, -DENOISE, -TEMPORAL and -FRAMES.  Without any of these
// flags nothing changes.
// Bloom (pt_bloom_host, pt_display_present_bloom, not in the reference): -BLOOM <strength, default 0: off> spreads the light above
// -BLOOM_THRESHOLD <luminance after exposure, default 1> over its neighbourhood with a pyramid of -BLOOM_LEVELS <1 .. 8, default 5>
// levels, on the linear mean at the written size: ... -> linear mean -> meter -> bloom -> grade -> tone map -> -GAUSS / -MEDIAN ->
// quantize (without -TONE / -EXPOSURE / -AUTO_EXPOSURE the grade is the reference's: no curve, e = 1); previews stay unbloomed.
// It works on the host path and with -DEVICE_RESOLVE 1, with byte-identical files, and with every flag grading works with.
// Without -BLOOM, or with -BLOOM 0, nothing changes.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <iostream>
#include <string>
#include <vector>

#include "pt_hip.h"

namespace {

struct Options {   // defaults: config.h:16-29
    int height = 512, width = 512, rays_per_pixel = 20, max_ray_reflections = 8, median = 0, gauss = 0;
    float eps = 1e-4f, error = 0.001f;
    int update = 32;
    float gamma_correction = 1 / 2.2f;
    std::string model_path = "../models/", model_name = "Tor.obj", skybox;
    int seed = 42, time_limit = 0;
    std::string out;
    int device = 0, quiet = 0, timing = 0;
    int gpus = 0, rehearse = 0, selfcoll = 0, bench_steps = 0, bench_warmup = 1, fast_exit = 0;
    std::string devices;
    long long t0_ns = 0;   // -T0_NS: CLOCK_REALTIME of the parent just before it started this process (bench.py), for the start-up phase
    bool camera = false;   // any of -EYE / -LOOKAT / -UP / -FOV / -ASPECT given
    std::string eye = "0,0,-20", lookat = "0,0,0", up = "0,1,0";
    float fov = 53.13010235415598f, aspect = 0.0f;
    std::string aperture, focus;   // -APERTURE / -FOCUS as given
    bool aperture_given = false, focus_given = false;
    int denoise = 0;               // -DENOISE: a-trous levels, 0 = off
    float dn_sigma_l = 0.0f, dn_sigma_p = 0.0f;
    int frames = 1;                // -FRAMES
    float temporal = 0.0f;         // -TEMPORAL: max_frames of the history, 0 = no temporal stage
    std::string eye_end, lookat_end;   // -EYE_END / -LOOKAT_END as given ("" = the start value)
    int device_resolve = 0;        // -DEVICE_RESOLVE: 1 = the images' bytes are made on the device (pt_display_*)
    int render_scale = 1;          // -RENDER_SCALE: the frame is traced at (W / s) x (H / s) and upsampled to W x H
    std::string tone = "reference";   // -TONE
    bool grading = false;          // any of -TONE / -EXPOSURE / -AUTO_EXPOSURE given
    float exposure_stops = 0.0f, key = 0.0f, adapt = 0.0f;   // -EXPOSURE, -KEY, -ADAPT (0 = the library's default)
    int auto_exposure = 0, percentile = 0;                   // -AUTO_EXPOSURE, -PERCENTILE
    float bloom = 0.0f, bloom_threshold = 0.0f;              // -BLOOM, -BLOOM_THRESHOLD (0 = the library's default)
    int bloom_levels = 0;                                    // -BLOOM_LEVELS
};

long long now_ms() {
    using namespace std::chrono;
    return duration_cast<milliseconds>(system_clock::now().time_since_epoch()).count();
}

void parse(int argc, char **argv, Options &o) {   // pairs `flag value` from argv[1] on, unknown flags ignored
    for (int i = 1; i < argc - 1; i += 2) {
        const std::string f = argv[i];
        const char *v = argv[i + 1];
        if (f == "--H") o.height = std::atoi(v);
        if (f == "--W") o.width = std::atoi(v);
        if (f == "-RPP") o.rays_per_pixel = std::atoi(v);
        if (f == "-MRR") o.max_ray_reflections = std::atoi(v);
        if (f == "-EPS") o.eps = static_cast<float>(std::atof(v));
        if (f == "-ERR") o.error = static_cast<float>(std::atof(v));
        if (f == "-MEDIAN") { o.median = std::atoi(v); o.gauss = 0; }
        if (f == "-UPDATE") o.update = std::atoi(v);
        if (f == "-MODEL_PATH") o.model_path = v;
        if (f == "-MODEL_NAME") o.model_name = v;
        if (f == "-GAUSS") { o.gauss = std::atoi(v); o.median = 0; }
        if (f == "-GAMMA") o.gamma_correction = static_cast<float>(std::atof(v));
        if (f == "-SKYBOX") o.skybox = v;
        if (f == "-SEED") o.seed = std::atoi(v);
        if (f == "-TL") o.time_limit = std::atoi(v);
        if (f == "-OUT") o.out = v;
        if (f == "-DEVICE") o.device = std::atoi(v);
        if (f == "-QUIET") o.quiet = std::atoi(v);
        if (f == "-TIMING") o.timing = std::atoi(v);
        if (f == "-GPUS") o.gpus = std::atoi(v);
        if (f == "-DEVICES") o.devices = v;
        if (f == "-REHEARSE") o.rehearse = std::atoi(v);
        if (f == "-SELFCOLL") o.selfcoll = std::atoi(v);
        if (f == "-BENCH_STEPS") o.bench_steps = std::atoi(v);
        if (f == "-BENCH_WARMUP") o.bench_warmup = std::atoi(v);
        if (f == "-T0_NS") o.t0_ns = std::atoll(v);
        if (f == "-FASTEXIT") o.fast_exit = std::atoi(v);
        if (f == "-EYE") { o.eye = v; o.camera = true; }
        if (f == "-LOOKAT") { o.lookat = v; o.camera = true; }
        if (f == "-UP") { o.up = v; o.camera = true; }
        if (f == "-FOV") { o.fov = static_cast<float>(std::atof(v)); o.camera = true; }
        if (f == "-ASPECT") { o.aspect = static_cast<float>(std::atof(v)); o.camera = true; }
        if (f == "-APERTURE") { o.aperture = v; o.aperture_given = true; }
        if (f == "-FOCUS") { o.focus = v; o.focus_given = true; }
        if (f == "-DENOISE") o.denoise = std::atoi(v);
        if (f == "-DN_SIGMA_L") o.dn_sigma_l = static_cast<float>(std::atof(v));
        if (f == "-DN_SIGMA_P") o.dn_sigma_p = static_cast<float>(std::atof(v));
        if (f == "-FRAMES") o.frames = std::atoi(v);
        if (f == "-TEMPORAL") o.temporal = static_cast<float>(std::atof(v));
        if (f == "-EYE_END") o.eye_end = v;
        if (f == "-LOOKAT_END") o.lookat_end = v;
        if (f == "-DEVICE_RESOLVE") o.device_resolve = std::atoi(v);
        if (f == "-RENDER_SCALE") o.render_scale = std::atoi(v);
        if (f == "-TONE") { o.tone = v; o.grading = true; }
        if (f == "-EXPOSURE") { o.exposure_stops = static_cast<float>(std::atof(v)); o.grading = true; }
        if (f == "-AUTO_EXPOSURE") { o.auto_exposure = std::atoi(v); o.grading = true; }
        if (f == "-KEY") o.key = static_cast<float>(std::atof(v));
        if (f == "-PERCENTILE") o.percentile = std::atoi(v);
        if (f == "-ADAPT") o.adapt = static_cast<float>(std::atof(v));
        if (f == "-BLOOM") o.bloom = static_cast<float>(std::atof(v));
        if (f == "-BLOOM_THRESHOLD") o.bloom_threshold = static_cast<float>(std::atof(v));
        if (f == "-BLOOM_LEVELS") o.bloom_levels = std::atoi(v);
    }
}

// "x,y,z": three finite numbers, nothing else
bool parse_vec3(const std::string &text, float out[3]) {
    const char *p = text.c_str();
    for (int k = 0; k < 3; ++k) {
        char *end = nullptr;
        out[k] = std::strtof(p, &end);
        if (end == p || !std::isfinite(out[k])) return false;
        if (*end != (k < 2 ? ',' : '\0')) return false;
        p = end + 1;
    }
    return true;
}

// one finite number, nothing else
bool parse_float(const std::string &text, float &out) {
    char *end = nullptr;
    out = std::strtof(text.c_str(), &end);
    return end != text.c_str() && *end == '\0' && std::isfinite(out);
}

int die(const char *what) {
    std::cerr << what << ": " << pt_last_error() << std::endl;
    return 1;
}

}  // namespace

int main(int argc, char **argv) {
    const long long start_time = now_ms();
    Options o;
    parse(argc, argv, o);
    if (std::getenv("PT_RENDER_PRINT_CONFIG")) {   // tests/test_ref_parts.py: the parsed Config fields, as the reference's own parser is asked for them
        const unsigned sd = o.seed < 0 ? static_cast<unsigned>(std::time(nullptr)) : static_cast<unsigned>(o.seed);
        std::printf("height %d\nwidth %d\nrays_per_pixel %d\nmax_ray_reflections %d\nmedian %d\ngauss %d\neps %.9g\nerror %.9g\nupdate %d\n"
                    "gamma_correction %.9g\nmodel_path %s\nmodel_name %s\nskybox %s\ntime_limit %d\nseed %u\n",
                    o.height, o.width, o.rays_per_pixel, o.max_ray_reflections, o.median, o.gauss, static_cast<double>(o.eps),
                    static_cast<double>(o.error), o.update, static_cast<double>(o.gamma_correction), o.model_path.c_str(),
                    o.model_name.c_str(), o.skybox.c_str(), o.time_limit, sd);
        return 0;
    }
    pt_camera camera;
    if (o.camera) {
        float eye[3], at[3], up[3];
        if (!parse_vec3(o.eye, eye) || !parse_vec3(o.lookat, at) || !parse_vec3(o.up, up)) {
            std::cerr << "pt_render: -EYE / -LOOKAT / -UP take three comma-separated numbers, x,y,z" << std::endl;
            return 2;
        }
        if (pt_camera_look_at(eye, at, up, o.fov, o.aspect, &camera) != PT_OK) return die("pt_render");
    }
    pt_lens lens{0.0f, 0.0f};
    if (o.aperture_given && !(parse_float(o.aperture, lens.radius) && lens.radius >= 0.0f)) {
        std::cerr << "pt_render: -APERTURE takes a radius >= 0" << std::endl;
        return 2;
    }
    if (o.focus_given) {
        if (!(parse_float(o.focus, lens.focus_distance) && lens.focus_distance > 0.0f)) {
            std::cerr << "pt_render: -FOCUS takes a distance > 0" << std::endl;
            return 2;
        }
    } else {   // the distance from the eye to the point looked at: 20 for the reference's camera
        float eye[3] = {0.0f, 0.0f, -20.0f}, at[3] = {0.0f, 0.0f, 0.0f};
        if (o.camera) {
            parse_vec3(o.eye, eye);
            parse_vec3(o.lookat, at);
        }
        double d2 = 0.0;
        for (int i = 0; i < 3; ++i) d2 += (static_cast<double>(at[i]) - eye[i]) * (static_cast<double>(at[i]) - eye[i]);
        lens.focus_distance = static_cast<float>(std::sqrt(d2));
    }
    const bool has_lens = lens.radius > 0.0f;
    if (std::getenv("PT_RENDER_PRINT_CAMERA")) {
        if (!o.camera) {
            std::printf("camera none\n");
        } else {
            const float *rows[4] = {camera.origin, camera.right, camera.up, camera.forward};
            const char *names[4] = {"origin", "right", "up", "forward"};
            for (int r = 0; r < 4; ++r)
                std::printf("%s %.9g %.9g %.9g\n", names[r], static_cast<double>(rows[r][0]), static_cast<double>(rows[r][1]),
                            static_cast<double>(rows[r][2]));
        }
        if (has_lens) std::printf("lens %.9g %.9g\n", static_cast<double>(lens.radius), static_cast<double>(lens.focus_distance));
        return 0;
    }
    if (o.width <= 0 || o.height <= 0) {
        std::cerr << "pt_render: --W and --H must be positive" << std::endl;
        return 2;
    }
    if (o.render_scale < 1 || o.render_scale > PT_UPSAMPLE_MAX_SCALE || o.width % o.render_scale || o.height % o.render_scale) {
        std::cerr << "pt_render: -RENDER_SCALE takes 1, 2, 3 or 4, and --W and --H must be multiples of it" << std::endl;
        return 1;
    }
    const int scale = o.render_scale;
    const int tw = o.width / scale, th = o.height / scale;   // the traced size; --W x --H is the written size
    pt_upsample_params upsample;
    std::memset(&upsample, 0, sizeof upsample);
    upsample.scale = scale; upsample.sigma_plane = o.dn_sigma_p;
    const bool sequence = o.frames > 1 || o.temporal > 0.0f;
    if (o.frames > 1 && o.time_limit != 0) {
        std::cerr << "pt_render: -TL is not defined for a sequence (-FRAMES > 1)" << std::endl;
        return 2;
    }
    if (o.frames < 1 || !(o.temporal >= 0.0f)) {
        std::cerr << "pt_render: -FRAMES takes a count >= 1 and -TEMPORAL a history length >= 0" << std::endl;
        return 2;
    }
    bool device_resolve = o.device_resolve != 0;
    if (device_resolve && (o.gauss || o.median)) {
        std::cerr << "pt_render: -DEVICE_RESOLVE is ignored with -GAUSS / -MEDIAN: they filter the tone-mapped float image, on the host path" << std::endl;
        device_resolve = false;
    }
    if (device_resolve && !(std::isfinite(o.gamma_correction) && o.gamma_correction > 0.0f)) {
        std::cerr << "pt_render: -DEVICE_RESOLVE is ignored: it needs a finite -GAMMA > 0" << std::endl;
        device_resolve = false;
    }
    // -TONE / -EXPOSURE / -AUTO_EXPOSURE: what every graded image is asked for; the library checks it (no device needed)
    // -BLOOM: a stage of the graded chain; alone it runs with the zeroed grade, whose bytes are the ungraded ones
    pt_bloom_params bloom;
    std::memset(&bloom, 0, sizeof bloom);
    bloom.strength = o.bloom; bloom.threshold = o.bloom_threshold; bloom.levels = o.bloom_levels;
    // (checked here, not by a call of the library's device entry point: nothing before the scene is parsed may start the HIP runtime)
    if (!(std::isfinite(bloom.strength) && bloom.strength >= 0.0f) || !(std::isfinite(bloom.threshold) && bloom.threshold >= 0.0f) ||
        bloom.levels < 0 || bloom.levels > PT_BLOOM_MAX_LEVELS) {
        std::cerr << "pt_render: -BLOOM and -BLOOM_THRESHOLD take a number >= 0, -BLOOM_LEVELS 1 .. " << PT_BLOOM_MAX_LEVELS << std::endl;
        return 2;
    }
    const bool blooming = bloom.strength > 0.0f;
    const bool grading = o.grading || blooming;
    pt_grade_params grade;
    std::memset(&grade, 0, sizeof grade);
    if (o.grading) {
        const char *names[4] = {"reference", "clamp", "reinhard", "aces"};
        grade.curve = -1;
        for (int k = 0; k < 4; ++k)
            if (o.tone == names[k]) grade.curve = k;
        grade.exposure = std::exp2f(o.exposure_stops);
        grade.auto_exposure = o.auto_exposure != 0;
        grade.percentile = o.percentile; grade.key = o.key; grade.rate = o.adapt;
        const uint32_t empty[PT_METER_ENTRIES] = {0};
        float e = 0, target = 0;
        if (pt_exposure_from_histogram(empty, &grade, 0, 0.0f, &e, &target) != PT_OK) {
            std::cerr << "pt_render: -TONE takes reference, clamp, reinhard or aces; -EXPOSURE stops; -KEY, -ADAPT >= 0; -PERCENTILE 1 .. 100 ("
                      << pt_last_error() << ")" << std::endl;
            return 2;
        }
    }
    const unsigned seed = o.seed < 0 ? static_cast<unsigned>(std::time(nullptr)) : static_cast<unsigned>(o.seed);   // config.h:101-104

    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    const clk::time_point t_begin = clk::now();
    double pre_main_s = 0;   // exec + dynamic linking, when the parent told us when it started us
    if (o.t0_ns > 0) {
        timespec ts;
        clock_gettime(CLOCK_REALTIME, &ts);
        pre_main_s = (static_cast<long long>(ts.tv_sec) * 1000000000LL + ts.tv_nsec - o.t0_ns) * 1e-9;
    }
    // The model is parsed before the first HIP call (host-only scene): nothing below depends on the device yet.
    pt_scene *scene = nullptr;
    if (pt_scene_load_obj(o.model_path.c_str(), o.model_name.c_str(), -1, &scene) != PT_OK) return die("pt_render");
    if (!o.skybox.empty() && pt_scene_set_skybox_bmp(scene, o.skybox.c_str()) != PT_OK) return die("pt_render");   // scene.cpp:20-22
    if (o.camera && pt_scene_set_camera(scene, &camera) != PT_OK) return die("pt_render");   // the frame's device copies inherit it
    if (has_lens && pt_scene_set_lens(scene, &lens) != PT_OK) return die("pt_render");         // and its lens
    const clk::time_point t_parse = clk::now();
    const int n_dev = pt_device_count();   // first HIP call: runtime start-up
    if (n_dev < 1) {
        std::cerr << "pt_render: no HIP device (the integrator has no CPU fallback)" << std::endl;
        return 1;
    }
    const clk::time_point t_hip = clk::now();

    // Row bands -> devices (main.cpp:115,132,141: the reference's split of the rows over its threads).
    std::vector<int32_t> devices;
    if (!o.devices.empty()) {
        for (size_t at = 0; at <= o.devices.size();) {
            const size_t comma = std::min(o.devices.find(',', at), o.devices.size());
            devices.push_back(std::atoi(o.devices.substr(at, comma - at).c_str()));
            at = comma + 1;
        }
    } else if (o.gpus > 0) {
        for (int b = 0; b < o.gpus; ++b) devices.push_back(o.rehearse ? b % n_dev : b);
    } else {
        devices.push_back(o.device);
    }
    uint32_t flags = 0;
    if (o.rehearse) flags |= PT_FRAME_REHEARSE;
    if (o.selfcoll) flags |= PT_FRAME_SELF_COLLECTIVE;
    pt_frame *frame = nullptr;
    if (pt_frame_create(scene, devices.data(), static_cast<int32_t>(devices.size()), tw, th, flags, &frame) != PT_OK)
        return die("pt_render");
    int32_t transport = 0;
    pt_frame_info(frame, nullptr, nullptr, nullptr, &transport);
    const char *transport_name = transport == PT_FRAME_TRANSPORT_RCCL ? "rccl" : transport == PT_FRAME_TRANSPORT_DEVICE_COPIES ? "device_copies" : "none";
    if (transport == PT_FRAME_TRANSPORT_DEVICE_COPIES)
        std::cerr << "pt_render: REHEARSAL -- " << devices.size() << " row bands on " << n_dev << " device(s); the gather is device-to-device "
                     "copies, not the RCCL collective" << std::endl;
    const clk::time_point t_load = clk::now();

    pt_render_params rp;
    std::memset(&rp, 0, sizeof rp);
    rp.width = tw; rp.height = th; rp.row_begin = 0; rp.row_end = th;
    rp.max_ray_reflections = o.max_ray_reflections;
    rp.eps = o.eps; rp.error = o.error; rp.seed = seed;

    if (o.bench_steps > 0) {
        // k whole frames: zero the accumulators, every pass on every device, the gather, wait for all of it
        auto one_frame = [&]() {
            rp.pass_begin = 0;
            rp.pass_count = o.rays_per_pixel;
            return pt_frame_clear(frame) == PT_OK && pt_frame_render(frame, &rp, nullptr) == PT_OK && pt_frame_gather(frame) == PT_OK;
        };
        for (int i = 0; i < std::max(o.bench_warmup, 0); ++i)
            if (!one_frame()) return die("pt_render");
        if (pt_frame_wait(frame) != PT_OK) return die("pt_render");
        const clk::time_point a = clk::now();
        for (int i = 0; i < o.bench_steps; ++i)
            if (!one_frame()) return die("pt_render");
        if (pt_frame_wait(frame) != PT_OK) return die("pt_render");
        const double dt = secs(a, clk::now());
        const double samples = static_cast<double>(tw) * th * o.rays_per_pixel * o.bench_steps;
        // With more than one band: one more frame, untimed, taken apart -- every band's own kernel time (HIP events on its
        // stream), then, with all kernels done, the gather alone on the host's clock -- so that the first run on several devices
        // says where the time went and not only how long it took.
        std::string diagnosis;
        if (devices.size() > 1) {
            pt_render_stats st;
            rp.pass_begin = 0;
            rp.pass_count = o.rays_per_pixel;
            std::vector<float> band_ms(devices.size(), -1.0f);
            if (pt_frame_clear(frame) != PT_OK || pt_frame_render(frame, &rp, &st) != PT_OK || pt_frame_wait(frame) != PT_OK ||
                pt_frame_band_kernel_ms(frame, band_ms.data()) != PT_OK)
                return die("pt_render");
            const clk::time_point g0 = clk::now();
            if (pt_frame_gather(frame) != PT_OK || pt_frame_wait(frame) != PT_OK) return die("pt_render");
            const double gather_ms = secs(g0, clk::now()) * 1e3;
            char buf[64];
            diagnosis = ", \"band_kernel_ms\": [";
            for (size_t b = 0; b < band_ms.size(); ++b) {
                std::snprintf(buf, sizeof buf, "%s%.3f", b ? ", " : "", static_cast<double>(band_ms[b]));
                diagnosis += buf;
            }
            std::snprintf(buf, sizeof buf, "], \"gather_alone_ms\": %.3f", gather_ms);
            diagnosis += buf;
        }
        std::printf("{\"cxx_frame\": true, \"value\": %.3f, \"unit\": \"Msamples/s\", \"ms_per_step\": %.4f, \"steps\": %d, \"warmup\": %d, "
                    "\"bands\": %zu, \"devices_visible\": %d, \"transport\": \"%s\", \"width\": %d, \"height\": %d, \"spp\": %d, \"mrr\": %d, \"error\": %g%s}\n",
                    samples / dt / 1e6, dt / o.bench_steps * 1e3, o.bench_steps, o.bench_warmup, devices.size(), n_dev, transport_name, tw, th,
                    o.rays_per_pixel, o.max_ray_reflections, static_cast<double>(o.error), diagnosis.c_str());
        pt_frame_destroy(frame);
        pt_scene_destroy(scene);
        return 0;
    }

    const size_t px = static_cast<size_t>(tw) * th;
    // Page-locked accumulators: the read-back then runs at PCIe speed without staging copies.  They are allocated on first
    // use -- normally while the GPUs are busy with the frame (pinning 116 MB takes 20 ms, which the host has nothing else to
    // do with between enqueueing the passes and waiting for them).
    struct Pinned {
        void *p = nullptr;
        ~Pinned() { pt_host_free(p); }
    } pin_sum, pin_sum2, pin_count;
    float *sum = nullptr, *sum2 = nullptr;
    int32_t *count = nullptr;
    std::vector<uint8_t> bgr;
    double alloc_s = 0;
    auto ensure_buffers = [&]() {
        if (sum) return true;
        const clk::time_point a = clk::now();
        pin_sum.p = pt_host_alloc(3 * px * sizeof(float));
        pin_sum2.p = pt_host_alloc(3 * px * sizeof(float));
        pin_count.p = pt_host_alloc(px * sizeof(int32_t));
        if (!pin_sum.p || !pin_sum2.p || !pin_count.p) return false;
        sum = static_cast<float *>(pin_sum.p);
        sum2 = static_cast<float *>(pin_sum2.p);
        count = static_cast<int32_t *>(pin_count.p);
        bgr.resize(3 * px);
        alloc_s += secs(a, clk::now());
        return true;
    };
    float disp[3] = {0, INFINITY, 0};
    double read_s = 0, preview_s = 0;

    auto read_back = [&]() {   // gathers the bands (one collective) if any changed, waits, copies the frame out
        if (!ensure_buffers()) return static_cast<int>(PT_ERR_OUT_OF_MEMORY);
        const clk::time_point a = clk::now();
        const int rc = pt_frame_read(frame, sum, sum2, count);
        read_s += secs(a, clk::now());
        return rc;
    };

    // -DEVICE_RESOLVE: the display of the frame, and what a present is asked for
    pt_display *display = nullptr;
    pt_display_params show;
    std::memset(&show, 0, sizeof show);
    show.gamma = o.gamma_correction;
    show.temporal = o.temporal > 0.0f ? 1 : 0;
    show.temporal_params.max_frames = o.temporal;
    show.denoise.levels = o.denoise; show.denoise.sigma_luminance = o.dn_sigma_l; show.denoise.sigma_plane = o.dn_sigma_p;
    if (device_resolve && pt_display_create_frame(frame, o.eps, &display) != PT_OK) return die("pt_render");

    std::vector<uint8_t> out_bgr;   // -RENDER_SCALE s > 1: the written image
    if (scale > 1) out_bgr.resize(3 * static_cast<size_t>(o.width) * o.height);

    // grading on the host path: linear mean and count -> meter and exposure (if automatic; a sequence's frame starts from the
    // previous frame's) -> bloom (-BLOOM) -> grade -> tone map -> the reference's filters -> set_pixel
    bool has_exposure = false;
    float last_exposure = 0.0f;
    auto graded_to_bytes = [&](int w, int h, const float *mean, const int32_t *cnt, uint8_t *out) {
        float e = grade.exposure > 0.0f ? grade.exposure : 1.0f, target = 0.0f;   // (0 = 1, as the library reads it)
        if (grade.auto_exposure) {
            uint32_t hist[PT_METER_ENTRIES];
            if (pt_meter_host(devices[0], w, h, mean, cnt, hist, nullptr) != PT_OK ||
                pt_exposure_from_histogram(hist, &grade, has_exposure ? 1 : 0, last_exposure, &e, &target) != PT_OK)
                return false;
            has_exposure = true;
            last_exposure = e;
        }
        std::vector<float> rgb(3 * static_cast<size_t>(w) * h);
        if (blooming) {
            if (pt_bloom_host(devices[0], w, h, mean, cnt, e, &bloom, rgb.data(), nullptr) != PT_OK) return false;
            mean = rgb.data();
        }
        if (pt_grade_host(w, h, mean, cnt, e, grade.curve, rgb.data()) != PT_OK) return false;
        pt_tonemap(w, h, rgb.data(), cnt, o.gamma_correction, rgb.data());
        if ((o.gauss || o.median) && pt_post_filter_host(devices[0], w, h, rgb.data(), o.gauss, o.median) != PT_OK) return false;
        return pt_quantize(w, h, rgb.data(), cnt, out) == PT_OK;
    };
    // ... from accumulators: their mean is sum / n
    auto graded_from_accumulators = [&](const float *fs, const float *fs2, const int32_t *fc, uint8_t *out) {
        std::vector<float> mean(3 * px);
        std::vector<int32_t> cnt(px);
        pt_denoise_params none;
        std::memset(&none, 0, sizeof none);
        return pt_denoise_host(devices[0], tw, th, fs, fs2, fc, nullptr, nullptr, nullptr, nullptr, &none, mean.data(), cnt.data(), nullptr) == PT_OK &&
               graded_to_bytes(tw, th, mean.data(), cnt.data(), out);
    };
    // the device path's present: plain, scaled, or either with grading
    auto present = [&](pt_display_info *info) {
        if (blooming) return pt_display_present_bloom(display, &show, scale > 1 ? &upsample : nullptr, &grade, &bloom, scale > 1 ? out_bgr.data() : bgr.data(), info, nullptr);
        if (grading) return pt_display_present_graded(display, &show, scale > 1 ? &upsample : nullptr, &grade, scale > 1 ? out_bgr.data() : bgr.data(), info, nullptr);
        return scale > 1 ? pt_display_present_scaled(display, &show, &upsample, out_bgr.data(), info) : pt_display_present(display, &show, bgr.data(), info);
    };

    // -RENDER_SCALE s > 1: the written image, and the host chain that makes it from the traced frame's mean and count --
    // features at the written size from `view` (the scene on the first device, with the frame's camera), the upsample, the
    // tone map, the reference's filters and set_pixel
    auto upsample_to_output = [&](pt_scene *view, const float *mean_lo, const int32_t *count_lo) {
        const size_t opx = static_cast<size_t>(o.width) * o.height;
        std::vector<float> pos(3 * opx), nrm(3 * opx), alb(3 * opx), mean(3 * opx), rgb(3 * opx);
        std::vector<int32_t> hit(opx), count_out(opx);
        pt_render_params fp = rp;
        fp.width = o.width; fp.height = o.height; fp.row_begin = 0; fp.row_end = o.height;
        if (pt_render_features_host(view, &fp, hit.data(), nullptr, pos.data(), nrm.data(), alb.data()) != PT_OK ||
            pt_upsample_host(devices[0], o.width, o.height, mean_lo, count_lo, pos.data(), nrm.data(), alb.data(), hit.data(), &upsample, mean.data(),
                             count_out.data(), nullptr) != PT_OK)
            return false;
        if (grading) return graded_to_bytes(o.width, o.height, mean.data(), count_out.data(), out_bgr.data());
        pt_tonemap(o.width, o.height, mean.data(), count_out.data(), o.gamma_correction, rgb.data());
        if ((o.gauss || o.median) && pt_post_filter_host(devices[0], o.width, o.height, rgb.data(), o.gauss, o.median) != PT_OK) return false;
        return pt_quantize(o.width, o.height, rgb.data(), count_out.data(), out_bgr.data()) == PT_OK;
    };
    // what the files hold: the traced frame's bytes, or the upsampled image's
    auto out_bytes = [&]() { return scale > 1 ? out_bgr.data() : bgr.data(); };

    if (sequence) {
        // n frames: frame i renders its own pass range from its own camera, is merged with the history (-TEMPORAL), denoised
        // (-DENOISE), tone-mapped, filtered, quantized and written; the last one also takes the usual outputs
        float eye0[3], at0[3], up[3], eye1[3], at1[3];
        if (!parse_vec3(o.eye, eye0) || !parse_vec3(o.lookat, at0) || !parse_vec3(o.up, up) ||
            !parse_vec3(o.eye_end.empty() ? o.eye : o.eye_end, eye1) || !parse_vec3(o.lookat_end.empty() ? o.lookat : o.lookat_end, at1)) {
            std::cerr << "pt_render: -EYE / -EYE_END / -LOOKAT / -LOOKAT_END / -UP take three comma-separated numbers, x,y,z" << std::endl;
            return 2;
        }
        const bool own_camera = o.camera || !o.eye_end.empty() || !o.lookat_end.empty();
        pt_scene *view = nullptr;   // the scene on the first device: the history's and the feature buffers' handle
        pt_temporal *history = nullptr;
        if (!display && (o.temporal > 0.0f || o.denoise > 0 || scale > 1) && pt_scene_clone_to_device(scene, devices[0], &view) != PT_OK) return die("pt_render");
        if (!display && o.temporal > 0.0f && pt_temporal_create(view, tw, th, o.eps, &history) != PT_OK) return die("pt_render");
        if (!ensure_buffers()) return die("pt_render");
        std::vector<float> msum, msum2, mean, rgb, pos, nrm, alb;
        std::vector<int32_t> mcount, mean_count, hit;
        if (history) { msum.resize(3 * px); msum2.resize(3 * px); mcount.resize(px); }
        if ((o.denoise > 0 || scale > 1) && !display) { mean.resize(3 * px); mean_count.resize(px); }
        if (o.denoise > 0 && !history && !display) { pos.resize(3 * px); nrm.resize(3 * px); alb.resize(3 * px); hit.resize(px); }
        if ((o.denoise > 0 && !display) || o.gauss || o.median) rgb.resize(3 * px);
        pt_temporal_params tp;
        std::memset(&tp, 0, sizeof tp);
        tp.max_frames = o.temporal;
        pt_denoise_params dp;
        std::memset(&dp, 0, sizeof dp);
        dp.levels = o.denoise; dp.sigma_luminance = o.dn_sigma_l; dp.sigma_plane = o.dn_sigma_p;
        for (int i = 0; i < o.frames; ++i) {
            if (own_camera) {
                float eye[3], at[3];
                for (int k = 0; k < 3; ++k) {
                    eye[k] = static_cast<float>(eye0[k] + (static_cast<double>(eye1[k]) - eye0[k]) * i / std::max(1, o.frames - 1));
                    at[k] = static_cast<float>(at0[k] + (static_cast<double>(at1[k]) - at0[k]) * i / std::max(1, o.frames - 1));
                }
                if (pt_camera_look_at(eye, at, up, o.fov, o.aspect, &camera) != PT_OK || pt_frame_set_camera(frame, &camera) != PT_OK ||
                    (view && pt_scene_set_camera(view, &camera) != PT_OK))
                    return die("pt_render");
            }
            rp.pass_begin = i * o.rays_per_pixel;
            rp.pass_count = o.rays_per_pixel;
            if (pt_frame_clear(frame) != PT_OK || pt_frame_render(frame, &rp, nullptr) != PT_OK) return die("pt_render");
            if (display) {
                // the bytes come from the device; only the last frame is also read back, for the statistics in the output's name
                if (i == o.frames - 1) {
                    if (read_back() != PT_OK) return die("pt_render");
                    pt_resolve(tw, th, sum, sum2, count, o.gamma_correction, bgr.data(), disp);
                }
                if (present(nullptr) != PT_OK) return die("pt_render");
            } else {
                if (read_back() != PT_OK) return die("pt_render");
                pt_resolve(tw, th, sum, sum2, count, o.gamma_correction, bgr.data(), disp);   // the statistics of the frame as rendered
                const float *fs = sum, *fs2 = sum2;
                const int32_t *fc = count;
                if (history) {
                    if (pt_temporal_push_host(history, sum, sum2, count, &tp, o.denoise > 0 ? &dp : nullptr, msum.data(), msum2.data(), mcount.data(),
                                              nullptr, o.denoise > 0 ? mean.data() : nullptr, o.denoise > 0 ? mean_count.data() : nullptr, nullptr) != PT_OK)
                        return die("pt_render");
                    fs = msum.data(); fs2 = msum2.data(); fc = mcount.data();
                } else if (o.denoise > 0) {
                    if (pt_render_features_host(view, &rp, hit.data(), nullptr, pos.data(), nrm.data(), alb.data()) != PT_OK ||
                        pt_denoise_host(devices[0], tw, th, fs, fs2, fc, pos.data(), nrm.data(), alb.data(), hit.data(), &dp, mean.data(),
                                        mean_count.data(), nullptr) != PT_OK)
                        return die("pt_render");
                }
                if (scale > 1) {
                    // the traced frame's mean (the filter's, or sum / n of the frame as rendered or merged), upsampled
                    pt_denoise_params none;
                    std::memset(&none, 0, sizeof none);
                    if (o.denoise == 0 && pt_denoise_host(devices[0], tw, th, fs, fs2, fc, nullptr, nullptr, nullptr, nullptr, &none, mean.data(),
                                                          mean_count.data(), nullptr) != PT_OK)
                        return die("pt_render");
                    if (!upsample_to_output(view, mean.data(), mean_count.data())) return die("pt_render");
                } else if (grading) {
                    // the mean the filter made, or sum / n of the frame as rendered or merged; then meter, grade, tone map
                    if (o.denoise > 0 ? !graded_to_bytes(tw, th, mean.data(), mean_count.data(), bgr.data()) : !graded_from_accumulators(fs, fs2, fc, bgr.data()))
                        return die("pt_render");
                } else if (o.denoise > 0) {
                    pt_tonemap(tw, th, mean.data(), mean_count.data(), o.gamma_correction, rgb.data());
                    if ((o.gauss || o.median) && pt_post_filter_host(devices[0], tw, th, rgb.data(), o.gauss, o.median) != PT_OK) return die("pt_render");
                    pt_quantize(tw, th, rgb.data(), mean_count.data(), bgr.data());
                } else if (o.gauss || o.median) {
                    float unused[3];
                    pt_resolve_float(tw, th, fs, fs2, fc, o.gamma_correction, rgb.data(), unused);
                    if (pt_post_filter_host(devices[0], tw, th, rgb.data(), o.gauss, o.median) != PT_OK) return die("pt_render");
                    pt_quantize(tw, th, rgb.data(), fc, bgr.data());
                } else if (history) {
                    pt_resolve(tw, th, fs, fs2, fc, o.gamma_correction, bgr.data(), nullptr);
                }
            }
            if (o.frames > 1) {
                char frame_name[32];
                std::snprintf(frame_name, sizeof frame_name, "frame_%04d.bmp", i);
                if (pt_write_bmp(frame_name, o.width, o.height, out_bytes()) != PT_OK) return die("pt_render");
            }
            if (!o.quiet) std::cerr << "frame " << i + 1 << " of " << o.frames << std::endl;
        }
        const long long end_time = now_ms();
        const std::time_t t = std::time(nullptr);
        const std::tm *now = std::localtime(&t);
        const std::string name =   // main.cpp:206-213, for the last frame
            std::to_string(now->tm_year + 1900) + '-' + std::to_string(now->tm_mon + 1) + '-' + std::to_string(now->tm_mday) + '-' +
            std::to_string(now->tm_hour) + '-' + std::to_string(now->tm_min) + '-' + std::to_string(now->tm_sec) + "  " +
            std::to_string(end_time - start_time) + "   " + std::to_string(o.rays_per_pixel) + " of " + std::to_string(o.rays_per_pixel) +
            "  max_disp " + std::to_string(disp[0]) + "  min_disp " + std::to_string(disp[1]) + "  aver_disp " + std::to_string(disp[2]);
        int rc = 0;
        if (!o.out.empty()) {
            if (pt_write_bmp(o.out.c_str(), o.width, o.height, out_bytes()) != PT_OK) rc = die("pt_render");
        } else {
            if (pt_write_bmp((name + ".bmp").c_str(), o.width, o.height, out_bytes()) != PT_OK) rc = die("pt_render");
            if (pt_write_bmp("../result.bmp", o.width, o.height, out_bytes()) != PT_OK) rc = die("pt_render");
        }
        std::cout << name << std::endl;
        pt_temporal_destroy(history);
        if (view) pt_scene_destroy(view);
        pt_display_destroy(display);
        pt_frame_destroy(frame);
        pt_scene_destroy(scene);
        return rc;
    }

    // Pass slices end exactly where the reference writes a preview (after every pass p with p % update == 0,
    // main.cpp:144-158) so that previews happen between GPU calls; with a time limit they are also kept short.
    int rays_count = 0;
    double ms_per_pass = 0;   // measured on the previous slice (0 = not yet known)
    while (rays_count < o.rays_per_pixel) {
        const long long elapsed_ms = now_ms() - start_time;
        if (o.time_limit != 0 && elapsed_ms >= 1000LL * o.time_limit) break;   // main.cpp:111-114
        int slice_end = o.rays_per_pixel;
        if (o.update != 0) {
            const int next_preview = (rays_count % o.update == 0) ? rays_count : (rays_count / o.update + 1) * o.update;
            slice_end = std::min(o.rays_per_pixel, next_preview + 1);
        }
        if (o.time_limit != 0) {
            // the reference would start every pass that begins before the deadline: run as many as are expected to,
            // at most ~75 ms worth, at least one
            int n = 1;
            if (ms_per_pass > 0) {
                const double left_ms = 1000.0 * o.time_limit - static_cast<double>(elapsed_ms);
                n = static_cast<int>(std::min(75.0, left_ms) / ms_per_pass);
                n = std::max(1, n);
            }
            slice_end = std::min(slice_end, rays_count + n);
        }
        rp.pass_begin = rays_count;
        rp.pass_count = slice_end - rays_count;
        const clk::time_point a = clk::now();
        if (pt_frame_render(frame, &rp, nullptr) != PT_OK) return die("pt_render");
        if (o.time_limit != 0) {   // wait for the slice (without asking for statistics: the statistics-free kernels are the fast ones)
            if (pt_frame_wait(frame) != PT_OK) return die("pt_render");
            ms_per_pass = 1e3 * secs(a, clk::now()) / rp.pass_count;
        }
        for (int p = rays_count; p < slice_end; ++p) {
            if (o.update != 0 && p % o.update == 0) {
                const clk::time_point b = clk::now();
                if (read_back() != PT_OK) return die("pt_render");
                pt_resolve(tw, th, sum, sum2, count, o.gamma_correction, bgr.data(), nullptr);
                if (o.out.empty() && pt_write_bmp("../result.bmp", tw, th, bgr.data()) != PT_OK)
                    std::cerr << pt_last_error() << std::endl;   // the reference's save_image only prints, too
                std::cerr << "Image update" << std::endl;
                preview_s += secs(b, clk::now());
            }
            if (!o.quiet) std::cerr << p + 1 << " rays per pixel were sent" << std::endl;
        }
        rays_count = slice_end;
    }
    const clk::time_point t_enqueued = clk::now();
    if (pt_frame_gather(frame) != PT_OK) return die("pt_render");   // the frame's one collective (nothing to do for one band)
    const double alloc_before = alloc_s;
    if (!ensure_buffers()) return die("pt_render");                 // (while the devices work)
    const double alloc_in_wait = alloc_s - alloc_before;
    if (pt_frame_wait(frame) != PT_OK) return die("pt_render");     // the last slice (and, in a fresh process, the
    const clk::time_point t_kernels = clk::now();                    // one-time load of the kernels' code object)
    if (read_back() != PT_OK) return die("pt_render");
    const clk::time_point t_render = clk::now();

    double features_s = 0, denoise_s = 0;
    float denoise_kernel_ms = 0;
    if (display) {
        // the statistics of the frame as rendered, on the host; the image's bytes from the device (features, denoiser, tone map)
        pt_resolve(tw, th, sum, sum2, count, o.gamma_correction, bgr.data(), disp);
        const clk::time_point f1 = clk::now();
        pt_display_info shown;
        if (present(&shown) != PT_OK) return die("pt_render");
        if (o.denoise > 0) {
            denoise_s = secs(f1, clk::now());
            denoise_kernel_ms = shown.kernel_ms;
        }
    } else if (scale > 1) {
        // the statistics of the traced frame; its mean (the filter's with -DENOISE, else sum / n); the upsample to the written size
        std::vector<float> mean(3 * px), pos, nrm, alb;
        std::vector<int32_t> hit, count_lo(px);
        pt_resolve(tw, th, sum, sum2, count, o.gamma_correction, bgr.data(), disp);
        pt_scene *view = nullptr;
        if (pt_scene_clone_to_device(scene, devices[0], &view) != PT_OK) return die("pt_render");
        pt_denoise_params dp;
        std::memset(&dp, 0, sizeof dp);
        dp.levels = o.denoise; dp.sigma_luminance = o.dn_sigma_l; dp.sigma_plane = o.dn_sigma_p;
        if (o.denoise > 0) {
            pos.resize(3 * px); nrm.resize(3 * px); alb.resize(3 * px); hit.resize(px);
            if (pt_render_features_host(view, &rp, hit.data(), nullptr, pos.data(), nrm.data(), alb.data()) != PT_OK) return die("pt_render");
        }
        const clk::time_point f1 = clk::now();
        if (pt_denoise_host(devices[0], tw, th, sum, sum2, count, pos.data(), nrm.data(), alb.data(), hit.data(), &dp, mean.data(), count_lo.data(),
                            &denoise_kernel_ms) != PT_OK)
            return die("pt_render");
        const bool ok = upsample_to_output(view, mean.data(), count_lo.data());
        pt_scene_destroy(view);
        if (!ok) return die("pt_render");
        denoise_s = secs(f1, clk::now());
    } else if (o.denoise > 0) {
        // the statistics of the frame as rendered; then the first hits of the pinhole view on the frame's first device, the
        // denoiser on the linear mean, the tone map, the reference's filters and set_pixel
        std::vector<float> rgb(3 * px), mean(3 * px), pos(3 * px), nrm(3 * px), alb(3 * px);
        std::vector<int32_t> hit(px), count_out(px);
        pt_resolve_float(tw, th, sum, sum2, count, o.gamma_correction, rgb.data(), disp);
        const clk::time_point f0 = clk::now();
        pt_scene *view = nullptr;
        if (pt_scene_clone_to_device(scene, devices[0], &view) != PT_OK) return die("pt_render");
        const int frc = pt_render_features_host(view, &rp, hit.data(), nullptr, pos.data(), nrm.data(), alb.data());
        pt_scene_destroy(view);
        if (frc != PT_OK) return die("pt_render");
        const clk::time_point f1 = clk::now();
        pt_denoise_params dp;
        std::memset(&dp, 0, sizeof dp);
        dp.levels = o.denoise; dp.sigma_luminance = o.dn_sigma_l; dp.sigma_plane = o.dn_sigma_p;
        if (pt_denoise_host(devices[0], tw, th, sum, sum2, count, pos.data(), nrm.data(), alb.data(), hit.data(), &dp,
                            mean.data(), count_out.data(), &denoise_kernel_ms) != PT_OK)
            return die("pt_render");
        features_s = secs(f0, f1);
        denoise_s = secs(f1, clk::now());
        if (grading) {
            if (!graded_to_bytes(tw, th, mean.data(), count_out.data(), bgr.data())) return die("pt_render");
        } else {
            pt_tonemap(tw, th, mean.data(), count_out.data(), o.gamma_correction, rgb.data());
            if ((o.gauss || o.median) && pt_post_filter_host(devices[0], tw, th, rgb.data(), o.gauss, o.median) != PT_OK) return die("pt_render");
            pt_quantize(tw, th, rgb.data(), count_out.data(), bgr.data());
        }
    } else if (grading) {   // the statistics of the frame as rendered; then sum / n, meter, grade, tone map, filters, set_pixel
        pt_resolve(tw, th, sum, sum2, count, o.gamma_correction, bgr.data(), disp);
        if (!graded_from_accumulators(sum, sum2, count, bgr.data())) return die("pt_render");
    } else if (o.gauss || o.median) {   // main.cpp:187-201: filters act on the tonemapped float image, then set_pixel
        std::vector<float> rgb(3 * px);
        pt_resolve_float(tw, th, sum, sum2, count, o.gamma_correction, rgb.data(), disp);
        if (pt_post_filter_host(devices[0], tw, th, rgb.data(), o.gauss, o.median) != PT_OK) return die("pt_render");
        pt_quantize(tw, th, rgb.data(), count, bgr.data());
    } else {
        pt_resolve(tw, th, sum, sum2, count, o.gamma_correction, bgr.data(), disp);
    }
    const clk::time_point t_resolve = clk::now();
    const long long end_time = now_ms();
    const std::time_t t = std::time(nullptr);
    const std::tm *now = std::localtime(&t);
    const std::string name =   // main.cpp:206-213
        std::to_string(now->tm_year + 1900) + '-' + std::to_string(now->tm_mon + 1) + '-' + std::to_string(now->tm_mday) + '-' +
        std::to_string(now->tm_hour) + '-' + std::to_string(now->tm_min) + '-' + std::to_string(now->tm_sec) + "  " +
        std::to_string(end_time - start_time) + "   " + std::to_string(rays_count) + " of " + std::to_string(o.rays_per_pixel) +
        "  max_disp " + std::to_string(disp[0]) + "  min_disp " + std::to_string(disp[1]) + "  aver_disp " + std::to_string(disp[2]);
    int rc = 0;
    if (!o.out.empty()) {
        if (pt_write_bmp(o.out.c_str(), o.width, o.height, out_bytes()) != PT_OK) rc = die("pt_render");
    } else {
        if (pt_write_bmp((name + ".bmp").c_str(), o.width, o.height, out_bytes()) != PT_OK) rc = die("pt_render");
        if (pt_write_bmp("../result.bmp", o.width, o.height, out_bytes()) != PT_OK) rc = die("pt_render");
    }
    std::cout << name << std::endl;
    if (o.timing) {
        const clk::time_point t_end = clk::now();
        double host_s[2] = {0, 0};
        pt_scene_timings(scene, host_s);
        std::fprintf(stderr, "{\"pre_main_s\": %.4f, \"parse_s\": %.4f, \"hip_startup_s\": %.4f, \"frame_setup_s\": %.4f, \"host_alloc_s\": %.4f, "
                             "\"enqueue_s\": %.4f, \"hierarchy_build_s\": %.4f, \"kernels_wait_s\": %.4f, \"read_back_s\": %.4f, \"previews_s\": %.4f, "
                             "\"resolve_s\": %.4f, \"bmp_write_s\": %.4f, \"main_s\": %.4f, \"bands\": %zu, \"transport\": \"%s\", "
                             "\"features_s\": %.4f, \"denoise_s\": %.4f, \"denoise_kernel_ms\": %.3f}\n",
                     pre_main_s, secs(t_begin, t_parse), secs(t_parse, t_hip), secs(t_hip, t_load), alloc_in_wait,
                     secs(t_load, t_enqueued) - preview_s, host_s[1], secs(t_enqueued, t_kernels) - alloc_in_wait, secs(t_kernels, t_render), preview_s,
                     secs(t_render, t_resolve), secs(t_resolve, t_end), secs(t_begin, t_end), devices.size(), transport_name, features_s, denoise_s,
                     static_cast<double>(denoise_kernel_ms));
    }
    if (o.fast_exit) {
        // Every file is written and closed; tearing the HIP runtime down (code objects, device heap, RCCL) is all that a normal
        // exit would add.
        std::cout.flush();
        std::cerr.flush();
        std::_Exit(rc);
    }
    pt_display_destroy(display);
    pt_frame_destroy(frame);
    pt_scene_destroy(scene);
    return rc;
}
