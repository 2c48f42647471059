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
// A projection (pt_scene_set_projection, not in the reference): -PROJECTION perspective|ortho|fisheye|equirect (default perspective:
// nothing changes).  ortho: parallel rays along the view direction from a plane -ORTHO_HEIGHT <h> scene units high and h x -ASPECT
// wide around -EYE (default: the height the perspective view of -FOV has at the distance |LOOKAT - EYE|, 2 tan(FOV / 2) times it).
// fisheye: equidistant, -FOV is the angle across the image height (and FOV x ASPECT across its width; it may exceed 180).  equirect:
// the full sphere, 360 x 180 degrees.  An unknown name ends the program; -APERTURE, -SHUTTER and -TEMPORAL are refused with a
// projection other than perspective, with the library's message.  PT_RENDER_PRINT_CAMERA=1 then also prints
// "projection <kind> <span_x> <span_y>".
// An environment (pt_scene_set_environment_file, not in the reference): -ENV <file.hdr|file.pfm> lights the scene with an HDR panorama
// (a miss adds throughput x radiance; it is the background too), -ENV_GAIN <g> scales it (default 1), -ENV_ROTATE <degrees> turns it
// about +y (default 0), -ENV_SIZE <n> is the size of the octahedral map it is resampled into (default 0: by the picture's height).
// -ENV together with -SKYBOX is refused; -ENV_GAIN, -ENV_ROTATE and -ENV_SIZE need -ENV.  Every other flag combines.
// Dielectric materials (pt_scene_set_dielectrics, not in the reference): -GLASS m:ior[:r:g:b][,m:ior[:r:g:b]...] makes material m of
// the model (counted as usemtl counts them) smooth glass of refractive index ior (0.125 .. 8) whose transmitted light is multiplied
// by the tint r:g:b (each 0 .. 1, default 1:1:1), e.g. -GLASS 4:1.5 or -GLASS 4:1.5:0.9:1:0.9,2:1.33.  A malformed entry, a value out
// of range, an index outside the model and an emissive material end the program with status 2.  Every other flag combines.
// Albedo textures (pt_scene_set_textures, not in the reference): -TEXTURE m:file.bmp[:nearest|bilinear][,m:file.bmp...] multiplies the
// diffuse (or emissive) colour of material m of the model (counted as usemtl counts them) by the 24-bit BMP, looked up at the OBJ's vt
// coordinates with repeat wrap (default bilinear); -TEXTURE mtl takes every map_Kd line of the model's MTL instead, the files relative
// to -MODEL_PATH.  -TEXTURE_GAMMA <g> decodes the bytes as pow(b / 255, g) (default 2.2; 1 = linear).  A malformed entry, an unreadable
// file, an index outside the model and a material that is also in -GLASS end the program with status 2.  Every other flag combines.
// Smooth shading (pt_scene_set_shading_normals, not in the reference): -SMOOTH auto generates a normal per triangle corner from the mesh
// (pt_smooth_normals: welded vertices, angle-weighted, faces within -CREASE degrees of each other, default 60) and shades the glossy
// and diffuse lobes and the dielectrics with the interpolated normal; -SMOOTH vn loads the model with PT_LOAD_GEOMETRIC_PLANES and takes
// the file's own vn instead.  A malformed value, -CREASE without -SMOOTH auto or outside 0 .. 180 end the program with status 2.  Every
// other flag combines.  Not built: normal maps and smoothing groups (`s` lines).
// Rough specular reflection (pt_scene_set_roughness, not in the reference): -ROUGH m:alpha[,m:alpha...] gives the glossy lobe of each
// material m a GGX lobe of roughness alpha in 2^-10 .. 1 instead of the mirror; -ROUGH mtl takes every material of the model's MTL that
// has a Pr line and a glossy lobe (Ns and Ks not zero, not emissive), with Pr clamped into that range.  A malformed entry, an alpha
// outside the range, an index outside the model, a material listed twice, one without a glossy lobe and one that is also in -GLASS end
// the program with status 2.  Every other flag combines.  Not built: rough dielectrics, anisotropy, a Fresnel term, roughness textures.
// Direct lighting (pt_scene_set_direct_lighting, not in the reference): -DIRECT 1 sends a shadow ray to a sampled point of a light at
// every scattering diffuse hit and counts every path once (pt_hip.h: direct lighting); -DIRECT 0 is a run without the flag.  Any
// other value, a model without a light and an emissive material that -TEXTURE lists end the program with status 2.  Every other flag
// combines.  Not built: multiple importance sampling, sampling by power, direct terms for the GGX lobe, textured emitters.
// Environment sampling (pt_scene_set_environment_sampling, not in the reference): -DIRECT_ENV 1, with -ENV, sends the shadow ray of every
// scattering diffuse hit to a direction drawn from the environment in proportion to its radiance or -- where the model has emitters --
// to a point of a light, the environment with probability -DIRECT_ENV_SHARE p (0 < p < 1; default: by the two sources' power, within
// 1/8 .. 7/8), and counts every path once (pt_hip.h: environment sampling); -DIRECT_ENV 0 is a run without the flag.  A missing -ENV, a
// -SKYBOX, a share outside the range, a black environment and an emissive material that -TEXTURE lists end the program with status 2.
// Every other flag combines, -DIRECT too.  Not built: multiple importance sampling with the diffuse lobe, a term for the GGX lobe.
// Russian roulette (pt_scene_set_roulette, not in the reference): -RR start[:floor], with -DIRECT 1 or -DIRECT_ENV 1, ends a path from
// scattering step `start` (a whole number >= 1) on with a probability that follows its throughput and divides the survivors by it, the
// probability of surviving never below `floor` (2^-10 .. 1; default 1/16), so the estimate stays unbiased and -MRR can be raised until
// the cap no longer matters (pt_hip.h: Russian roulette); -RR 0 is a run without the flag.  A malformed value, one out of range and
// -RR without either of the two flags end the program with status 2.  Every other flag combines.
// The denoiser (pt_denoise_host, not in the reference): -DENOISE <levels> (default 0: off; 5 is the usual choice) filters the final
// image's linear mean with the feature-guided a-trous filter before the tone map, -DN_SIGMA_L / -DN_SIGMA_P set its luminance and
// plane-distance widths (default 0: the library's).  The dispersion numbers and the file name are those of the undenoised frame; the
// filter runs on the first device of the frame.  Previews (-UPDATE) stay undenoised.  Without the flag nothing changes.
// A sequence (pt_temporal_*, not in the reference): -FRAMES n (default 1) renders n frames, frame i with passes [i RPP, (i + 1) RPP)
// of the same seed, and writes each as frame_%04d.bmp in the working directory; the last frame also takes the usual outputs (the
// named file and ../result.bmp, or -OUT).  -EYE_END x,y,z and -LOOKAT_END x,y,z (default: -EYE and -LOOKAT) move the camera: frame
// i looks from start + (end - start) i / (n - 1), computed in double, through pt_camera_look_at.  -TEMPORAL m (default 0: off)
// merges every frame with the reprojected history of the earlier ones before it is resolved, m being the cap of the history's age
// in frames (32 is the usual choice); with -DENOISE the filter then runs on the merged frame, in the same chain on the device.
// A sequence writes no previews and prints no -TIMING line, and -TL with -FRAMES > 1 is refused.  Without -FRAMES and -TEMPORAL
// nothing changes.
// Motion blur (pt_scene_set_camera_motion, not in the reference): -SHUTTER f (0 <= f <= 1, default 0: off) keeps the shutter open
// for the fraction f of a frame interval.  Frame i starts at its pose above and ends at the pose of the same formula with i + f in
// place of i (beyond -EYE_END for the last frame; with -FRAMES 1 at EYE + f (EYE_END - EYE)); every path draws its own time in
// between (PT_RENDER_PRINT_CAMERA=1 then also prints both poses of every frame, "shutter <frame> start|end" and twelve numbers).
// Features, the temporal history and the display stages use the start pose.  Without -SHUTTER, with -SHUTTER 0 or
// without -EYE_END / -LOOKAT_END every file is byte-identical.
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
// 1: no smoothing> -- in a sequence frame i starts from frame i - 1's exposure.  Previews (-UPDATE) stay ungraded.  It works on
// the host path and with -DEVICE_RESOLVE 1, with byte-identical files, and with -RENDER_SCALE, -DENOISE, -TEMPORAL and -FRAMES.  Without any of these
// flags nothing changes.
// Bloom (pt_bloom_host, pt_display_present_bloom, not in the reference): -BLOOM <strength, default 0: off> spreads the light above
// -BLOOM_THRESHOLD <luminance after exposure, default 1> over its neighbourhood with a pyramid of -BLOOM_LEVELS <1 .. 8, default 5>
// levels, on the linear mean at the written size, after the meter and before the grade (without -TONE / -EXPOSURE / -AUTO_EXPOSURE
// the grade is the reference's: no curve, e = 1); previews stay unbloomed.
// It works on the host path and with -DEVICE_RESOLVE 1, with byte-identical files, and with every flag grading works with.
// Without -BLOOM, or with -BLOOM 0, nothing changes.
// Local exposure (pt_local_host, pt_display_present_local, not in the reference): -LOCAL <strength, default 0: off> multiplies every
// pixel by a gain from an edge-aware base of the luminance around it -- above -LOCAL_PIVOT <luminance after exposure, default 0.18>
// it is pulled down, below it lifted by at most 1 + strength -- made with -LOCAL_LEVELS <1 .. 8, default 5> levels of a 5 x 5
// spline whose range weight is -LOCAL_SIGMA <default 0.5>, on the linear mean at the written size, after bloom and before the
// grade (alone it runs with the zeroed grade, as -BLOOM does); previews stay as they are.  It works on the host path and with
// -DEVICE_RESOLVE 1, with byte-identical files, and with every flag grading works with.  Without -LOCAL, or with -LOCAL 0, nothing changes.
// Colour grading (pt_colour_host, pt_display_present_colour, not in the reference): -WB <r,g,b gains, default 1,1,1>, -SATURATION <s,
// default 1; 0 is grey> and -COLOR_MATRIX <m00,..,m22, row-major, default the identity> are folded into one 3 x 3 matrix on the
// linear mean, after local exposure and before the exposure and the curve; -LUT <file.cube> applies a 3D LUT (LUT_3D_SIZE 2 .. 65,
// domain 0 .. 1, tetrahedral interpolation) to the curve's output, before the gamma conversion.  The meter, bloom and local exposure
// see the mean before the matrix; previews stay as they are.  It works on the host path and with -DEVICE_RESOLVE 1, with
// byte-identical files, and with every flag grading works with (alone it runs with the zeroed grade).  Without these flags nothing
// changes.
// Lens optics (pt_optics_host, pt_display_present_optics, not in the reference): -DISTORTION <k1,k2, default 0,0> bends straight lines
// (f = 1 + r2 (k1 + k2 r2) with r measured in half image heights; k1 < 0 barrel, k1 > 0 pincushion), -CA <a, default 0> magnifies the
// red and blue channels by 1 - a and 1 + a (lateral chromatic aberration), -VIGNETTE <v, default 0> darkens the corners by
// 1 / (1 + v r2)^2, on the linear mean at the written size, after the upsample and BEFORE the meter, bloom, local exposure and the
// grade, which see the image the lens delivers and its count; previews stay as they are.  The library judges the values (|k| <= 4,
// |a| <= 0.25, 0 <= v <= 64) and its message goes to stderr with exit status 2.  It works on the host path and with -DEVICE_RESOLVE 1,
// with byte-identical files, and with every flag grading works with (alone it runs with the zeroed grade).  Without these flags
// nothing changes.
// Sharpening (pt_sharpen_host, pt_display_present_sharpen, not in the reference): -SHARPEN <strength in 0 .. 1, default 0: off>
// multiplies every pixel by a gain from a contrast-adaptive sharpen of its compressed luminance against the four pixels round it,
// whose negative lobe is at most -SHARPEN_LIMIT <in 0 .. 0.1875, default 0: 0.1875>, on the linear mean at the written size, after
// bloom and local exposure and immediately before the colour stage or the grade (alone it runs with the zeroed grade, as -LOCAL
// does); the meter does not see it, and previews stay as they are.  It works on the host path and with -DEVICE_RESOLVE 1, with
// byte-identical files, and with every flag grading works with.  Without -SHARPEN, or with -SHARPEN 0, nothing changes.
// Film grain and dithered quantization (pt_grain_quantize, pt_display_present_grain, not in the reference): -GRAIN <strength in 0 .. 1,
// default 0: off> adds monochrome grain of lattice pitch -GRAIN_SIZE <pixels in 1 .. 8, default 1> to the graded value, weighted
// towards the mid-tones; -DITHER <amount in 0 .. 1 levels, default 0: off> dithers the 8-bit quantization with triangular noise, which
// takes the bands out of smooth gradients; -GRAIN_SEED <n, default 0> seeds both, and a -FRAMES sequence draws new noise every frame
// (the frame's index).  It is the chain's last step, in the place of the tone map and the quantization (alone it runs with the zeroed
// grade); black, clipped white and emitters keep their bytes under grain.  It works on the host path and with -DEVICE_RESOLVE 1, with
// byte-identical files, and with every flag grading works with, but not with -GAUSS / -MEDIAN.  Without -GRAIN and -DITHER nothing changes.
// Scene-linear output (pt_linear_encode, pt_display_present_linear, not in the reference): -LINEAR_OUT <file.pfm | file.hdr> also writes
// the LINEAR mean of the final image -- after optics, bloom, local exposure and sharpening, before the colour stage, the exposure, the
// curve and the grain -- as a PFM (three floats per pixel) or a flat Radiance picture (RGBE); the extension picks the format and any
// other is refused.  -LINEAR_EXPOSED 1 multiplies it by the exposure the grade used (metered or -EXPOSURE) and needs one of the flags
// that make a grade.  The file goes beside the final BMP, never beside a preview; in a -FRAMES sequence every frame_%04d.bmp has its
// frame_%04d.pfm / .hdr too.  -GAUSS / -MEDIAN act behind the tone map and do not touch it.  It works on the host path and with
// -DEVICE_RESOLVE 1, with byte-identical files; the BMPs are those of a run without the flag.  PT_RENDER_PRINT_CONFIG=1 prints
// linear_out, linear_format and linear_exposed behind the reference's fields when the flags are given.  Without -LINEAR_OUT nothing
// changes.
// The image chain is stated once, in HostChain::bytes, in the order the paragraphs above give: temporal merge -> first-hit
// features and denoise (else sum / n where a mean is needed) -> upsample to the written size -> optics -> meter, bloom, local exposure, sharpening, colour / grade -> tone map
// -> -GAUSS / -MEDIAN -> quantize (or grain and dithered quantization in the last three's place).  A single frame and every frame of a sequence go through it; with -DEVICE_RESOLVE 1 the
// bytes come from present() instead.
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

using clk = std::chrono::steady_clock;

// What the run is asked for: the flags as parse() reads them (defaults: config.h:16-29), then what configure() makes of them.
struct Options {
    int height = 512, width = 512, rays_per_pixel = 20, max_ray_reflections = 8, median = 0, gauss = 0;   // --H x --W: the written size
    float eps = 1e-4f, error = 0.001f;
    int update = 32;
    float gamma_correction = 1 / 2.2f;
    std::string model_path = "../models/", model_name = "Tor.obj", skybox;
    int seed = 42, time_limit = 0;
    std::string out;
    int device = 0, quiet = 0, timing = 0;
    int gpus = 0, rehearse = 0, selfcoll = 0, bench_steps = 0, bench_warmup = 1, fast_exit = 0;
    std::string device_names;      // -DEVICES as given
    long long t0_ns = 0;   // -T0_NS: CLOCK_REALTIME of the parent just before it started this process (bench.py), for the start-up phase
    bool camera = false;   // any of -EYE / -LOOKAT / -UP / -FOV / -ASPECT given
    std::string eye = "0,0,-20", lookat = "0,0,0", up = "0,1,0", eye_end, lookat_end;   // as given ("" = the start value)
    float fov = 53.13010235415598f, aspect = 0.0f;
    std::string env, env_gain, env_rotate, env_size;   // -ENV / -ENV_GAIN / -ENV_ROTATE / -ENV_SIZE as given
    pt_environment_params env_params = {1.0f, 0.0f, 0};
    std::string glass_text;                // -GLASS as given
    std::string rough_text;                // -ROUGH as given
    std::string direct_text;               // -DIRECT as given
    bool direct = false;
    std::string direct_env_text, direct_env_share_text;   // -DIRECT_ENV, -DIRECT_ENV_SHARE as given
    bool direct_env = false;
    float direct_env_share = 0.0f;         // 0 = the library's default
    std::string rr_text;                   // -RR as given
    int32_t rr_start = 0;                  // 0 = no roulette
    float rr_floor = PT_ROULETTE_DEFAULT_FLOOR;
    std::vector<pt_rough> rough;           // what it makes (empty with -ROUGH mtl: the model's MTL decides)
    bool rough_mtl = false;
    std::string smooth_text, crease_text;  // -SMOOTH / -CREASE as given
    int smooth = 0;                        // what they make: 0 none, 1 auto, 2 vn
    float crease = PT_SMOOTH_DEFAULT_CREASE;
    std::string texture_text, texture_gamma_text;   // -TEXTURE / -TEXTURE_GAMMA as given
    struct TextureSpec { int32_t material; std::string file; int32_t filter; };
    std::vector<TextureSpec> textures;     // what -TEXTURE makes (empty with -TEXTURE mtl: the model's MTL decides)
    bool texture_mtl = false;
    float texture_gamma = 2.2f;
    std::vector<pt_dielectric> glass;      // what it makes
    std::string projection_name = "perspective", ortho_height;   // -PROJECTION / -ORTHO_HEIGHT as given
    pt_projection projection{};    // what they make; kind 0 (perspective) = none is set
    float view_height = 0.0f;      // -PROJECTION ortho: the height of the view in scene units
    std::string aperture, focus;   // -APERTURE / -FOCUS as given
    std::string shutter_text;      // -SHUTTER as given
    float shutter = 0.0f;          // the fraction of a frame interval the shutter is open; 0 = off
    bool aperture_given = false, focus_given = false;
    int frames = 1;                // -FRAMES
    int device_resolve = 0;        // -DEVICE_RESOLVE as given
    int scale = 1;                 // -RENDER_SCALE: the frame is traced at (W / s) x (H / s) and upsampled to W x H
    std::string tone = "reference";   // -TONE
    bool tone_flags = false;       // any of -TONE / -EXPOSURE / -AUTO_EXPOSURE given
    float exposure_stops = 0.0f, key = 0.0f, adapt = 0.0f;   // -EXPOSURE, -KEY, -ADAPT (0 = the library's default)
    int auto_exposure = 0, percentile = 0;                   // -AUTO_EXPOSURE, -PERCENTILE
    // each stage's parameters, built once (a zeroed block holds the library's defaults)
    pt_denoise_params denoise{};   // -DENOISE (levels, 0 = off), -DN_SIGMA_L, -DN_SIGMA_P
    pt_temporal_params temporal{}; // -TEMPORAL: max_frames of the history, 0 = no temporal stage
    pt_bloom_params bloom{};       // -BLOOM, -BLOOM_THRESHOLD, -BLOOM_LEVELS
    pt_local_params local{};       // -LOCAL, -LOCAL_PIVOT, -LOCAL_LEVELS, -LOCAL_SIGMA
    pt_sharpen_params sharpen{};   // -SHARPEN, -SHARPEN_LIMIT
    pt_grain_params grain{};       // -GRAIN, -GRAIN_SIZE, -DITHER, -GRAIN_SEED (frame: set per image)
    std::string wb, saturation, colour_matrix, lut_path;   // -WB, -SATURATION, -COLOR_MATRIX, -LUT as given
    pt_colour_params colour{};     // what they make; colour.lut is owned here
    pt_lut *lut = nullptr;
    std::string distortion, ca, vignette;   // -DISTORTION, -CA, -VIGNETTE as given
    pt_optics_params optics{};     // what they make
    std::string linear_out;        // -LINEAR_OUT as given
    int linear_exposed = 0;        // -LINEAR_EXPOSED as given
    pt_linear_params linear{};     // what they make; format 0 without -LINEAR_OUT
    pt_upsample_params upsample{};
    pt_grade_params grade{};       // zeroed without -TONE / -EXPOSURE / -AUTO_EXPOSURE: the reference's bytes
    pt_display_params show{};      // what a present of the device path is asked for
    // what configure() resolves
    int tw = 0, th = 0;            // the traced size
    unsigned rng_seed = 0;         // config.h:101-104
    bool sequence = false;         // -FRAMES > 1 or -TEMPORAL
    bool merging = false;          // -TEMPORAL > 0
    bool display = false;          // -DEVICE_RESOLVE 1 and nothing that keeps the image on the host path
    bool blooming = false, localising = false, grading = false;   // -BLOOM > 0; -LOCAL > 0; either, colour, or any of the tone flags
    bool colouring = false;        // a matrix that is not the identity, or a LUT
    bool sharpening = false;       // -SHARPEN > 0 (it makes `grading` true as well)
    bool graining = false;         // -GRAIN > 0 or -DITHER > 0 (it makes `grading` true as well)
    bool optical = false;          // any of -DISTORTION / -CA / -VIGNETTE is not zero (it makes `grading` true as well)
    pt_camera view;                // with `camera`
    pt_lens lens{0.0f, 0.0f};
    bool has_lens = false;
    float eye0[3], at0[3], up0[3], eye1[3], at1[3];   // the vectors, parsed; a sequence moves from 0 to 1
    bool moving = false;           // a sequence sets a camera of its own every frame
    bool blurring = false;         // -SHUTTER > 0 and a camera that moves: every frame gets an end pose (pt_frame_set_camera_motion)
    std::vector<int32_t> devices;  // row bands -> devices; choose_devices() fills it once the device count is known
    Options() = default;
    Options(const Options &) = delete;
    ~Options() { pt_lut_destroy(lut); }
};

long long now_ms() {
    using namespace std::chrono;
    return duration_cast<milliseconds>(system_clock::now().time_since_epoch()).count();
}

double secs(clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); }

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
        if (f == "-DEVICES") o.device_names = v;
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
        if (f == "-PROJECTION") o.projection_name = v;
        if (f == "-ENV") o.env = v;
        if (f == "-ENV_GAIN") o.env_gain = v;
        if (f == "-ENV_ROTATE") o.env_rotate = v;
        if (f == "-ENV_SIZE") o.env_size = v;
        if (f == "-GLASS") o.glass_text = v;
        if (f == "-ROUGH") o.rough_text = v;
        if (f == "-DIRECT") o.direct_text = v;
        if (f == "-DIRECT_ENV") o.direct_env_text = v;
        if (f == "-DIRECT_ENV_SHARE") o.direct_env_share_text = v;
        if (f == "-RR") o.rr_text = v;
        if (f == "-SMOOTH") o.smooth_text = v;
        if (f == "-CREASE") o.crease_text = v;
        if (f == "-TEXTURE") o.texture_text = v;
        if (f == "-TEXTURE_GAMMA") o.texture_gamma_text = v;
        if (f == "-ORTHO_HEIGHT") o.ortho_height = v;
        if (f == "-APERTURE") { o.aperture = v; o.aperture_given = true; }
        if (f == "-FOCUS") { o.focus = v; o.focus_given = true; }
        if (f == "-SHUTTER") o.shutter_text = v;
        if (f == "-DENOISE") o.denoise.levels = std::atoi(v);
        if (f == "-DN_SIGMA_L") o.denoise.sigma_luminance = static_cast<float>(std::atof(v));
        if (f == "-DN_SIGMA_P") o.denoise.sigma_plane = static_cast<float>(std::atof(v));
        if (f == "-FRAMES") o.frames = std::atoi(v);
        if (f == "-TEMPORAL") o.temporal.max_frames = static_cast<float>(std::atof(v));
        if (f == "-EYE_END") o.eye_end = v;
        if (f == "-LOOKAT_END") o.lookat_end = v;
        if (f == "-DEVICE_RESOLVE") o.device_resolve = std::atoi(v);
        if (f == "-RENDER_SCALE") o.scale = std::atoi(v);
        if (f == "-TONE") { o.tone = v; o.tone_flags = true; }
        if (f == "-EXPOSURE") { o.exposure_stops = static_cast<float>(std::atof(v)); o.tone_flags = true; }
        if (f == "-AUTO_EXPOSURE") { o.auto_exposure = std::atoi(v); o.tone_flags = true; }
        if (f == "-KEY") o.key = static_cast<float>(std::atof(v));
        if (f == "-PERCENTILE") o.percentile = std::atoi(v);
        if (f == "-ADAPT") o.adapt = static_cast<float>(std::atof(v));
        if (f == "-BLOOM") o.bloom.strength = static_cast<float>(std::atof(v));
        if (f == "-BLOOM_THRESHOLD") o.bloom.threshold = static_cast<float>(std::atof(v));
        if (f == "-BLOOM_LEVELS") o.bloom.levels = std::atoi(v);
        if (f == "-LOCAL") o.local.strength = static_cast<float>(std::atof(v));
        if (f == "-LOCAL_PIVOT") o.local.pivot = static_cast<float>(std::atof(v));
        if (f == "-LOCAL_LEVELS") o.local.levels = std::atoi(v);
        if (f == "-LOCAL_SIGMA") o.local.sigma = static_cast<float>(std::atof(v));
        if (f == "-SHARPEN") o.sharpen.strength = static_cast<float>(std::atof(v));
        if (f == "-SHARPEN_LIMIT") o.sharpen.limit = static_cast<float>(std::atof(v));
        if (f == "-GRAIN") o.grain.strength = static_cast<float>(std::atof(v));
        if (f == "-GRAIN_SIZE") o.grain.size = static_cast<float>(std::atof(v));
        if (f == "-DITHER") o.grain.dither = static_cast<float>(std::atof(v));
        if (f == "-GRAIN_SEED") o.grain.seed = static_cast<uint32_t>(std::strtoul(v, nullptr, 10));
        if (f == "-WB") o.wb = v;
        if (f == "-SATURATION") o.saturation = v;
        if (f == "-COLOR_MATRIX") o.colour_matrix = v;
        if (f == "-LUT") o.lut_path = v;
        if (f == "-DISTORTION") o.distortion = v;
        if (f == "-CA") o.ca = v;
        if (f == "-VIGNETTE") o.vignette = v;
        if (f == "-LINEAR_OUT") o.linear_out = v;
        if (f == "-LINEAR_EXPOSED") o.linear_exposed = std::atoi(v);
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

// "m00,..,m22": nine finite numbers, nothing else
bool parse_vec9(const std::string &text, float out[9]) {
    const char *p = text.c_str();
    for (int k = 0; k < 9; ++k) {
        char *end = nullptr;
        out[k] = std::strtof(p, &end);
        if (end == p || !std::isfinite(out[k])) return false;
        if (*end != (k < 8 ? ',' : '\0')) return false;
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

// one number, nothing else -- finite or not: whoever asks judges the value
bool parse_number(const char *text, char stop, float &out, const char **rest) {
    char *end = nullptr;
    out = std::strtof(text, &end);
    if (end == text || *end != stop) return false;
    *rest = end + 1;
    return true;
}

int die(const char *what) {
    std::cerr << what << ": " << pt_last_error() << std::endl;
    return 1;
}

int refuse(int status, const std::string &why) {
    std::cerr << "pt_render: " << why << std::endl;
    return status;
}

// The camera at `eye` looking at `at` under the run's projection: pt_camera_look_at with -FOV, or for ortho pt_camera_ortho with the
// view's height; a fisheye or an equirectangular view takes its angles from the projection, so its camera is made with the default
// -FOV (only the axes' directions matter, and a fisheye's -FOV may exceed what a pinhole can have).
bool view_from(const Options &o, const float eye[3], const float at[3], pt_camera &out) {
    if (o.projection.kind == PT_PROJECTION_ORTHOGRAPHIC) return pt_camera_ortho(eye, at, o.up0, o.view_height, o.aspect, &out) == PT_OK;
    const float fov = o.projection.kind == PT_PROJECTION_PERSPECTIVE ? o.fov : Options().fov;
    return pt_camera_look_at(eye, at, o.up0, fov, o.aspect, &out) == PT_OK;
}

// The camera at time `i` of the sequence, in frames: start + (end - start) i / (n - 1), in double, through pt_camera_look_at.  Frame i
// starts at i and, with -SHUTTER f, ends at i + f (the last frame's end pose lies beyond -EYE_END; with -FRAMES 1 it is EYE + f (EYE_END - EYE)).
bool pose_at(const Options &o, double i, pt_camera &out) {
    float eye[3], at[3];
    for (int k = 0; k < 3; ++k) {
        eye[k] = static_cast<float>(o.eye0[k] + (static_cast<double>(o.eye1[k]) - o.eye0[k]) * i / std::max(1, o.frames - 1));
        at[k] = static_cast<float>(o.at0[k] + (static_cast<double>(o.at1[k]) - o.at0[k]) * i / std::max(1, o.frames - 1));
    }
    return view_from(o, eye, at, out);
}

// PT_RENDER_PRINT_CAMERA with an open shutter: every frame's two poses as the run would set them (no device needed).
bool shutter_poses(Options &o) {
    if (!o.blurring) return true;
    if (!parse_vec3(o.eye, o.eye0) || !parse_vec3(o.lookat, o.at0) || !parse_vec3(o.up, o.up0) ||
        !parse_vec3(o.eye_end.empty() ? o.eye : o.eye_end, o.eye1) || !parse_vec3(o.lookat_end.empty() ? o.lookat : o.lookat_end, o.at1)) {
        std::cerr << "pt_render: -EYE / -EYE_END / -LOOKAT / -LOOKAT_END / -UP take three comma-separated numbers, x,y,z" << std::endl;
        return false;
    }
    for (int i = 0; i < o.frames; ++i)
        for (int e = 0; e < 2; ++e) {
            pt_camera c;
            if (!pose_at(o, i + (e ? static_cast<double>(o.shutter) : 0.0), c)) {
                std::cerr << "pt_render: " << pt_last_error() << std::endl;
                return false;
            }
            std::printf("shutter %d %s", i, e ? "end" : "start");
            const float *rows[4] = {c.origin, c.right, c.up, c.forward};
            for (int k = 0; k < 12; ++k) std::printf(" %.9g", static_cast<double>(rows[k / 3][k % 3]));
            std::printf("\n");
        }
    return true;
}

// Fills `o` from the command line and makes every refusal that needs neither the model nor a device.  Returns -1 to go on,
// else the exit status.  Nothing in here may start the HIP runtime: the model is parsed before the first HIP call, and
// PT_RENDER_PRINT_CONFIG / PT_RENDER_PRINT_CAMERA return before any device call (the CPU tests run them without a device).
int configure(int argc, char **argv, Options &o) {
    parse(argc, argv, o);
    o.rng_seed = o.seed < 0 ? static_cast<unsigned>(std::time(nullptr)) : static_cast<unsigned>(o.seed);
    // -LINEAR_OUT: the extension is the format
    if (!o.linear_out.empty()) {
        const size_t dot = o.linear_out.rfind('.');
        const std::string ext = dot == std::string::npos ? "" : o.linear_out.substr(dot);
        o.linear.format = ext == ".pfm" ? PT_LINEAR_PFM : ext == ".hdr" ? PT_LINEAR_RGBE : 0;
        if (!o.linear.format || dot == 0) return refuse(2, "-LINEAR_OUT takes a file name that ends in .pfm or .hdr");
    }
    if (o.linear_exposed != 0 && o.linear_exposed != 1) return refuse(2, "-LINEAR_EXPOSED takes 0 or 1");
    if (o.linear_exposed && o.linear_out.empty()) return refuse(2, "-LINEAR_EXPOSED needs -LINEAR_OUT");
    o.linear.exposed = o.linear_exposed;
    // with the linear flags the printout waits for every refusal below: the ones that depend on the other flags are among them
    const bool print_config = std::getenv("PT_RENDER_PRINT_CONFIG") != nullptr;
    if (print_config && o.linear_out.empty()) {   // tests/test_ref_parts.py: the parsed Config fields, as the reference's own parser is asked for them
        std::printf("height %d\nwidth %d\nrays_per_pixel %d\nmax_ray_reflections %d\nmedian %d\ngauss %d\neps %.9g\nerror %.9g\nupdate %d\n"
                    "gamma_correction %.9g\nmodel_path %s\nmodel_name %s\nskybox %s\ntime_limit %d\nseed %u\n",
                    o.height, o.width, o.rays_per_pixel, o.max_ray_reflections, o.median, o.gauss, static_cast<double>(o.eps),
                    static_cast<double>(o.error), o.update, static_cast<double>(o.gamma_correction), o.model_path.c_str(),
                    o.model_name.c_str(), o.skybox.c_str(), o.time_limit, o.rng_seed);
        return 0;
    }
    // the camera's vectors, parsed here and nowhere else (without -EYE / -LOOKAT / -UP they are the defaults, which parse)
    const bool vectors = parse_vec3(o.eye, o.eye0) && parse_vec3(o.lookat, o.at0) && parse_vec3(o.up, o.up0);
    // -ENV: an environment or a skybox, not both; its three knobs only with it
    if (!o.env.empty() && !o.skybox.empty()) return refuse(2, "-ENV and -SKYBOX exclude each other: a scene has a skybox or an environment");
    if (o.env.empty() && !(o.env_gain.empty() && o.env_rotate.empty() && o.env_size.empty())) return refuse(2, "-ENV_GAIN, -ENV_ROTATE and -ENV_SIZE need -ENV");
    if (!o.env_gain.empty() && !(parse_float(o.env_gain, o.env_params.gain) && o.env_params.gain >= 0.0f)) return refuse(2, "-ENV_GAIN takes a gain >= 0");
    if (!o.env_rotate.empty() && !parse_float(o.env_rotate, o.env_params.rotate_y_degrees)) return refuse(2, "-ENV_ROTATE takes an angle in degrees");
    if (!o.env_size.empty()) {
        float n = 0.0f;
        if (!(parse_float(o.env_size, n) && n >= 8.0f && n <= 4096.0f && n == static_cast<float>(static_cast<int>(n)))) return refuse(2, "-ENV_SIZE takes a whole number in 8 .. 4096");
        o.env_params.size = static_cast<int32_t>(n);
    }
    // -GLASS: entries m:ior or m:ior:r:g:b, separated by commas; the values' ranges are the library's (pt_hip.h: pt_dielectric)
    for (size_t at = 0; !o.glass_text.empty() && at <= o.glass_text.size();) {
        const size_t comma = std::min(o.glass_text.find(',', at), o.glass_text.size());
        const std::string entry = o.glass_text.substr(at, comma - at);
        at = comma + 1;
        std::vector<std::string> part;
        for (size_t b = 0; b <= entry.size();) {
            const size_t colon = std::min(entry.find(':', b), entry.size());
            part.push_back(entry.substr(b, colon - b));
            b = colon + 1;
        }
        float m = 0.0f;
        pt_dielectric d = {0, 0.0f, {1.0f, 1.0f, 1.0f}};
        bool ok = (part.size() == 2 || part.size() == 5) && parse_float(part[0], m) && m >= 0.0f && m <= 16777216.0f &&
                  m == static_cast<float>(static_cast<int32_t>(m)) && part[0].find_first_not_of("0123456789") == std::string::npos && parse_float(part[1], d.ior);
        for (size_t c = 2; ok && c < part.size(); ++c) ok = parse_float(part[c], d.tint[c - 2]);
        if (!ok) return refuse(2, "-GLASS takes m:ior or m:ior:r:g:b entries separated by commas, not \"" + entry + "\"");
        if (!(d.ior >= 0.125f && d.ior <= 8.0f)) return refuse(2, "-GLASS: ior must lie in 0.125 .. 8, not " + part[1]);
        for (float t : d.tint)
            if (!(t >= 0.0f && t <= 1.0f)) return refuse(2, "-GLASS: a tint component must lie in 0 .. 1 (\"" + entry + "\")");
        d.material = static_cast<int32_t>(m);
        o.glass.push_back(d);
    }
    // -DIRECT 0 | 1
    if (!o.direct_text.empty()) {
        if (o.direct_text != "0" && o.direct_text != "1") return refuse(2, "-DIRECT takes 0 or 1, not \"" + o.direct_text + "\"");
        o.direct = o.direct_text == "1";
    }
    // -DIRECT_ENV 0 | 1 and -DIRECT_ENV_SHARE p: the environment's share of the shadow rays, strictly between 0 and 1
    if (!o.direct_env_text.empty()) {
        if (o.direct_env_text != "0" && o.direct_env_text != "1") return refuse(2, "-DIRECT_ENV takes 0 or 1, not \"" + o.direct_env_text + "\"");
        o.direct_env = o.direct_env_text == "1";
    }
    if (!o.direct_env_share_text.empty()) {
        if (!o.direct_env) return refuse(2, "-DIRECT_ENV_SHARE needs -DIRECT_ENV 1");
        if (!parse_float(o.direct_env_share_text, o.direct_env_share) || !(o.direct_env_share > 0.0f && o.direct_env_share < 1.0f))
            return refuse(2, "-DIRECT_ENV_SHARE takes a number strictly between 0 and 1, not \"" + o.direct_env_share_text + "\"");
    }
    if (o.direct_env && !o.skybox.empty()) return refuse(2, "-DIRECT_ENV samples an environment (-ENV), not a -SKYBOX");
    if (o.direct_env && o.env.empty()) return refuse(2, "-DIRECT_ENV needs -ENV");
    // -RR start[:floor]: start a whole number (0 = a run without the flag), floor in 2^-10 .. 1
    if (!o.rr_text.empty()) {
        const size_t colon = o.rr_text.find(':');
        const std::string start = o.rr_text.substr(0, colon);
        float sv = 0.0f;
        const bool ok = !start.empty() && start.size() <= 7 && start.find_first_not_of("0123456789") == std::string::npos && parse_float(start, sv) &&
                        (colon == std::string::npos || parse_float(o.rr_text.substr(colon + 1), o.rr_floor));
        if (!ok) return refuse(2, "-RR takes start or start:floor (a whole number >= 0 and a number), not \"" + o.rr_text + "\"");
        if (!(o.rr_floor >= 0.0009765625f && o.rr_floor <= 1.0f)) return refuse(2, "-RR: the floor must lie in 2^-10 .. 1, not " + o.rr_text.substr(colon + 1));
        o.rr_start = static_cast<int32_t>(sv);
        if (o.rr_start > 0 && !o.direct && !o.direct_env) return refuse(2, "-RR needs -DIRECT 1 or -DIRECT_ENV 1 (roulette needs their per-path accounting)");
    }
    // -ROUGH: "mtl", or entries m:alpha separated by commas; alpha's range is the library's (pt_hip.h: rough specular)
    if (o.rough_text == "mtl") o.rough_mtl = true;
    for (size_t at = 0; !o.rough_text.empty() && !o.rough_mtl && at <= o.rough_text.size();) {
        const size_t comma = std::min(o.rough_text.find(',', at), o.rough_text.size());
        const std::string entry = o.rough_text.substr(at, comma - at);
        at = comma + 1;
        const size_t colon = entry.find(':');
        float m = 0.0f;
        pt_rough d = {0, 0.0f};
        const std::string index = entry.substr(0, colon);
        const bool ok = colon != std::string::npos && entry.find(':', colon + 1) == std::string::npos && !index.empty() &&
                        index.find_first_not_of("0123456789") == std::string::npos && parse_float(index, m) && m <= 16777216.0f &&
                        m == static_cast<float>(static_cast<int32_t>(m)) && parse_float(entry.substr(colon + 1), d.alpha);
        if (!ok) return refuse(2, "-ROUGH takes mtl or m:alpha entries separated by commas, not \"" + entry + "\"");
        if (!(d.alpha >= PT_ROUGH_ALPHA_MIN && d.alpha <= PT_ROUGH_ALPHA_MAX)) return refuse(2, "-ROUGH: alpha must lie in 2^-10 .. 1, not " + entry.substr(colon + 1));
        d.material = static_cast<int32_t>(m);
        o.rough.push_back(d);
    }
    // -SMOOTH auto | vn, -CREASE degrees
    if (!o.smooth_text.empty()) {
        if (o.smooth_text == "auto") o.smooth = 1;
        else if (o.smooth_text == "vn") o.smooth = 2;
        else return refuse(2, "-SMOOTH takes auto or vn, not \"" + o.smooth_text + "\"");
    }
    if (!o.crease_text.empty()) {
        if (o.smooth != 1) return refuse(2, "-CREASE needs -SMOOTH auto");
        if (!(parse_float(o.crease_text, o.crease) && o.crease >= 0.0f && o.crease <= 180.0f)) return refuse(2, "-CREASE takes an angle in 0 .. 180 degrees");
    }
    // -TEXTURE: "mtl", or entries m:file[:nearest|bilinear] separated by commas (a file name may hold colons, not commas)
    if (o.texture_text == "mtl") o.texture_mtl = true;
    for (size_t at = 0; !o.texture_text.empty() && !o.texture_mtl && at <= o.texture_text.size();) {
        const size_t comma = std::min(o.texture_text.find(',', at), o.texture_text.size());
        const std::string entry = o.texture_text.substr(at, comma - at);
        at = comma + 1;
        const size_t c1 = entry.find(':');
        Options::TextureSpec t = {0, "", PT_TEXTURE_BILINEAR};
        float m = 0.0f;
        bool ok = c1 != std::string::npos && c1 > 0 && entry.find_first_not_of("0123456789") == c1 && parse_float(entry.substr(0, c1), m) && m <= 16777216.0f;
        if (ok) {
            t.file = entry.substr(c1 + 1);
            const size_t c2 = t.file.rfind(':');
            const std::string last = c2 == std::string::npos ? "" : t.file.substr(c2 + 1);
            if (last == "nearest" || last == "bilinear") {
                t.filter = last == "nearest" ? PT_TEXTURE_NEAREST : PT_TEXTURE_BILINEAR;
                t.file.resize(c2);
            }
            ok = !t.file.empty();
        }
        if (!ok) return refuse(2, "-TEXTURE takes mtl or m:file.bmp[:nearest|bilinear] entries separated by commas, not \"" + entry + "\"");
        t.material = static_cast<int32_t>(m);
        o.textures.push_back(t);
    }
    if (!o.texture_gamma_text.empty()) {
        if (o.texture_text.empty()) return refuse(2, "-TEXTURE_GAMMA needs -TEXTURE");
        if (!(parse_float(o.texture_gamma_text, o.texture_gamma) && o.texture_gamma > 0.0f && o.texture_gamma <= 16.0f)) return refuse(2, "-TEXTURE_GAMMA takes a number in (0, 16]");
    }
    // -PROJECTION: the kind by name, its angles from -FOV and -ASPECT; ortho needs a camera of its own (right and up are the view's extent)
    if (o.projection_name == "perspective") o.projection.kind = PT_PROJECTION_PERSPECTIVE;
    else if (o.projection_name == "ortho") o.projection.kind = PT_PROJECTION_ORTHOGRAPHIC;
    else if (o.projection_name == "fisheye") o.projection.kind = PT_PROJECTION_FISHEYE;
    else if (o.projection_name == "equirect") o.projection.kind = PT_PROJECTION_EQUIRECTANGULAR;
    else return refuse(2, "-PROJECTION takes perspective, ortho, fisheye or equirect, not '" + o.projection_name + "'");
    if (!o.ortho_height.empty() && o.projection.kind != PT_PROJECTION_ORTHOGRAPHIC) return refuse(2, "-ORTHO_HEIGHT needs -PROJECTION ortho");
    if (o.projection.kind == PT_PROJECTION_ORTHOGRAPHIC) {
        if (!vectors) return refuse(2, "-EYE / -LOOKAT / -UP take three comma-separated numbers, x,y,z");
        if (!o.ortho_height.empty()) {
            if (!(parse_float(o.ortho_height, o.view_height) && o.view_height > 0.0f)) return refuse(2, "-ORTHO_HEIGHT takes a height > 0");
        } else {   // what the perspective view of -FOV shows at the distance of the point looked at
            double d2 = 0.0;
            for (int i = 0; i < 3; ++i) d2 += (static_cast<double>(o.at0[i]) - o.eye0[i]) * (static_cast<double>(o.at0[i]) - o.eye0[i]);
            o.view_height = static_cast<float>(2.0 * std::tan(static_cast<double>(o.fov) * (M_PI / 360.0)) * std::sqrt(d2));
        }
        o.camera = true;
    } else if (o.projection.kind != PT_PROJECTION_PERSPECTIVE) {
        if (pt_projection_make(o.projection.kind, o.projection.kind == PT_PROJECTION_FISHEYE ? o.fov : 0.0f, o.aspect, &o.projection) != PT_OK) return die("pt_render");
    }
    if (o.camera) {
        if (!vectors) return refuse(2, "-EYE / -LOOKAT / -UP take three comma-separated numbers, x,y,z");
        if (!view_from(o, o.eye0, o.at0, o.view)) return die("pt_render");
    }
    if (o.aperture_given && !(parse_float(o.aperture, o.lens.radius) && o.lens.radius >= 0.0f)) return refuse(2, "-APERTURE takes a radius >= 0");
    if (o.focus_given) {
        if (!(parse_float(o.focus, o.lens.focus_distance) && o.lens.focus_distance > 0.0f)) return refuse(2, "-FOCUS takes a distance > 0");
    } else {   // the distance from the eye to the point looked at: 20 for the reference's camera
        double d2 = 0.0;
        for (int i = 0; i < 3; ++i) d2 += (static_cast<double>(o.at0[i]) - o.eye0[i]) * (static_cast<double>(o.at0[i]) - o.eye0[i]);
        o.lens.focus_distance = static_cast<float>(std::sqrt(d2));
    }
    o.has_lens = o.lens.radius > 0.0f;
    if (!o.shutter_text.empty() && !(parse_float(o.shutter_text, o.shutter) && o.shutter >= 0.0f && o.shutter <= 1.0f))
        return refuse(2, "-SHUTTER takes the open fraction of a frame interval, 0 .. 1");
    const bool travels = !o.eye_end.empty() || !o.lookat_end.empty();
    o.blurring = o.shutter > 0.0f && travels;
    if (!print_config && std::getenv("PT_RENDER_PRINT_CAMERA")) {
        if (!o.camera) {
            std::printf("camera none\n");
        } else {
            const float *rows[4] = {o.view.origin, o.view.right, o.view.up, o.view.forward};
            const char *names[4] = {"origin", "right", "up", "forward"};
            for (int r = 0; r < 4; ++r)
                std::printf("%s %.9g %.9g %.9g\n", names[r], static_cast<double>(rows[r][0]), static_cast<double>(rows[r][1]),
                            static_cast<double>(rows[r][2]));
        }
        if (o.has_lens) std::printf("lens %.9g %.9g\n", static_cast<double>(o.lens.radius), static_cast<double>(o.lens.focus_distance));
        if (o.projection.kind != PT_PROJECTION_PERSPECTIVE)
            std::printf("projection %d %.9g %.9g\n", o.projection.kind, static_cast<double>(o.projection.span_x), static_cast<double>(o.projection.span_y));
        // with -SHUTTER > 0 and a camera that travels: the start and the end pose of every frame, "shutter <frame> start|end <12 numbers>"
        if (!shutter_poses(o)) return 2;
        return 0;
    }
    if (o.width <= 0 || o.height <= 0) return refuse(2, "--W and --H must be positive");
    if (o.scale < 1 || o.scale > PT_UPSAMPLE_MAX_SCALE || o.width % o.scale || o.height % o.scale)
        return refuse(1, "-RENDER_SCALE takes 1, 2, 3 or 4, and --W and --H must be multiples of it");
    o.tw = o.width / o.scale;
    o.th = o.height / o.scale;
    o.upsample.scale = o.scale;
    o.upsample.sigma_plane = o.denoise.sigma_plane;
    o.merging = o.temporal.max_frames > 0.0f;
    o.sequence = o.frames > 1 || o.merging;
    if (o.frames > 1 && o.time_limit != 0) return refuse(2, "-TL is not defined for a sequence (-FRAMES > 1)");
    if (o.frames < 1 || !(o.temporal.max_frames >= 0.0f)) return refuse(2, "-FRAMES takes a count >= 1 and -TEMPORAL a history length >= 0");
    o.display = o.device_resolve != 0;
    if (o.display && (o.gauss || o.median)) {
        std::cerr << "pt_render: -DEVICE_RESOLVE is ignored with -GAUSS / -MEDIAN: they filter the tone-mapped float image, on the host path" << std::endl;
        o.display = false;
    }
    if (o.display && !(std::isfinite(o.gamma_correction) && o.gamma_correction > 0.0f)) {
        std::cerr << "pt_render: -DEVICE_RESOLVE is ignored: it needs a finite -GAMMA > 0" << std::endl;
        o.display = false;
    }
    o.show.gamma = o.gamma_correction;
    o.show.temporal = o.merging ? 1 : 0;
    o.show.temporal_params = o.temporal;
    o.show.denoise = o.denoise;
    // -BLOOM: a stage of the graded chain; alone it runs with the zeroed grade, whose bytes are the ungraded ones.  Checked here
    // and not by a call of the library's device entry point, which would start the HIP runtime.
    if (!(std::isfinite(o.bloom.strength) && o.bloom.strength >= 0.0f) || !(std::isfinite(o.bloom.threshold) && o.bloom.threshold >= 0.0f) ||
        o.bloom.levels < 0 || o.bloom.levels > PT_BLOOM_MAX_LEVELS)
        return refuse(2, "-BLOOM and -BLOOM_THRESHOLD take a number >= 0, -BLOOM_LEVELS 1 .. " + std::to_string(PT_BLOOM_MAX_LEVELS));
    o.blooming = o.bloom.strength > 0.0f;
    // -LOCAL: the same, behind bloom
    if (!(std::isfinite(o.local.strength) && o.local.strength >= 0.0f) || !(std::isfinite(o.local.pivot) && o.local.pivot >= 0.0f) ||
        !(std::isfinite(o.local.sigma) && o.local.sigma >= 0.0f) || o.local.levels < 0 || o.local.levels > PT_LOCAL_MAX_LEVELS)
        return refuse(2, "-LOCAL, -LOCAL_PIVOT and -LOCAL_SIGMA take a number >= 0, -LOCAL_LEVELS 1 .. " + std::to_string(PT_LOCAL_MAX_LEVELS));
    o.localising = o.local.strength > 0.0f;
    // -SHARPEN: the same, behind local exposure
    if (!(std::isfinite(o.sharpen.strength) && o.sharpen.strength >= 0.0f && o.sharpen.strength <= 1.0f) ||
        !(std::isfinite(o.sharpen.limit) && o.sharpen.limit >= 0.0f && o.sharpen.limit <= 0.1875f))
        return refuse(2, "-SHARPEN takes a number in 0 .. 1, -SHARPEN_LIMIT a number in 0 .. 0.1875");
    o.sharpening = o.sharpen.strength > 0.0f;
    // -GRAIN / -DITHER: the same, at the chain's end
    if (!(std::isfinite(o.grain.strength) && o.grain.strength >= 0.0f && o.grain.strength <= 1.0f) ||
        !(std::isfinite(o.grain.size) && (o.grain.size == 0.0f || (o.grain.size >= 1.0f && o.grain.size <= 8.0f))) ||
        !(std::isfinite(o.grain.dither) && o.grain.dither >= 0.0f && o.grain.dither <= 1.0f))
        return refuse(2, "-GRAIN and -DITHER take a number in 0 .. 1, -GRAIN_SIZE a number in 1 .. 8");
    o.graining = o.grain.strength > 0.0f || o.grain.dither > 0.0f;
    if (o.graining && (o.gauss || o.median)) return refuse(2, "-GRAIN and -DITHER do not work with -GAUSS / -MEDIAN");
    // -WB / -SATURATION / -COLOR_MATRIX / -LUT: the colour stage, in the grade's place; alone it runs with the zeroed grade too.  The
    // .cube file is read here, by the library's host-only reader.
    if (!o.wb.empty() && !(parse_vec3(o.wb, o.colour.wb) && o.colour.wb[0] >= 0.0f && o.colour.wb[1] >= 0.0f && o.colour.wb[2] >= 0.0f))
        return refuse(2, "-WB takes three comma-separated gains >= 0, r,g,b");
    if (!o.saturation.empty()) {
        if (!(parse_float(o.saturation, o.colour.saturation) && o.colour.saturation >= 0.0f)) return refuse(2, "-SATURATION takes a number >= 0 (0: grey, 1: unchanged)");
        o.colour.saturation_set = 1;
    }
    if (!o.colour_matrix.empty() && !parse_vec9(o.colour_matrix, o.colour.matrix))
        return refuse(2, "-COLOR_MATRIX takes nine comma-separated numbers, m00,m01,m02,m10,..,m22");
    if (!o.lut_path.empty()) {
        if (pt_lut_load_cube(o.lut_path.c_str(), &o.lut) != PT_OK) return die("pt_render: -LUT");
        o.colour.lut = o.lut;
    }
    {
        float m[9];
        if (pt_colour_matrix(&o.colour, m) != PT_OK) return refuse(2, std::string("-WB / -SATURATION / -COLOR_MATRIX (") + pt_last_error() + ")");
        const float identity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        o.colouring = o.lut != nullptr || std::memcmp(m, identity, sizeof m) != 0;
    }
    // -DISTORTION / -CA / -VIGNETTE: the optics stage, ahead of the meter; alone it runs with the zeroed grade too.  The values are
    // the library's to judge: pt_optics_host checks them before it looks at a device, so a call that names none answers for them.
    if (!o.distortion.empty() || !o.ca.empty() || !o.vignette.empty()) {
        const char *rest = nullptr;
        if (!o.distortion.empty() && !(parse_number(o.distortion.c_str(), ',', o.optics.k1, &rest) && parse_number(rest, '\0', o.optics.k2, &rest)))
            return refuse(2, "-DISTORTION takes two comma-separated numbers, k1,k2");
        if (!o.ca.empty() && !parse_number(o.ca.c_str(), '\0', o.optics.ca, &rest)) return refuse(2, "-CA takes a number");
        if (!o.vignette.empty() && !parse_number(o.vignette.c_str(), '\0', o.optics.vignette, &rest)) return refuse(2, "-VIGNETTE takes a number");
        const float one_mean[3] = {0, 0, 0};
        const int32_t one_count = 0;
        float out_mean[3];
        int32_t out_count;
        if (pt_optics_host(-1, 1, 1, one_mean, &one_count, &o.optics, out_mean, &out_count, nullptr) == PT_ERR_INVALID_ARGUMENT)
            return refuse(2, std::string("-DISTORTION / -CA / -VIGNETTE (") + pt_last_error() + ")");
        o.optical = o.optics.k1 != 0.0f || o.optics.k2 != 0.0f || o.optics.ca != 0.0f || o.optics.vignette != 0.0f;
    }
    o.grading = o.tone_flags || o.blooming || o.localising || o.sharpening || o.graining || o.colouring || o.optical;
    // -TONE / -EXPOSURE / -AUTO_EXPOSURE: what every graded image is asked for
    if (o.tone_flags) {
        const char *names[4] = {"reference", "clamp", "reinhard", "aces"};
        o.grade.curve = -1;
        for (int k = 0; k < 4; ++k)
            if (o.tone == names[k]) o.grade.curve = k;
        o.grade.exposure = std::exp2f(o.exposure_stops);
        o.grade.auto_exposure = o.auto_exposure != 0;
        o.grade.percentile = o.percentile; o.grade.key = o.key; o.grade.rate = o.adapt;
        // the library's own check of the block, through an entry point that is host-only: it needs and starts no device
        const uint32_t empty[PT_METER_ENTRIES] = {0};
        float e = 0, target = 0;
        if (pt_exposure_from_histogram(empty, &o.grade, 0, 0.0f, &e, &target) != PT_OK)
            return refuse(2, std::string("-TONE takes reference, clamp, reinhard or aces; -EXPOSURE stops; -KEY, -ADAPT >= 0; -PERCENTILE 1 .. 100 (") +
                                 pt_last_error() + ")");
    }
    if (o.sequence || o.blurring) {
        if (!vectors || !parse_vec3(o.eye_end.empty() ? o.eye : o.eye_end, o.eye1) || !parse_vec3(o.lookat_end.empty() ? o.lookat : o.lookat_end, o.at1))
            return refuse(2, "-EYE / -EYE_END / -LOOKAT / -LOOKAT_END / -UP take three comma-separated numbers, x,y,z");
        o.moving = o.sequence && (o.camera || travels);
    }
    if (o.linear.exposed && !o.grading)
        return refuse(2, "-LINEAR_EXPOSED needs a grade (-TONE, -EXPOSURE, -AUTO_EXPOSURE or a stage that runs with one): without one there is no exposure");
    if (print_config) {   // the reference's fields, then the linear output's
        std::printf("height %d\nwidth %d\nrays_per_pixel %d\nmax_ray_reflections %d\nmedian %d\ngauss %d\neps %.9g\nerror %.9g\nupdate %d\n"
                    "gamma_correction %.9g\nmodel_path %s\nmodel_name %s\nskybox %s\ntime_limit %d\nseed %u\n"
                    "linear_out %s\nlinear_format %s\nlinear_exposed %d\n",
                    o.height, o.width, o.rays_per_pixel, o.max_ray_reflections, o.median, o.gauss, static_cast<double>(o.eps),
                    static_cast<double>(o.error), o.update, static_cast<double>(o.gamma_correction), o.model_path.c_str(),
                    o.model_name.c_str(), o.skybox.c_str(), o.time_limit, o.rng_seed, o.linear_out.c_str(),
                    o.linear.format == PT_LINEAR_PFM ? "pfm" : "hdr", o.linear.exposed);
        return 0;
    }
    return -1;
}

// Row bands -> devices (main.cpp:115,132,141: the reference's split of the rows over its threads).
void choose_devices(Options &o, int n_dev) {
    if (!o.device_names.empty()) {
        for (size_t at = 0; at <= o.device_names.size();) {
            const size_t comma = std::min(o.device_names.find(',', at), o.device_names.size());
            o.devices.push_back(std::atoi(o.device_names.substr(at, comma - at).c_str()));
            at = comma + 1;
        }
    } else if (o.gpus > 0) {
        for (int b = 0; b < o.gpus; ++b) o.devices.push_back(o.rehearse ? b % n_dev : b);
    } else {
        o.devices.push_back(o.device);
    }
}

// What the library is asked for at w x h; the drivers set the pass range
pt_render_params render_params(const Options &o, int w, int h) {
    pt_render_params rp;
    std::memset(&rp, 0, sizeof rp);
    rp.width = w; rp.height = h; rp.row_begin = 0; rp.row_end = h;
    rp.max_ray_reflections = o.max_ray_reflections;
    rp.eps = o.eps; rp.error = o.error; rp.seed = o.rng_seed;
    return rp;
}

// What main() sets up for its driver, and the one teardown
struct Run {
    const Options &o;
    long long start_time = 0;
    pt_scene *scene = nullptr;
    pt_frame *frame = nullptr;
    pt_display *display = nullptr;   // -DEVICE_RESOLVE: the display of the frame
    pt_render_params rp{};
    int n_dev = 0;
    uint32_t frame_index = 0;        // of the image to come in a sequence: the grain's frame
    const char *transport_name = "none";
    clk::time_point t_begin, t_parse, t_hip, t_load;
    double pre_main_s = 0;   // exec + dynamic linking, when the parent told us when it started us
    explicit Run(const Options &options) : o(options) {}
    ~Run() {
        pt_display_destroy(display);
        pt_frame_destroy(frame);
        pt_scene_destroy(scene);
    }
};

// The frame on the host.  Page-locked accumulators: the read-back then runs at PCIe speed without staging copies.  They are
// allocated on first use -- normally while the GPUs are busy with the frame (pinning 116 MB takes 20 ms, which the host has
// nothing else to do with between enqueueing the passes and waiting for them).
struct HostFrame {
    const size_t px;               // of the traced frame
    float *sum = nullptr, *sum2 = nullptr;
    int32_t *count = nullptr;
    std::vector<uint8_t> bgr;      // the traced frame's bytes: previews, the dispersion resolve, the unscaled image
    std::vector<uint8_t> out_bgr;  // -RENDER_SCALE s > 1: the written image
    std::vector<uint8_t> linear;   // -LINEAR_OUT: the body of the written image's linear file
    double alloc_s = 0, read_s = 0;
    explicit HostFrame(const Options &o) : px(static_cast<size_t>(o.tw) * o.th) {
        if (o.scale > 1) out_bgr.resize(3 * static_cast<size_t>(o.width) * o.height);
        linear.resize(pt_linear_bytes(o.width, o.height, o.linear.format));   // (nothing without -LINEAR_OUT)
    }
    HostFrame(const HostFrame &) = delete;
    ~HostFrame() {
        pt_host_free(sum);
        pt_host_free(sum2);
        pt_host_free(count);
    }
    bool ensure() {
        if (sum && sum2 && count) return true;
        const clk::time_point a = clk::now();
        sum = static_cast<float *>(pt_host_alloc(3 * px * sizeof(float)));
        sum2 = static_cast<float *>(pt_host_alloc(3 * px * sizeof(float)));
        count = static_cast<int32_t *>(pt_host_alloc(px * sizeof(int32_t)));
        if (!sum || !sum2 || !count) return false;
        bgr.resize(3 * px);
        alloc_s += secs(a, clk::now());
        return true;
    }
    int read(pt_frame *frame) {   // gathers the bands (one collective) if any changed, waits, copies the frame out
        if (!ensure()) return static_cast<int>(PT_ERR_OUT_OF_MEMORY);
        const clk::time_point a = clk::now();
        const int rc = pt_frame_read(frame, sum, sum2, count);
        read_s += secs(a, clk::now());
        return rc;
    }
    // what the files hold: the traced frame's bytes, or the upsampled image's
    uint8_t *image() { return out_bgr.empty() ? bgr.data() : out_bgr.data(); }
};

// The device path's present: plain, scaled, or either with grading, bloom, local exposure, colour, optics, sharpening or grain
int present(const Run &r, HostFrame &host, pt_display_info *info) {
    const Options &o = r.o;
    const pt_upsample_params *up = o.scale > 1 ? &o.upsample : nullptr;
    if (o.linear.format) {   // one present makes the bytes and the linear body: the history is pushed once
        pt_grain_params grain = o.grain;
        grain.frame = r.frame_index;
        if (o.grading)
            return pt_display_present_linear(r.display, &o.show, up, &o.grade, &o.bloom, &o.local, &o.colour, &o.optics, &o.sharpen, &grain, &o.linear,
                                             host.image(), host.linear.data(), info, nullptr);
        return pt_display_present_linear(r.display, &o.show, up, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &o.linear,
                                         host.image(), host.linear.data(), info, nullptr);
    }
    if (o.graining) {
        pt_grain_params grain = o.grain;
        grain.frame = r.frame_index;
        return pt_display_present_grain(r.display, &o.show, up, &o.grade, &o.bloom, &o.local, &o.colour, &o.optics, &o.sharpen, &grain, host.image(),
                                        info, nullptr);
    }
    if (o.sharpening)
        return pt_display_present_sharpen(r.display, &o.show, up, &o.grade, &o.bloom, &o.local, &o.colour, &o.optics, &o.sharpen, host.image(), info,
                                          nullptr);
    if (o.optical)
        return pt_display_present_optics(r.display, &o.show, up, &o.grade, &o.bloom, &o.local, &o.colour, &o.optics, host.image(), info, nullptr);
    if (o.colouring) return pt_display_present_colour(r.display, &o.show, up, &o.grade, &o.bloom, &o.local, &o.colour, host.image(), info, nullptr);
    if (o.localising) return pt_display_present_local(r.display, &o.show, up, &o.grade, &o.bloom, &o.local, host.image(), info, nullptr);
    if (o.blooming) return pt_display_present_bloom(r.display, &o.show, up, &o.grade, &o.bloom, host.image(), info, nullptr);
    if (o.grading) return pt_display_present_graded(r.display, &o.show, up, &o.grade, host.image(), info, nullptr);
    return up ? pt_display_present_scaled(r.display, &o.show, up, host.image(), info) : pt_display_present(r.display, &o.show, host.image(), info);
}

struct ChainTimes {   // the -TIMING line's figures of the image stages; nonzero only with a stage
    double features_s = 0, denoise_s = 0;
    float denoise_kernel_ms = 0;
};

// The host path: an image's bytes from a frame's accumulators.  It owns what the stages need between frames and calls: the
// scene on the first device (the history's and the feature buffers' handle), cloned on first use and only when a stage asks for
// it; the temporal history; the scratch planes; the exposure of the previous metered frame.
class HostChain {
public:
    HostChain(const Options &options, const pt_scene *base) : o(options), scene(base) {}
    HostChain(const HostChain &) = delete;
    ~HostChain() {
        pt_temporal_destroy(history);
        if (view) pt_scene_destroy(view);
    }
    // a sequence's camera of the frame to come: the view follows the frame
    bool set_camera(const pt_camera &c) {
        camera = c;
        moved = true;
        return !view || pt_scene_set_camera(view, &camera) == PT_OK;
    }
    bool bytes(HostFrame &host, uint32_t frame_index, float dispersion[3], ChainTimes &times);

private:
    bool features(int w, int h) {   // the first hits of the pinhole view at w x h
        const size_t n = static_cast<size_t>(w) * h;
        pos.resize(3 * n); nrm.resize(3 * n); alb.resize(3 * n); hit.resize(n);
        const pt_render_params fp = render_params(o, w, h);
        return pt_render_features_host(view, &fp, hit.data(), nullptr, pos.data(), nrm.data(), alb.data()) == PT_OK;
    }
    const Options &o;
    const pt_scene *scene;
    pt_scene *view = nullptr;
    pt_camera camera;
    bool moved = false;
    pt_temporal *history = nullptr;
    const pt_denoise_params mean_only{};   // levels 0: mean = sum / n, on the host
    std::vector<float> msum, msum2, mean, up_mean, rgb, pos, nrm, alb;
    std::vector<float> lens_mean;
    std::vector<int32_t> mcount, mean_count, up_count, lens_count, hit;
    bool has_exposure = false;
    float last_exposure = 0.0f;
};

// host.sum / sum2 / count -> host.image(), and the dispersion figures of the frame as rendered (they go into the output's name:
// neither the history nor any filter changes them).  Every stage appears once, in the chain's order.
bool HostChain::bytes(HostFrame &host, uint32_t frame_index, float dispersion[3], ChainTimes &times) {
    const int dev = o.devices[0], tw = o.tw, th = o.th;
    const size_t px = host.px;
    const bool denoising = o.denoise.levels > 0, filtering = o.gauss || o.median;
    const bool need_mean = denoising || o.scale > 1 || o.grading || o.linear.format != 0;   // else the reference's resolve does the whole image
    const float *fs = host.sum, *fs2 = host.sum2;
    const int32_t *fc = host.count;
    // The statistics -- and with no stage at all the image: nothing else runs on the plain path.  -GAUSS / -MEDIAN alone, on the
    // frame as rendered, takes them from its own resolve below.
    float *stats = dispersion;
    if (need_mean || o.merging || !filtering) {
        pt_resolve(tw, th, fs, fs2, fc, o.gamma_correction, host.bgr.data(), stats);
        stats = nullptr;
    }
    const clk::time_point t_features = clk::now();
    if ((o.merging || denoising || o.scale > 1) && !view) {
        if (pt_scene_clone_to_device(scene, dev, &view) != PT_OK || (moved && pt_scene_set_camera(view, &camera) != PT_OK)) return false;
    }
    if (o.merging) {   // temporal merge (with -DENOISE the filter runs on the merged frame in the same chain on the device)
        if (!history && pt_temporal_create(view, tw, th, o.eps, &history) != PT_OK) return false;
        msum.resize(3 * px); msum2.resize(3 * px); mcount.resize(px);
        if (denoising) { mean.resize(3 * px); mean_count.resize(px); }
        if (pt_temporal_push_host(history, fs, fs2, fc, &o.temporal, denoising ? &o.denoise : nullptr, msum.data(), msum2.data(), mcount.data(), nullptr,
                                  denoising ? mean.data() : nullptr, denoising ? mean_count.data() : nullptr, nullptr) != PT_OK)
            return false;
        fs = msum.data(); fs2 = msum2.data(); fc = mcount.data();
    } else if (denoising && !features(tw, th)) {   // first-hit features of the traced frame
        return false;
    }
    const clk::time_point t_denoise = clk::now();
    if (!need_mean) {
        // The two cases that need no mean keep the reference's own steps (main.cpp:162-201): the filters act on the tone-mapped
        // float image, then set_pixel with the accumulators' count; a merged frame with nothing else is resolved as it is.
        if (filtering) {
            rgb.resize(3 * px);
            pt_resolve_float(tw, th, fs, fs2, fc, o.gamma_correction, rgb.data(), stats);
            return pt_post_filter_host(dev, tw, th, rgb.data(), o.gauss, o.median) == PT_OK && pt_quantize(tw, th, rgb.data(), fc, host.bgr.data()) == PT_OK;
        }
        return !o.merging || pt_resolve(tw, th, fs, fs2, fc, o.gamma_correction, host.bgr.data(), nullptr) == PT_OK;
    }
    if (!(o.merging && denoising)) {   // denoise, else sum / n (of the frame as rendered or merged)
        mean.resize(3 * px); mean_count.resize(px);
        if (pt_denoise_host(dev, tw, th, fs, fs2, fc, pos.data(), nrm.data(), alb.data(), hit.data(), denoising ? &o.denoise : &mean_only, mean.data(),
                            mean_count.data(), &times.denoise_kernel_ms) != PT_OK)
            return false;
    }
    const clk::time_point t_mean = clk::now();
    int w = tw, h = th;
    const float *m = mean.data();
    const int32_t *n = mean_count.data();
    if (o.scale > 1) {   // upsample: features at the written size from the same view, the traced frame's mean reconstructed there
        w = o.width; h = o.height;
        up_mean.resize(3 * static_cast<size_t>(w) * h); up_count.resize(static_cast<size_t>(w) * h);
        if (!features(w, h) || pt_upsample_host(dev, w, h, m, n, pos.data(), nrm.data(), alb.data(), hit.data(), &o.upsample, up_mean.data(),
                                                up_count.data(), nullptr) != PT_OK)
            return false;
        m = up_mean.data(); n = up_count.data();
    }
    if (o.optical) {   // optics: what follows reads the image the lens delivers, and its count
        lens_mean.resize(3 * static_cast<size_t>(w) * h); lens_count.resize(static_cast<size_t>(w) * h);
        if (pt_optics_host(dev, w, h, m, n, &o.optics, lens_mean.data(), lens_count.data(), nullptr) != PT_OK) return false;
        m = lens_mean.data(); n = lens_count.data();
    }
    rgb.resize(3 * static_cast<size_t>(w) * h);
    float e = o.grade.exposure > 0.0f ? o.grade.exposure : 1.0f;   // (0 = 1, as the library reads it)
    if (o.grading) {   // meter (a sequence's frame starts from the previous frame's exposure), bloom, local exposure, sharpening
        float target = 0.0f;
        if (o.grade.auto_exposure) {
            uint32_t hist[PT_METER_ENTRIES];
            if (pt_meter_host(dev, w, h, m, n, hist, nullptr) != PT_OK ||
                pt_exposure_from_histogram(hist, &o.grade, has_exposure ? 1 : 0, last_exposure, &e, &target) != PT_OK)
                return false;
            has_exposure = true;
            last_exposure = e;
        }
        if (o.blooming) {
            if (pt_bloom_host(dev, w, h, m, n, e, &o.bloom, rgb.data(), nullptr) != PT_OK) return false;
            m = rgb.data();
        }
        if (o.localising) {
            if (pt_local_host(dev, w, h, m, n, e, &o.local, rgb.data(), nullptr) != PT_OK) return false;
            m = rgb.data();
        }
        if (o.sharpening) {
            if (pt_sharpen_host(dev, w, h, m, n, e, &o.sharpen, rgb.data(), nullptr) != PT_OK) return false;
            m = rgb.data();
        }
    }
    // the linear file's body: the mean every stage above left, before the colour stage or the grade sees it
    if (o.linear.format && pt_linear_encode(w, h, m, n, e, &o.linear, host.linear.data()) != PT_OK) return false;
    if (o.grading) {   // colour / grade
        if (o.colouring ? pt_colour_host(w, h, m, n, e, o.grade.curve, &o.colour, rgb.data()) != PT_OK
                        : pt_grade_host(w, h, m, n, e, o.grade.curve, rgb.data()) != PT_OK)
            return false;
        m = rgb.data();
    }
    if (o.graining) {   // grain and dithered quantization, in the last three steps' place
        pt_grain_params grain = o.grain;
        grain.frame = frame_index;
        if (pt_grain_quantize(w, h, m, n, o.gamma_correction, &grain, host.image()) != PT_OK) return false;
    } else {
        pt_tonemap(w, h, m, n, o.gamma_correction, rgb.data());
        if (filtering && pt_post_filter_host(dev, w, h, rgb.data(), o.gauss, o.median) != PT_OK) return false;
        if (pt_quantize(w, h, rgb.data(), n, host.image()) != PT_OK) return false;
    }
    if (o.scale > 1) {   // the scaled chain is timed as one: the mean, the upsample and what follows it
        times.denoise_s = secs(t_denoise, clk::now());
    } else if (denoising) {   // (the view's clone is part of the features' time)
        times.features_s = secs(t_features, t_denoise);
        times.denoise_s = secs(t_denoise, t_mean);
    }
    return true;
}

// The reference's result name (main.cpp:206-213)
std::string result_name(long long elapsed_ms, int rays_done, int rays_asked, const float dispersion[3]) {
    const std::time_t t = std::time(nullptr);
    const std::tm *now = std::localtime(&t);
    return std::to_string(now->tm_year + 1900) + '-' + std::to_string(now->tm_mon + 1) + '-' + std::to_string(now->tm_mday) + '-' +
           std::to_string(now->tm_hour) + '-' + std::to_string(now->tm_min) + '-' + std::to_string(now->tm_sec) + "  " +
           std::to_string(elapsed_ms) + "   " + std::to_string(rays_done) + " of " + std::to_string(rays_asked) +
           "  max_disp " + std::to_string(dispersion[0]) + "  min_disp " + std::to_string(dispersion[1]) + "  aver_disp " + std::to_string(dispersion[2]);
}

// -LINEAR_OUT's picture, under `path`
int write_linear(const Options &o, const std::string &path, const uint8_t *body) {
    return o.linear.format == PT_LINEAR_PFM ? pt_write_pfm(path.c_str(), o.width, o.height, body) : pt_write_hdr(path.c_str(), o.width, o.height, body);
}

// -OUT, or the named file and ../result.bmp, and -LINEAR_OUT's file; the name goes to stdout either way.  Returns the exit status.
int write_outputs(const Options &o, const std::string &name, const uint8_t *image, const uint8_t *linear) {
    int rc = 0;
    if (o.linear.format && write_linear(o, o.linear_out, linear) != PT_OK) rc = die("pt_render");
    if (!o.out.empty()) {
        if (pt_write_bmp(o.out.c_str(), o.width, o.height, image) != PT_OK) rc = die("pt_render");
    } else {
        if (pt_write_bmp((name + ".bmp").c_str(), o.width, o.height, image) != PT_OK) rc = die("pt_render");
        if (pt_write_bmp("../result.bmp", o.width, o.height, image) != PT_OK) rc = die("pt_render");
    }
    std::cout << name << std::endl;
    return rc;
}

// An image's bytes from the frame as it was read back: the host chain, or with -DEVICE_RESOLVE 1 the device's present -- then the
// dispersion figures, where they are wanted, come from the reference's resolve on the host.
bool make_image(Run &r, HostFrame &host, HostChain &chain, bool want_stats, float dispersion[3], ChainTimes &times) {
    const Options &o = r.o;
    if (!r.display) return chain.bytes(host, r.frame_index, dispersion, times);
    if (want_stats) pt_resolve(o.tw, o.th, host.sum, host.sum2, host.count, o.gamma_correction, host.bgr.data(), dispersion);
    const clk::time_point a = clk::now();
    pt_display_info shown;
    if (present(r, host, &shown) != PT_OK) return false;
    if (o.denoise.levels > 0) {
        times.denoise_s = secs(a, clk::now());
        times.denoise_kernel_ms = shown.kernel_ms;
    }
    return true;
}

bool bench_frame(pt_frame *frame, const pt_render_params &rp) {   // zero the accumulators, every pass on every device, the gather
    return pt_frame_clear(frame) == PT_OK && pt_frame_render(frame, &rp, nullptr) == PT_OK && pt_frame_gather(frame) == PT_OK;
}

// -BENCH_STEPS k: k whole frames, and wait for all of it, after w untimed ones; one JSON line on stdout and no image
int run_bench(Run &r) {
    const Options &o = r.o;
    pt_render_params rp = r.rp;
    rp.pass_begin = 0;
    rp.pass_count = o.rays_per_pixel;
    for (int i = 0; i < std::max(o.bench_warmup, 0); ++i)
        if (!bench_frame(r.frame, rp)) return die("pt_render");
    if (pt_frame_wait(r.frame) != PT_OK) return die("pt_render");
    const clk::time_point a = clk::now();
    for (int i = 0; i < o.bench_steps; ++i)
        if (!bench_frame(r.frame, rp)) return die("pt_render");
    if (pt_frame_wait(r.frame) != PT_OK) return die("pt_render");
    const double dt = secs(a, clk::now());
    const double samples = static_cast<double>(o.tw) * o.th * o.rays_per_pixel * o.bench_steps;
    // With more than one band: one more frame, untimed, taken apart -- every band's own kernel time (HIP events on its
    // stream), then, with all kernels done, the gather alone on the host's clock -- so that the first run on several devices
    // says where the time went and not only how long it took.
    std::string diagnosis;
    if (o.devices.size() > 1) {
        pt_render_stats st;
        std::vector<float> band_ms(o.devices.size(), -1.0f);
        if (pt_frame_clear(r.frame) != PT_OK || pt_frame_render(r.frame, &rp, &st) != PT_OK || pt_frame_wait(r.frame) != PT_OK ||
            pt_frame_band_kernel_ms(r.frame, band_ms.data()) != PT_OK)
            return die("pt_render");
        const clk::time_point g0 = clk::now();
        if (pt_frame_gather(r.frame) != PT_OK || pt_frame_wait(r.frame) != PT_OK) return die("pt_render");
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
                samples / dt / 1e6, dt / o.bench_steps * 1e3, o.bench_steps, o.bench_warmup, o.devices.size(), r.n_dev, r.transport_name, o.tw, o.th,
                o.rays_per_pixel, o.max_ray_reflections, static_cast<double>(o.error), diagnosis.c_str());
    return 0;
}

// -FRAMES n / -TEMPORAL: frame i renders its own pass range from its own camera, goes through the chain and is written; the
// last one also takes the usual outputs.  No previews, no -TIMING line.
int run_sequence(Run &r) {
    const Options &o = r.o;
    HostFrame host(o);
    HostChain chain(o, r.scene);
    if (!host.ensure()) return die("pt_render");
    pt_render_params rp = r.rp;
    float dispersion[3] = {0, INFINITY, 0};
    ChainTimes unused;
    for (int i = 0; i < o.frames; ++i) {
        if (o.moving) {
            pt_camera camera, end;
            // (the previous frame's motion goes first: a camera is checked against the motion its handle has)
            if (o.blurring && pt_frame_set_camera_motion(r.frame, nullptr) != PT_OK) return die("pt_render");
            if (!pose_at(o, i, camera) || pt_frame_set_camera(r.frame, &camera) != PT_OK || !chain.set_camera(camera)) return die("pt_render");
            if (o.blurring && (!pose_at(o, i + static_cast<double>(o.shutter), end) || pt_frame_set_camera_motion(r.frame, &end) != PT_OK))
                return die("pt_render");
        }
        rp.pass_begin = i * o.rays_per_pixel;
        rp.pass_count = o.rays_per_pixel;
        r.frame_index = static_cast<uint32_t>(i);
        if (pt_frame_clear(r.frame) != PT_OK || pt_frame_render(r.frame, &rp, nullptr) != PT_OK) return die("pt_render");
        // on the device path only the last frame is also read back, for the statistics in the output's name
        const bool last = i == o.frames - 1;
        if ((!r.display || last) && host.read(r.frame) != PT_OK) return die("pt_render");
        if (!make_image(r, host, chain, last, dispersion, unused)) return die("pt_render");
        if (o.frames > 1) {
            char frame_name[32];
            std::snprintf(frame_name, sizeof frame_name, "frame_%04d.bmp", i);
            if (pt_write_bmp(frame_name, o.width, o.height, host.image()) != PT_OK) return die("pt_render");
            if (o.linear.format) {   // the frame's BMP name with the extension replaced
                std::snprintf(frame_name, sizeof frame_name, "frame_%04d.%s", i, o.linear.format == PT_LINEAR_PFM ? "pfm" : "hdr");
                if (write_linear(o, frame_name, host.linear.data()) != PT_OK) return die("pt_render");
            }
        }
        if (!o.quiet) std::cerr << "frame " << i + 1 << " of " << o.frames << std::endl;
    }
    return write_outputs(o, result_name(now_ms() - r.start_time, o.rays_per_pixel, o.rays_per_pixel, dispersion), host.image(), host.linear.data());
}

// One frame: the pass slices with previews and -TL, then the chain, the outputs and the -TIMING line.
int run_frame(Run &r) {
    const Options &o = r.o;
    HostFrame host(o);
    HostChain chain(o, r.scene);
    pt_render_params rp = r.rp;
    double preview_s = 0;
    // Pass slices end exactly where the reference writes a preview (after every pass p with p % update == 0,
    // main.cpp:144-158) so that previews happen between GPU calls; with a time limit they are also kept short.
    int rays_count = 0;
    double ms_per_pass = 0;   // measured on the previous slice (0 = not yet known)
    while (rays_count < o.rays_per_pixel) {
        const long long elapsed_ms = now_ms() - r.start_time;
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
        if (pt_frame_render(r.frame, &rp, nullptr) != PT_OK) return die("pt_render");
        if (o.time_limit != 0) {   // wait for the slice (without asking for statistics: the statistics-free kernels are the fast ones)
            if (pt_frame_wait(r.frame) != PT_OK) return die("pt_render");
            ms_per_pass = 1e3 * secs(a, clk::now()) / rp.pass_count;
        }
        for (int p = rays_count; p < slice_end; ++p) {
            if (o.update != 0 && p % o.update == 0) {   // a preview: the traced frame, ungraded, at its own size
                const clk::time_point b = clk::now();
                if (host.read(r.frame) != PT_OK) return die("pt_render");
                pt_resolve(o.tw, o.th, host.sum, host.sum2, host.count, o.gamma_correction, host.bgr.data(), nullptr);
                if (o.out.empty() && pt_write_bmp("../result.bmp", o.tw, o.th, host.bgr.data()) != PT_OK)
                    std::cerr << pt_last_error() << std::endl;   // the reference's save_image only prints, too
                std::cerr << "Image update" << std::endl;
                preview_s += secs(b, clk::now());
            }
            if (!o.quiet) std::cerr << p + 1 << " rays per pixel were sent" << std::endl;
        }
        rays_count = slice_end;
    }
    const clk::time_point t_enqueued = clk::now();
    if (pt_frame_gather(r.frame) != PT_OK) return die("pt_render");   // the frame's one collective (nothing to do for one band)
    const double alloc_before = host.alloc_s;
    if (!host.ensure()) return die("pt_render");                      // (while the devices work)
    const double alloc_in_wait = host.alloc_s - alloc_before;
    if (pt_frame_wait(r.frame) != PT_OK) return die("pt_render");     // the last slice (and, in a fresh process, the
    const clk::time_point t_kernels = clk::now();                      // one-time load of the kernels' code object)
    if (host.read(r.frame) != PT_OK) return die("pt_render");
    const clk::time_point t_render = clk::now();

    float dispersion[3] = {0, INFINITY, 0};
    ChainTimes times;
    if (!make_image(r, host, chain, true, dispersion, times)) return die("pt_render");
    const clk::time_point t_resolve = clk::now();
    const int rc = write_outputs(o, result_name(now_ms() - r.start_time, rays_count, o.rays_per_pixel, dispersion), host.image(), host.linear.data());
    if (o.timing) {
        const clk::time_point t_end = clk::now();
        double host_s[2] = {0, 0};
        pt_scene_timings(r.scene, host_s);
        std::fprintf(stderr, "{\"pre_main_s\": %.4f, \"parse_s\": %.4f, \"hip_startup_s\": %.4f, \"frame_setup_s\": %.4f, \"host_alloc_s\": %.4f, "
                             "\"enqueue_s\": %.4f, \"hierarchy_build_s\": %.4f, \"kernels_wait_s\": %.4f, \"read_back_s\": %.4f, \"previews_s\": %.4f, "
                             "\"resolve_s\": %.4f, \"bmp_write_s\": %.4f, \"main_s\": %.4f, \"bands\": %zu, \"transport\": \"%s\", "
                             "\"features_s\": %.4f, \"denoise_s\": %.4f, \"denoise_kernel_ms\": %.3f}\n",
                     r.pre_main_s, secs(r.t_begin, r.t_parse), secs(r.t_parse, r.t_hip), secs(r.t_hip, r.t_load), alloc_in_wait,
                     secs(r.t_load, t_enqueued) - preview_s, host_s[1], secs(t_enqueued, t_kernels) - alloc_in_wait, secs(t_kernels, t_render), preview_s,
                     secs(t_render, t_resolve), secs(t_resolve, t_end), secs(r.t_begin, t_end), o.devices.size(), r.transport_name, times.features_s,
                     times.denoise_s, static_cast<double>(times.denoise_kernel_ms));
    }
    if (o.fast_exit) {
        // Every file is written and closed; tearing the HIP runtime down (code objects, device heap, RCCL) is all that a normal
        // exit would add.
        std::cout.flush();
        std::cerr.flush();
        std::_Exit(rc);
    }
    return rc;
}

}  // namespace

int main(int argc, char **argv) {
    const long long start_time = now_ms();
    Options o;
    const int refused = configure(argc, argv, o);
    if (refused >= 0) return refused;

    Run r(o);   // (its destructor is the teardown, on every way out but -FASTEXIT's)
    r.start_time = start_time;
    r.t_begin = clk::now();
    if (o.t0_ns > 0) {
        timespec ts;
        clock_gettime(CLOCK_REALTIME, &ts);
        r.pre_main_s = (static_cast<long long>(ts.tv_sec) * 1000000000LL + ts.tv_nsec - o.t0_ns) * 1e-9;
    }
    // The model is parsed before the first HIP call (host-only scene): nothing up to here depends on the device, and nothing up
    // to here may start the HIP runtime.
    if (pt_scene_load_obj_ex(o.model_path.c_str(), o.model_name.c_str(), -1, o.smooth == 2 ? PT_LOAD_GEOMETRIC_PLANES : 0u, &r.scene) != PT_OK) return die("pt_render");
    if (o.smooth != 0) {   // -SMOOTH: the generator's normals, or the file's
        int32_t n_tri = 0, n_mat = 0, has = 0;
        if (pt_scene_counts(r.scene, &n_tri, &n_mat) != PT_OK) return die("pt_render");
        std::vector<float> normals(9 * static_cast<size_t>(n_tri));
        if (o.smooth == 1) {
            std::vector<float> tri(14 * static_cast<size_t>(n_tri)), vertices(9 * static_cast<size_t>(n_tri));
            std::vector<int32_t> tri_mat(static_cast<size_t>(n_tri));
            if (pt_scene_get_triangles(r.scene, tri.data(), tri_mat.data()) != PT_OK) return die("pt_render");
            for (size_t t = 0; t < static_cast<size_t>(n_tri); ++t) std::copy(&tri[14 * t + 4], &tri[14 * t + 13], &vertices[9 * t]);
            if (pt_smooth_normals(n_tri, vertices.data(), o.crease, normals.data()) != PT_OK) return die("pt_render");
        } else if (pt_scene_get_vertex_normals(r.scene, normals.data(), &has) != PT_OK) {
            return die("pt_render");
        }
        if (n_tri > 0 && pt_scene_set_shading_normals(r.scene, normals.data()) != PT_OK) return refuse(2, std::string("-SMOOTH: ") + pt_last_error());
    }
    if (!o.skybox.empty() && pt_scene_set_skybox_bmp(r.scene, o.skybox.c_str()) != PT_OK) return die("pt_render");   // scene.cpp:20-22
    if (!o.env.empty() && pt_scene_set_environment_file(r.scene, o.env.c_str(), &o.env_params) != PT_OK) return die("pt_render");
    // -GLASS: what only the model can decide -- an index outside it, listed twice, an emissive material -- is refused here, with the library's words
    if (!o.glass.empty() && pt_scene_set_dielectrics(r.scene, o.glass.data(), static_cast<int32_t>(o.glass.size())) != PT_OK) return refuse(2, pt_last_error());
    // -ROUGH: after -GLASS, so that a material in both is refused with the library's words; mtl: the Pr lines of the materials with a glossy lobe
    if (o.rough_mtl) {
        int32_t n_tri = 0, n_mat = 0;
        if (pt_scene_counts(r.scene, &n_tri, &n_mat) != PT_OK) return die("pt_render");
        std::vector<float> pr(static_cast<size_t>(n_mat) + 1), mats(10 * static_cast<size_t>(n_mat) + 1);
        if (pt_scene_get_mtl_roughness(r.scene, pr.data()) != PT_OK || pt_scene_get_materials(r.scene, mats.data()) != PT_OK) return die("pt_render");
        for (int32_t m = 0; m < n_mat; ++m) {
            const float *p = &mats[10 * static_cast<size_t>(m)];   // Kd, Ke, Ks, Ns
            const bool emits = p[3] != 0.0f || p[4] != 0.0f || p[5] != 0.0f, ks = p[6] != 0.0f || p[7] != 0.0f || p[8] != 0.0f;
            if (pr[m] < 0.0f || emits || !ks || p[9] == 0.0f) continue;
            o.rough.push_back({m, std::min(std::max(pr[m], PT_ROUGH_ALPHA_MIN), PT_ROUGH_ALPHA_MAX)});
        }
        if (o.rough.empty()) std::fprintf(stderr, "pt_render: -ROUGH mtl: no material of the model's MTL has a Pr line and a glossy lobe, nothing is rough\n");
    }
    if (!o.rough.empty() && pt_scene_set_roughness(r.scene, o.rough.data(), static_cast<int32_t>(o.rough.size())) != PT_OK) return refuse(2, std::string("-ROUGH: ") + pt_last_error());
    // -TEXTURE: the files are read and the list set here, after -GLASS, so that a material in both is refused with the library's words
    if (o.texture_mtl) {
        int32_t n_tri = 0, n_mat = 0;
        if (pt_scene_counts(r.scene, &n_tri, &n_mat) != PT_OK) return die("pt_render");
        for (int32_t m = 0; m < n_mat; ++m) {
            const char *name = "";
            if (pt_scene_get_map_kd(r.scene, m, &name) != PT_OK) return die("pt_render");
            if (*name) o.textures.push_back({m, o.model_path + name, PT_TEXTURE_BILINEAR});
        }
        if (o.textures.empty()) std::fprintf(stderr, "pt_render: -TEXTURE mtl: the model's MTL has no map_Kd line, nothing is textured\n");
    }
    if (!o.textures.empty()) {
        std::vector<std::vector<float>> texels(o.textures.size());
        std::vector<pt_texture> list;
        for (size_t i = 0; i < o.textures.size(); ++i) {
            int32_t w = 0, h = 0;
            if (pt_texture_load_bmp(o.textures[i].file.c_str(), o.texture_gamma, &w, &h, nullptr) != PT_OK) return refuse(2, std::string("-TEXTURE: ") + pt_last_error());
            texels[i].resize(static_cast<size_t>(w) * h * 3);
            if (pt_texture_load_bmp(o.textures[i].file.c_str(), o.texture_gamma, &w, &h, texels[i].data()) != PT_OK) return refuse(2, std::string("-TEXTURE: ") + pt_last_error());
            list.push_back({o.textures[i].material, w, h, o.textures[i].filter, texels[i].data()});
        }
        if (pt_scene_set_textures(r.scene, list.data(), static_cast<int32_t>(list.size())) != PT_OK) return refuse(2, std::string("-TEXTURE: ") + pt_last_error());
    }
    // -DIRECT 1: after -TEXTURE, so that a textured emitter is refused with the library's words, as a model without a light is
    if (o.direct && pt_scene_set_direct_lighting(r.scene, 1) != PT_OK) return refuse(2, std::string("-DIRECT: ") + pt_last_error());
    // -DIRECT_ENV 1: likewise, after -ENV and -TEXTURE
    if (o.direct_env) {
        const pt_env_sampling sampling = {o.direct_env_share};
        if (pt_scene_set_environment_sampling(r.scene, &sampling) != PT_OK) return refuse(2, std::string("-DIRECT_ENV: ") + pt_last_error());
    }
    // -RR: after the two switches it needs
    if (o.rr_start > 0 && pt_scene_set_roulette(r.scene, o.rr_start, o.rr_floor) != PT_OK) return refuse(2, std::string("-RR: ") + pt_last_error());
    if (o.camera && pt_scene_set_camera(r.scene, &o.view) != PT_OK) return die("pt_render");   // the frame's device copies inherit it
    // and its projection -- set before the lens and the motion, which the library refuses on a handle with one, as it refuses the
    // temporal stage when the first frame reaches it: asked here, before any device is looked at, with the library's own words
    if (o.projection.kind != PT_PROJECTION_PERSPECTIVE) {
        if (pt_scene_set_projection(r.scene, &o.projection) != PT_OK) return die("pt_render");
        if (o.merging) return refuse(1, "temporal: the scene handle has a non-perspective projection, which the reprojection does not invert");
    }
    if (o.has_lens && pt_scene_set_lens(r.scene, &o.lens) != PT_OK) return die("pt_render");   // and its lens
    if (o.blurring && (!o.sequence || o.projection.kind != PT_PROJECTION_PERSPECTIVE)) {   // one frame with an open shutter: from -EYE / -LOOKAT towards -EYE_END / -LOOKAT_END
        pt_camera end;
        if (!pose_at(o, static_cast<double>(o.shutter), end) || pt_scene_set_camera_motion(r.scene, &end) != PT_OK) return die("pt_render");
    }
    r.t_parse = clk::now();
    r.n_dev = pt_device_count();   // first HIP call: runtime start-up
    if (r.n_dev < 1) return refuse(1, "no HIP device (the integrator has no CPU fallback)");
    r.t_hip = clk::now();

    choose_devices(o, r.n_dev);
    uint32_t flags = 0;
    if (o.rehearse) flags |= PT_FRAME_REHEARSE;
    if (o.selfcoll) flags |= PT_FRAME_SELF_COLLECTIVE;
    if (pt_frame_create(r.scene, o.devices.data(), static_cast<int32_t>(o.devices.size()), o.tw, o.th, flags, &r.frame) != PT_OK)
        return die("pt_render");
    int32_t transport = 0;
    pt_frame_info(r.frame, nullptr, nullptr, nullptr, &transport);
    r.transport_name = transport == PT_FRAME_TRANSPORT_RCCL ? "rccl" : transport == PT_FRAME_TRANSPORT_DEVICE_COPIES ? "device_copies" : "none";
    if (transport == PT_FRAME_TRANSPORT_DEVICE_COPIES)
        std::cerr << "pt_render: REHEARSAL -- " << o.devices.size() << " row bands on " << r.n_dev << " device(s); the gather is device-to-device "
                     "copies, not the RCCL collective" << std::endl;
    r.t_load = clk::now();
    r.rp = render_params(o, o.tw, o.th);

    if (o.bench_steps > 0) return run_bench(r);
    if (o.display && pt_display_create_frame(r.frame, o.eps, &r.display) != PT_OK) return die("pt_render");
    return o.sequence ? run_sequence(r) : run_frame(r);
}
