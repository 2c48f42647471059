/*
 * pt_hip.h -- C ABI of the MI355X radiance integrator (libpt_hip.so).
 *
 * The reference (Andareon/Path-Tracing) has no plugin/FFI interface; the seam this library cuts is the
 * pass loop of main() (main.cpp:110-160) expressed through the only object interface the reference has:
 *
 *   reference                                                     this ABI
 *   ------------------------------------------------------------  ---------------------------------------
 *   Scene::Scene(color_map&, color2_map&, samples_count&)          pt_scene_create / pt_scene_load_obj
 *     scene.h:17-18, scene.cpp:16-23                                 (accumulators are per-call arguments)
 *   void Scene::LoadModel(std::string)   scene.h:19, scene.cpp:26   pt_scene_load_obj
 *   Ray(begin,dir,depth,coords) + while(ray.IsValid())              pt_render_device / pt_render_host
 *     scene.TraceRay(ray)   main.cpp:116-140, scene.h:23, ray.h:21    (all passes x pixels x segments on the GPU)
 *   dispersion stats + tonemap + set_pixel   main.cpp:162-201       pt_resolve
 *   bitmap_image::save_image   bitmap_image.hpp:431-478             pt_write_bmp
 *   Config fields read by the path   config.h:16-29                 pt_render_params
 *
 * Conventions: plain C types only, caller owns every buffer it passes, every function returns a pt_status
 * (0 = ok) and never throws or exits; pt_last_error() returns the message of the calling thread's last failure.
 * Accumulators are row-major, pixel p = (y - row_begin) * width + x:
 *   sum  [3*p + c]  = sum of contributions        (color_map,     main.cpp:94)
 *   sum2 [3*p + c]  = sum of squared contributions (color2_map,    main.cpp:96)
 *   count[p]        = number of contributing paths (samples_count, main.cpp:98)
 * (the reference's [x][y] nesting is an artefact of vector<vector<>>, not a format).
 * A render call ADDS passes [pass_begin, pass_begin+pass_count) to the buffers it is given, so a frame can be
 * rendered in slices (previews, time limits: main.cpp:111-114,141-158) and an image in row bands (multi-GPU).
 * There is no CPU fallback: without a usable HIP device the render entry points fail with PT_ERR_NO_DEVICE.
 * Threads and streams: a pt_scene may be rendered from several host threads and on several streams.  Launches made through
 * pt_render_device / pt_render_host share the scene's scheduler state and are ordered on the device; every pt_session has
 * its own, so sessions of ONE scene (row bands of an image) run side by side, and launches of different scenes are
 * independent anyway.  Calls on one pt_session / pt_frame are serialised by the caller.  pt_scene_set_skybox_bmp,
 * pt_scene_set_camera, pt_scene_set_lens, pt_scene_set_camera_motion and pt_scene_destroy must not race with a render of the same scene.
 * Several GPUs: pt_frame_* (below) renders one image on the devices of one node from one host program -- row bands, one RCCL
 * group of sends / receives to the root -- the counterpart of the reference's `omp parallel for` over rows, main.cpp:115,132,141.
 */
#ifndef PT_HIP_H
#define PT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 5

typedef enum pt_status {
    PT_OK = 0,
    PT_ERR_INVALID_ARGUMENT = 1,
    PT_ERR_IO = 2,             /* scene.cpp:32-35: the reference prints and exit(1)s */
    PT_ERR_PARSE = 3,          /* malformed OBJ/MTL: undefined behaviour in the reference */
    PT_ERR_NO_DEVICE = 4,
    PT_ERR_HIP = 5,
    PT_ERR_OUT_OF_MEMORY = 6,
    PT_ERR_UNSUPPORTED = 7     /* a valid request this library does not implement (e.g. the reference's serial RNG streams) */
} pt_status;

typedef struct pt_scene pt_scene;   /* immutable after creation */

/* One triangle as the reference stores it (triangles.h:19-25): plane_[4], vertices_[3][3], square. */
#define PT_TRIANGLE_FLOATS 14
/* One material as parsed from the MTL (material.h:22-28): Kd[3], Ke[3], Ks[3], Ns. */
#define PT_MATERIAL_FLOATS 10

typedef struct pt_render_params {
    int32_t width, height;          /* --W / --H       config.h:16-17 */
    int32_t row_begin, row_end;     /* rows [row_begin,row_end) of the image are rendered; buffers hold only them */
    int32_t pass_begin, pass_count; /* passes (samples per pixel) to add: main.cpp:110 */
    int32_t max_ray_reflections;    /* -MRR            config.h:19 (maximum number of path SEGMENTS) */
    float eps;                      /* -EPS            config.h:22 */
    float error;                    /* -ERR            config.h:23 (adaptive sampling threshold; <0 disables) */
    uint32_t seed;                  /* -SEED           config.h:10 */
    int32_t rng_policy;             /* PT_RNG_COUNTER (0, the default of a zeroed struct) or PT_RNG_REFERENCE_STREAM */
    int32_t row_stride;             /* 0 or 1: the band is rows [row_begin, row_end).  n > 1: the band is every n-th TILE ROW of 8 image rows,
                                     * starting with rows row_begin .. row_begin + 7 (row_begin a multiple of 8), as far as they lie below
                                     * row_end; the buffers hold those tile rows packed, 8 rows each (pt_band_rows() rows in all; rows of the
                                     * last tile row at or beyond row_end are left untouched).  The interleaved split of a frame over the
                                     * devices of a node: device k of n takes row_begin = 8 k, row_stride = n, row_end = height -- every
                                     * device then sees the same mix of cheap and expensive rows (pt_frame_* does this itself). */
} pt_render_params;

/* Rows the sum / sum2 / count buffers of a call with these parameters hold: row_end - row_begin, or with a row stride 8 per tile row. */
int32_t pt_band_rows(const pt_render_params *params);

/* Random-number policies.
 * PT_RNG_COUNTER: stateless Philox4x32-10 keyed by (seed, global pixel, pass, segment) -- the policy the device
 *   implements; results are independent of tiling, banding and GPU count.
 * PT_RNG_REFERENCE_STREAM: the reference's two process-wide minstd_rand0 engines consumed in path order
 *   (material.h:16-20, main.cpp:91-92,126-128).  Draw k of the stream belongs to whichever path asks k-th, so every
 *   sample depends on all earlier ones: there is no parallel evaluation order, and the render entry points answer
 *   PT_ERR_UNSUPPORTED.  (The CPU oracle implements it for the reference's recorded md5s; tests/test_gpu_rng_policy.py
 *   states and checks the statistical tolerance between the two policies.) */
#define PT_RNG_COUNTER 0
#define PT_RNG_REFERENCE_STREAM 1

typedef struct pt_render_stats {
    uint64_t samples_traced;        /* primary rays generated (adaptive skips excluded) */
    uint64_t segments;              /* Scene::TraceRay equivalents */
    uint64_t contributing;          /* samples that reached an emitter */
    uint64_t exact_tests;           /* ray-triangle pairs that needed the reference's full arithmetic */
    uint64_t misses;                /* segments that found no triangle */
    uint64_t wave_segments;         /* wave-level: segment-loop iterations summed over wavefronts */
    uint64_t wave_node_rounds;      /* wave-level: rounds of the lane-balanced sphere-tree walk */
    uint64_t wave_exact_iterations; /* wave-level: rounds of the lane-balanced exact tests */
    float kernel_ms;                /* HIP-event time of the integrator kernel on the launch stream; <0 if not timed */
    int32_t n_triangles;
    int32_t n_chunks;               /* pass-range chunks per pixel tile in this launch (each reads + writes the tile once) */
    int32_t partial_commit_rounds;  /* wave-level: tree-walk rounds that could not commit all 64 lanes (queues full) */
    /* Verification build only (libpt_verify.so, -DPT_VERIFY_BRUTE; always 0 from the shipped library): after the culled
     * search every segment's ray is also run through Triangle::Intersect against ALL triangles (scene.cpp:116-120 as
     * written) on the device and the two closest hits are compared. */
    uint64_t verify_checked;        /* segments compared */
    uint64_t verify_mismatches;     /* segments whose (distance bits, triangle index) differed */
} pt_render_stats;

/* ---- scene ---------------------------------------------------------------------------------------- */

/* Parse an OBJ + its MTL with the reference's token-stream semantics (Scene::LoadModel, scene.cpp:26-109) and
 * upload the tables to `device` (HIP ordinal).  device < 0 builds a host-only scene (inspection, no rendering).
 * model_dir is Config::model_path (used as a prefix, e.g. "../models/"), model_name is Config::model_name. */
int pt_scene_load_obj(const char *model_dir, const char *model_name, int device, pt_scene **out);

/* Build a scene from already-prepared tables (same layout pt_scene_get_triangles returns). */
int pt_scene_create(const float *triangles, const int32_t *triangle_material, int32_t n_triangles,
                    const float *materials, int32_t n_materials, int device, pt_scene **out);

/* The same scene on another device (or host-only, device < 0): the parsed model, its tables and the culling hierarchies built
 * so far are SHARED with `scene` (reference-counted; either may be destroyed first), only the device copies are new.  The
 * copy inherits the skybox `scene` has at the time of the call. */
int pt_scene_clone_to_device(const pt_scene *scene, int device, pt_scene **out);

/* -SKYBOX (config.h:26, scene.cpp:20-22): load a 24-bit BMP with bitmap_image::load_bitmap's checks
 * (bitmap_image.hpp:1508-1603) as the scene's skybox; rays that hit nothing then add its bilinear sample to the
 * accumulators (scene.cpp:126-154).  NULL or "" removes the skybox.  Not to be called while a render is in flight.
 * A skybox belongs to the HANDLE it is set on (the reference's Scene holds its own bitmap, scene.h:14): copies made from this
 * handle afterwards (pt_scene_clone_to_device, pt_frame_create) inherit it, other copies of the same model keep theirs.  A
 * failed call leaves the handle's skybox as it was. */
int pt_scene_set_skybox_bmp(pt_scene *scene, const char *path);
/* Width and height of the handle's skybox, 0 x 0 if it has none. */
int pt_scene_skybox_size(const pt_scene *scene, int32_t *width, int32_t *height);

/* ---- camera ---------------------------------------------------------------------------------------- */

/* The view primary rays are made from.  Pixel (x, y) of a W x H image with the pass's jitter (jx, jy) in (-0.5, 0.5) gets
 *   u = (x + jx) / W - 0.5,  v = -(y + jy) / H + 0.5            (in double, then rounded to float: main.cpp:126-128)
 *   d = normalize((u * right + v * up) + forward)               (componentwise in float, nothing fused; glm's normalize)
 * and starts at `origin`.  right and up are not normalised: their lengths are the image's extent at unit distance along
 * forward.  The reference's fixed camera (main.cpp:126-129) is {0,0,-20}, {1,0,0}, {0,1,0}, {0,0,1}: with it every step above is
 * exact and a frame equals the camera-free frame bit for bit.
 * A camera belongs to the scene HANDLE, like the skybox: copies made from it afterwards (pt_scene_clone_to_device,
 * pt_frame_create) inherit it, and a render, session slice or frame slice uses the camera its handle has when the launch is
 * enqueued.  Setting it must not race with a render of the same handle.  Without one (the default) the library renders the
 * reference's view with the reference's own kernels. */
typedef struct pt_camera {
    float origin[3];
    float right[3];
    float up[3];
    float forward[3];
} pt_camera;

/* Largest |component| of a camera origin pt_scene_set_camera accepts for every scene.  The culling margins are derived for
 * origins within max(20, largest |origin component|, largest |vertex coordinate|) + 1 of the world origin; they grow with that
 * radius, and beyond this bound they would stop being meaningful in float arithmetic.  A scene whose own vertices reach farther
 * out (largest |vertex coordinate| > PT_CAMERA_MAX_ORIGIN) accepts origins up to that coordinate as well: they lie inside the
 * envelope the scene has anyway. */
#define PT_CAMERA_MAX_ORIGIN 4096.0f

/* A camera at `eye` looking at `target`, computed in double and rounded to float once:
 *   forward = unit(target - eye);  s = 2 tan(fov_y / 2);  a = aspect > 0 ? aspect : 1
 *   right   = unit(cross(up, forward)) * s * a;   up' = cross(forward, unit(cross(up, forward))) * s
 * aspect = W / H gives square pixels; aspect = 0 keeps the reference's mapping (the full width and the full height span the
 * same angle).  fov_y in degrees, 0 < fov_y < 180.  Fails with PT_ERR_INVALID_ARGUMENT for non-finite input, eye == target or
 * `up` parallel to the view direction.  eye (0,0,-20), target (0,0,0), up (0,1,0), fov_y = 2 atan(0.5) in degrees
 * (53.13010235415598), aspect 0 give exactly the reference camera. */
int pt_camera_look_at(const float eye[3], const float target[3], const float up[3], float fov_y_degrees, float aspect, pt_camera *out);
/* Sets the handle's camera; NULL returns to the reference's fixed camera.  PT_ERR_INVALID_ARGUMENT: a non-finite component, a
 * zero forward, or right / up / forward not linearly independent (|det| <= 1e-6 |right| |up| |forward|).  PT_ERR_UNSUPPORTED:
 * an origin component beyond PT_CAMERA_MAX_ORIGIN and beyond the scene's largest |vertex coordinate|.  A failed call leaves the handle as it was. */
int pt_scene_set_camera(pt_scene *scene, const pt_camera *camera);
/* The handle's camera; *is_set = 0 (and the reference camera in *camera) if it has none.  Either pointer may be NULL. */
int pt_scene_get_camera(const pt_scene *scene, pt_camera *camera, int32_t *is_set);

/* ---- lens (depth of field) ------------------------------------------------------------------------ */

/* A thin lens in front of the camera: primary rays start on a disc of `radius` around the camera origin, in the plane spanned by
 * right and up, and every ray of a pixel passes through the same point of the focal plane -- the plane perpendicular to forward
 * at `focus_distance` from the origin, which is therefore sharp.  With
 *   r^ = right / |right|,  u^ = up / |up|,  f^ = forward / |forward|       (computed in double, rounded to float once)
 * the primary ray of pixel (x, y), pass p, with the Philox words w0..w3 of counter (pixel, p, 0xFFFFFFFF, 0) (w0, w1: the jitter) is
 *   D      = (u * right + v * up) + forward                    (exactly as pt_camera computes it, before normalising)
 *   rho    = radius * sqrt(unit_float(w2));   phi = 2 * 3.141593f * unit_float(w3);   (sn, cs) = portable sin / cos of phi
 *   L_i    = (rho * cs) * r^_i + (rho * sn) * u^_i            (i = x, y, z)
 *   s      = focus_distance / ((D_x f^_x + D_y f^_y) + D_z f^_z)
 *   origin = camera origin + L;   direction = normalize(D * s - L)
 * in float, each operation correctly rounded and nothing fused (unit_float(w) = ((w >> 9) << 1 | 1) * 2^-24; normalize as
 * pt_camera's).  No other random number changes: with the same seed, a frame with a lens and one without draw the same words.
 * A lens belongs to the scene HANDLE, like the camera: copies made from it afterwards (pt_scene_clone_to_device, pt_frame_create)
 * inherit it, and a launch uses the lens its handle has when it is enqueued.  A lens on a handle without a camera applies to the
 * reference camera.  Setting it must not race with a render of the same handle. */
typedef struct pt_lens {
    float radius;           /* aperture radius, in scene units; 0 = a pinhole (no lens) */
    float focus_distance;   /* distance of the focal plane from the camera origin, along forward */
} pt_lens;

/* Sets the handle's lens; NULL or radius == 0 returns to the pinhole.  PT_ERR_INVALID_ARGUMENT: a non-finite value, radius < 0,
 * focus_distance <= 0, or a camera for which D . f^ could reach 0 in the image (|forward| <= |right . f^| + |up . f^|).
 * PT_ERR_UNSUPPORTED: a lens origin could lie beyond PT_CAMERA_MAX_ORIGIN.  pt_scene_set_camera applies the same checks to
 * the lens the handle already has.  A failed call leaves the handle as it was. */
int pt_scene_set_lens(pt_scene *scene, const pt_lens *lens);
/* The handle's lens; *is_set = 0 (and zeros in *lens) if it has none.  Either pointer may be NULL. */
int pt_scene_get_lens(const pt_scene *scene, pt_lens *lens, int32_t *is_set);

/* ---- camera motion (motion blur) ------------------------------------------------------------------ */

/* A camera that moves while the shutter is open: a second pt_camera, the END pose; the START pose is the handle's camera or,
 * without one, the reference's.  Every path draws its own time in the shutter interval and sees the camera interpolated there.
 * With a = start and b = end, each as 12 floats (origin, right, up, forward), the primary ray of pixel (x, y), pass p is
 *   t       = unit_float(w0'),  w0' = word 0 of the Philox counter (pixel, p, 0xFFFFFFFE, 0)   (same key; t in [2^-24, 1))
 *   delta_j = b_j - a_j                                          (one float subtraction per component, on the host)
 *   c_j(t)  = a_j + t * delta_j                                  (one product and one sum in float, nothing fused; j = 0 .. 11)
 * and then everything pt_camera states with c(t) in place of the camera: D = (u * right + v * up) + forward, the origin c_origin(t),
 * normalize as there.  The words w0..w3 of counter (pixel, p, 0xFFFFFFFF, 0) keep their meaning (jitter, lens) and no segment
 * word changes: with the same seed, a frame with motion and one without draw the same numbers for everything else.
 * With a lens, r^, u^, f^ are computed for a and for b exactly as pt_lens states (in double, rounded to float once), their
 * per-component float differences are taken on the host, and the axes are interpolated the same way,
 *   r^_j(t) = r^a_j + t * (r^b_j - r^a_j),   likewise u^ and f^;
 * the pt_lens formulas then run with c(t) and these axes.  The interpolated axes are NOT renormalised: for a rotation of theta
 * within one shutter their length is at least cos(theta / 2) (the chord's midpoint), so the disc shrinks by at most that factor.
 * An end pose equal to the start pose bit for bit is no motion: the handle then launches exactly the kernels it launches without.
 * The motion belongs to the scene HANDLE, like the camera and the lens: copies made from it afterwards (pt_scene_clone_to_device,
 * pt_frame_create) inherit it, and a launch uses the motion its handle has when it is enqueued.  Setting it must not race with a
 * render of the same handle.  First-hit features, the temporal reprojection and every pt_display stage read the START pose and
 * ignore the motion, as they ignore the lens. */

/* Sets the handle's camera motion; NULL (or an end pose equal to the handle's camera bit for bit) removes it.  Checked on the host,
 * in double, so that no t in [0, 1] gives a zero or non-finite D or a zero D . f^:
 *   PT_ERR_INVALID_ARGUMENT  `end` fails a check of pt_scene_set_camera (or, with a lens, of pt_scene_set_lens); or one of the
 *                            eight determinants det(right_X, up_Y, forward_Z), X, Y, Z in {start, end}, has |det| <= 1e-6 |right_X|
 *                            |up_Y| |forward_Z| or a sign other than the rest (det of the interpolated axes is a combination of the
 *                            eight with non-negative weights that sum to 1); or, with a lens, one of the four pairs (X, Y) has
 *                            forward_X . f^_Y <= |right_X . f^_Y| + |up_X . f^_Y| (D(t) . f^(t) is such a combination of them)
 *   PT_ERR_UNSUPPORTED       an origin component of `end` beyond PT_CAMERA_MAX_ORIGIN and the scene's largest |vertex coordinate|,
 *                            or an origin between the poses that could lie beyond the bound: per component the larger of the two
 *                            poses' values (with a lens, of |origin_i| + radius sqrt(r^_i^2 + u^_i^2), each pose with its own axes),
 *                            times 1 + 2^-18 for the rounding of a component that moves or lies in the disc
 * pt_scene_set_camera and pt_scene_set_lens apply the same checks to the motion the handle already has.  A failed call leaves the
 * handle as it was. */
int pt_scene_set_camera_motion(pt_scene *scene, const pt_camera *end);
/* The handle's end pose; *is_set = 0 (and the start pose in *end) if it has no motion.  Either pointer may be NULL. */
int pt_scene_get_camera_motion(const pt_scene *scene, pt_camera *end, int32_t *is_set);

/* ---- projection (orthographic, fisheye, equirectangular) ------------------------------------------- */

/* How a pixel becomes a primary ray.  pt_camera states the perspective projection; the other three kinds change only the primary
 * ray, from the same u, v:
 *   u = float((x + jx) / W - 0.5),  v = float(-(y + jy) / H + 0.5)          (in double, then rounded, as pt_camera forms them)
 * With o, r, p, f = the camera's origin, right, up, forward (on a handle without a camera: the reference camera's) and
 *   r^ = r / |r|,  u^ = p / |p|,  f^ = f / |f|                              (in double, rounded to float once, as pt_lens defines them)
 * everything below is float, each operation rounded to nearest, nothing fused.  normalize3(D) = D * (1 / sqrt((D_x^2 + D_y^2) +
 * D_z^2)) with the correctly rounded root and reciprocal, as for every bounce.  sincos is the portable sine and cosine of the
 * diffuse lobe; its domain is [0, 2 pi], so it is called on |angle| and the sign of the angle is put back on the sine by flipping
 * the sine's sign bit where the angle's is set.
 *   PERSPECTIVE      exactly what pt_camera states, through the same kernels: a handle with kind 0 is a handle without a projection.
 *   ORTHOGRAPHIC     origin_i  = o_i + (u * r_i + v * p_i)                  (i = x, y, z)
 *                    direction = normalize3(f), the same for every pixel
 *                    right and up are the extent of the view in scene units.
 *   FISHEYE          a = u * span_x,  b = v * span_y,  theta = sqrt(a * a + b * b)      (correctly rounded root)
 *                    (sn, cs) = sincos(theta);   k = theta == 0 ? 1 : sn / theta
 *                    D_i = ((k * a) * r^_i + (k * b) * u^_i) + cs * f^_i
 *                    direction = normalize3(D),  origin = o
 *                    Equidistant: the image radius is proportional to the angle from forward.  Angles beyond pi simply wrap; there
 *                    is no mask: a pixel outside the image circle is a ray like any other.
 *   EQUIRECTANGULAR  phi = u * span_x,  psi = v * span_y
 *                    (s_phi, c_phi) = sincos(|phi|) with the sign of phi put back on s_phi; the same for psi
 *                    D_i = ((c_psi * s_phi) * r^_i + s_psi * u^_i) + (c_psi * c_phi) * f^_i
 *                    direction = normalize3(D),  origin = o
 * span_x / span_y are the angles, in radians, the image's width / height cover; kinds 0 and 1 ignore them (pt_scene_get_projection
 * reports them as 0).  The random numbers are those of the pinhole: with the same seed, frames of different kinds draw the same words.
 * First-hit features (pt_render_features_host, and with it the denoiser, the upsampler and every pt_display stage that reads
 * features) use the same formulas with jitter 0.  The temporal reprojection inverts a pinhole: pt_temporal_push_host and a display
 * present with a temporal stage fail with PT_ERR_UNSUPPORTED on a handle with a non-perspective projection.
 * The projection belongs to the scene HANDLE, like the camera: copies made from it afterwards (pt_scene_clone_to_device,
 * pt_frame_create) inherit it, and a launch uses the projection its handle has when it is enqueued.  Setting it must not race with
 * a render of the same handle. */
#define PT_PROJECTION_PERSPECTIVE     0   /* pt_camera's, the default */
#define PT_PROJECTION_ORTHOGRAPHIC    1
#define PT_PROJECTION_FISHEYE         2   /* equidistant: image radius proportional to the angle from forward */
#define PT_PROJECTION_EQUIRECTANGULAR 3
typedef struct pt_projection {
    int32_t kind;
    float span_x;
    float span_y;
} pt_projection;   /* 12 bytes */

/* A projection of `kind` from a field of view, computed in double and rounded to float once.  With rad = fov_y_degrees * (pi / 180)
 * and a = aspect > 0 ? aspect : 1:  FISHEYE: span_y = rad, span_x = rad * a (fov_y_degrees > 0).  EQUIRECTANGULAR: the same, and
 * fov_y_degrees <= 0 means the full sphere, span_x = 2 pi, span_y = pi.  PERSPECTIVE, ORTHOGRAPHIC: both spans 0, the other
 * arguments are ignored.  PT_ERR_INVALID_ARGUMENT: an unknown kind, non-finite input or fov_y_degrees <= 0 for a fisheye (what
 * pt_scene_set_projection refuses is refused there). */
int pt_projection_make(int32_t kind, float fov_y_degrees, float aspect, pt_projection *out);
/* A camera for an orthographic view at `eye` looking at `target`, computed as pt_camera_look_at computes its own with s =
 * view_height: right and up have the lengths view_height * a and view_height (a = aspect > 0 ? aspect : 1), forward is a unit
 * vector.  PT_ERR_INVALID_ARGUMENT as there, and for view_height <= 0. */
int pt_camera_ortho(const float eye[3], const float target[3], const float up[3], float view_height, float aspect, pt_camera *out);
/* Sets the handle's projection; NULL or kind PT_PROJECTION_PERSPECTIVE returns to the pinhole.
 *   PT_ERR_INVALID_ARGUMENT  an unknown kind; for kinds 2 / 3 a span that is not finite or not positive; a fisheye with
 *                            0.5 * sqrt(span_x^2 + span_y^2) > 2 pi (the corner angle leaves the sincos's domain); an equirectangular
 *                            view with span_x > 4 pi or span_y > 4 pi (compared in double)
 *   PT_ERR_UNSUPPORTED       a non-perspective projection on a handle that has a lens (radius > 0) or a camera motion -- and the
 *                            reverse: pt_scene_set_lens / pt_scene_set_camera_motion with a lens / an end pose on a handle with a
 *                            non-perspective projection; clear one of the two first.  An orthographic view with an origin that
 *                            could leave the envelope: max_i(|o_i| + 0.5 (|r_i| + |p_i|)) * (1 + 2^-18) beyond PT_CAMERA_MAX_ORIGIN
 *                            and beyond the scene's largest |vertex coordinate|; pt_scene_set_camera applies the same check against
 *                            the projection the handle already has.
 * A failed call leaves the handle as it was.  (u and v reach 0.5 plus half a pixel at the left and the top edge.  The culling
 * envelope's slack of one scene unit covers that for the orthographic origins as long as |r_i| / W + |p_i| / H <= 1 for i = x, y, z;
 * a render of an image with coarser pixels fails with PT_ERR_UNSUPPORTED.) */
int pt_scene_set_projection(pt_scene *scene, const pt_projection *projection);
/* The handle's projection; *is_set = 0 (and kind 0, spans 0) if it has none.  Either pointer may be NULL. */
int pt_scene_get_projection(const pt_scene *scene, pt_projection *projection, int32_t *is_set);

int pt_scene_counts(const pt_scene *scene, int32_t *n_triangles, int32_t *n_materials);
int pt_scene_get_triangles(const pt_scene *scene, float *triangles, int32_t *triangle_material);
int pt_scene_get_materials(const pt_scene *scene, float *materials);
void pt_scene_destroy(pt_scene *scene);

/* ---- the hot path --------------------------------------------------------------------------------- */

/* d_sum/d_sum2/d_count are DEVICE pointers on the scene's device, sized for the row band (any 4-byte alignment;
 * 16-byte-aligned planes with width % 4 == 0 are written back with 16-byte stores).  The kernel is enqueued on
 * `hip_stream` (a hipStream_t, NULL = the default stream) and the call returns without synchronising unless `stats`
 * is non-NULL (then it waits for the kernel and fills `stats`). */
int pt_render_device(pt_scene *scene, const pt_render_params *params, float *d_sum, float *d_sum2,
                     int32_t *d_count, void *hip_stream, pt_render_stats *stats);

/* Same, with HOST buffers (PCIe-inclusive convenience path): upload, one launch, download; the device band is kept by
 * the scene between calls.  A driver that adds many pass slices to one frame should use a pt_session instead, which
 * moves the accumulators only when it is read. */
int pt_render_host(pt_scene *scene, const pt_render_params *params, float *sum, float *sum2, int32_t *count,
                   pt_render_stats *stats);

/* A render session keeps one row band's accumulators ON THE DEVICE between calls: the progressive driver
 * (main.cpp:110-160: a preview every `update` passes, the -TL check before every pass) adds pass slices with
 * pt_session_render and reads the band back only when it needs a preview or the final image.
 * params->width/height/row_begin/row_end (and row_stride) must equal the session's; pass_begin/pass_count select the slice. */
typedef struct pt_session pt_session;
int pt_session_create(pt_scene *scene, int32_t width, int32_t height, int32_t row_begin, int32_t row_end,
                      pt_session **out);                       /* accumulators start at zero */
/* the same for an interleaved band (pt_render_params::row_stride; 0 / 1 = pt_session_create): params->row_stride must equal it */
int pt_session_create_strided(pt_scene *scene, int32_t width, int32_t height, int32_t row_begin, int32_t row_end, int32_t row_stride,
                              pt_session **out);
int pt_session_render(pt_session *session, const pt_render_params *params, pt_render_stats *stats);
int pt_session_wait(pt_session *session);                                           /* until every slice queued so far is done */
int pt_session_read(pt_session *session, float *sum, float *sum2, int32_t *count);   /* waits, then copies out */
int pt_session_clear(pt_session *session);
void pt_session_destroy(pt_session *session);

/* ---- one image on several GPUs --------------------------------------------------------------------- */

/* The reference splits the image's rows over its OpenMP threads inside the pass loop (main.cpp:115,132,141); a pt_frame splits
 * them over DEVICES: n_bands bands (band b on devices[b]), every band a pt_session on its device.  The split is INTERLEAVED: band
 * b is every n_bands-th tile row of 8 image rows from rows 8 b on (pt_render_params::row_stride), so that every device renders
 * the same mix of cheap and expensive rows -- contiguous bands of the 3840 x 2160 Tor.obj frame cost 67 ... 90 ms in four and
 * 34 ... 46 ms in eight, and a frame is as slow as its slowest band.  (An image with fewer tile rows than bands keeps contiguous
 * bands, which differ by at most one row.)  pt_frame_render enqueues a pass slice on every device before it waits for anything;
 * pt_frame_gather brings the bands' accumulators (28 bytes per pixel) to the root device devices[0] with ONE RCCL group of
 * ncclSend / ncclRecv pairs -- each band's planes in one piece, into a staging buffer on the root, from where three strided device
 * copies per band put the tile rows in place in the root's full-frame planes (contiguous bands are received straight into their
 * rows, and the root's own band renders into the planes directly); pt_frame_read copies the full frame to the host, where the
 * unmodified pt_resolve runs.  The result is bit-identical to the one-device frame for any n_bands (the RNG is keyed by the global
 * pixel index).
 * `scene` is only read (any device, or host-only): the frame makes its own per-device copies, which share the parsed
 * model and the hierarchy.
 * flags: PT_FRAME_REHEARSE -- devices[] may name a device several times (the N-band code path on a one-GPU box); the
 *   gather is then NOT a collective but the same transfers as device-to-device copies (pt_frame_info: transport).
 *   Without it, two bands on one device are refused: nothing falls back silently.
 *   PT_FRAME_SELF_COLLECTIVE -- test aid: ONE band, rendered into a band buffer of its own and gathered to the frame planes
 *   of the same device by an RCCL send / receive to self, so that the collective path can be exercised on one device.
 * librccl.so is loaded on first use, by a frame with the RCCL transport (or pt_rccl_available); a one-band frame never loads it. */
typedef struct pt_frame pt_frame;
#define PT_FRAME_REHEARSE 1u
#define PT_FRAME_SELF_COLLECTIVE 2u
#define PT_FRAME_TRANSPORT_NONE 0            /* one band: it renders into the frame planes */
#define PT_FRAME_TRANSPORT_RCCL 1            /* one group of ncclSend / ncclRecv */
#define PT_FRAME_TRANSPORT_DEVICE_COPIES 2   /* rehearsal: hipMemcpyAsync / hipMemcpyPeerAsync */
int pt_frame_create(const pt_scene *scene, const int32_t *devices, int32_t n_bands, int32_t width, int32_t height,
                    uint32_t flags, pt_frame **out);                                  /* accumulators start at zero */
/* band_rows: 2 per band, [begin, end) (interleaved split: [8 b, height) -- of which the band holds every row_stride-th tile row);
 * band_device: 1 per band; any pointer may be NULL */
int pt_frame_info(const pt_frame *frame, int32_t *n_bands, int32_t *band_rows, int32_t *band_device, int32_t *transport);
/* 1: contiguous bands; n > 1: the interleaved split, band b = tile rows b, b + n, ... */
int pt_frame_row_stride(const pt_frame *frame, int32_t *row_stride);
/* params->width / height must equal the frame's, row_begin / row_end must be 0 / height (the frame owns the split);
 * pass_begin / pass_count select the slice.  Returns without waiting unless stats != NULL (then: sums over the bands,
 * kernel_ms = the slowest band's). */
int pt_frame_render(pt_frame *frame, const pt_render_params *params, pt_render_stats *stats);
/* Diagnosis of a multi-device run: the kernel time of every band (ms[n_bands], HIP events on the band's stream) of the last
 * pt_frame_render that asked for statistics, -1 where there is none.  stats->kernel_ms of that call is the slowest band's. */
int pt_frame_band_kernel_ms(const pt_frame *frame, float *ms);
int pt_frame_gather(pt_frame *frame);   /* enqueue the one collective of the frame; asynchronous */
int pt_frame_wait(pt_frame *frame);     /* until everything enqueued so far -- kernels and gather -- is done */
int pt_frame_read(pt_frame *frame, float *sum, float *sum2, int32_t *count);   /* gathers if a band changed since the last gather, waits, copies out */
int pt_frame_clear(pt_frame *frame);
/* pt_scene_set_camera on every device's copy of the frame's scene (NULL: the reference's camera).  The frame takes the camera
 * of the scene it was created from; this changes it for the slices enqueued afterwards.  Not while a slice is in flight. */
int pt_frame_set_camera(pt_frame *frame, const pt_camera *camera);
/* pt_scene_set_lens on every device's copy of the frame's scene (NULL: no lens), likewise. */
int pt_frame_set_lens(pt_frame *frame, const pt_lens *lens);
/* pt_scene_set_camera_motion on every device's copy of the frame's scene (NULL: no motion), likewise. */
int pt_frame_set_camera_motion(pt_frame *frame, const pt_camera *end);
/* pt_scene_set_projection on every device's copy of the frame's scene (NULL: the pinhole), likewise. */
int pt_frame_set_projection(pt_frame *frame, const pt_projection *projection);
void pt_frame_destroy(pt_frame *frame);
/* Can RCCL be loaded and does it export what the gather calls?  version = ncclGetVersion's.  Needs no GPU. */
int pt_rccl_available(int32_t *version);

/* Closest hit for caller-supplied rays: the triangle loop of Scene::TraceRay (scene.cpp:114-120) on the GPU.
 * origins/directions: 3 floats per ray (HOST buffers).  hit_index[i] = index of the accepted triangle with the
 * smallest distance (lowest index on ties) or -1, hit_t[i] = that distance (+inf on a miss).
 * The culling hierarchy's float-error margins are derived for the rays the integrator itself produces: unit
 * directions (normalised as Ray's constructor does, ray.h:23) and origins with max |component| <= max(20, largest
 * |component of the handle's camera origin|, largest |vertex coordinate|) + 1 (the camera -- the reference's at (0,0,-20)
 * unless pt_scene_set_camera set one --, or a point on a surface; with a lens, max_i(|origin_i| + radius sqrt(r^_i^2 + u^_i^2))
 * plus a rounding allowance instead of the origin; with a camera motion, the larger of the two poses' values).  A ray outside that envelope
 * (| |d|^2 - 1 | > 1e-5, a farther origin) is answered by the reference's own loop over ALL triangles on the
 * device instead, so every finite ray gets the reference's answer; only the speed differs.  A ray with a non-finite
 * component misses (all its distances are NaN, see the deviation below).
 * eps < 0 is allowed and means what it means in the reference: the last test of Triangle::Intersect,
 * abs(..) > eps (triangles.h:68), then rejects every triangle, so every ray misses.
 * Known deviation: a ray lying EXACTLY in a triangle's stored plane makes PlaneIntersect (triangles.h:10-13) return
 * 0/0 = NaN, which passes every comparison of Triangle::Intersect -- the reference then reports that triangle wherever
 * it is.  No geometric cull can follow that; for such a ray this function returns the closest regular hit instead.
 * The integrator cannot produce such rays (DESIGN.md "Known deviation").  The same holds for a triangle whose stored
 * plane is itself NaN (three collinear vertices and no `vn`: normalize(0)): the reference reports it for every ray,
 * this library never does. */
int pt_trace_rays_host(pt_scene *scene, int32_t n_rays, const float *origins, const float *directions, float eps,
                       int32_t *hit_index, float *hit_t);

/* ---- first-hit feature buffers ---------------------------------------------------------------------- */

/* What the camera sees first in every pixel: triangle, distance, position, normal, albedo -- the buffers picking, compositing and
 * a denoiser need.  HOST buffers for rows [row_begin, row_end) of the image (pixel p as above; hit_index / hit_t 1 value per
 * pixel, the others 3 floats); any output pointer may be NULL.  Of `params` width, height, row_begin, row_end, eps and
 * row_stride are used (row_stride 0 / 1 only; n > 1 is PT_ERR_UNSUPPORTED), the pass, seed and other fields are ignored.
 * Pixel (x, y) of a W x H image gets the ray pt_camera states with jitter 0:
 *   u = x / W - 0.5,  v = -y / H + 0.5                          (in double, then rounded to float)
 *   d = normalize((u * right + v * up) + forward)               (componentwise in float, nothing fused; d * (1 / sqrt((x x + y y) + z z)))
 * from `origin`, with the handle's camera or, without one, the reference's.  The handle's LENS IS IGNORED: features are those
 * of the pinhole view and stay sharp.  So is its CAMERA MOTION: features are those of the start pose.  Then
 *   hit_index, hit_t = what pt_trace_rays_host answers for that ray (-1 / +inf on a miss; its known deviation applies)
 *   position         = origin + d * hit_t                       (componentwise in float: one product, one sum)
 *   normal           = the hit triangle's stored plane normal (Triangle::GetNormal, triangles.h: plane_[0..2]; NOT flipped
 *                      towards the viewer)
 *   albedo           = Kd of the hit triangle's material (emitters included: the reference multiplies by Kd there too)
 * and a miss writes zeros to position, normal and albedo. */
int pt_render_features_host(pt_scene *scene, const pt_render_params *params, int32_t *hit_index, float *hit_t, float *position,
                            float *normal, float *albedo);

/* ---- feature-guided denoiser ------------------------------------------------------------------------ */

/* An edge-avoiding a-trous wavelet filter (the spatial half of SVGF, no temporal reuse) on the LINEAR per-pixel mean, guided by
 * the feature buffers above and by the sample variance the accumulators carry.  The chain of a denoised image is
 *   pt_denoise_host -> pt_tonemap -> pt_post_filter_host (optional) -> pt_quantize,  the last three with count_out.
 * All buffers are HOST buffers of the whole width x height image; the kernels run on HIP device `device`.  kernel_ms (may be
 * NULL) = HIP-event time of the kernel chain.  count_out (may be NULL): count, except that a pixel without samples which the
 * filter filled from its neighbours gets 1 -- the count to tone-map and quantize the result with.
 *
 * Parameters; a zeroed struct holds the defaults, except that `levels` says how much is filtered:
 *   levels              a-trous passes, 0 .. 8; 0 = no filtering: mean_rgb = sum / n (sum where n = 0), count_out = count, no
 *                       device and no feature buffer is needed (they may be NULL)
 *   sigma_luminance     s_l; 0 = 4;    sigma_plane  s_p, in scene units; 0 = 0.1    (negative or non-finite: invalid)
 *   normal_power_log2   k; 0 = 7; at most 16    (negative: invalid)
 *   demodulate_albedo   0 or positive = filter radiance divided by the albedo; negative = filter radiance itself
 *
 * The arithmetic, exactly: every operation below is ONE correctly rounded float operation in the order written (+ - * / sqrt,
 * comparisons; nothing fused, no exp / pow / reciprocal approximations), sums run over taps in row-major order (dy outer, dx
 * inner), a tap outside the image is skipped.  lum(c) = (0.2126 c_r + 0.7152 c_g) + 0.0722 c_b.  pos(t) = t > 0 ? t : 0.
 * A pixel has SAMPLES if n = count > 0, is a HIT if hit_index >= 0 (else a miss: it saw the sky), and two pixels are of one
 * CLASS if both are hits or both are misses.
 * 1. Per pixel and channel: m = sum / n;  a = max(albedo, 0.01) if demodulating and a hit (albedo > 0.01 ? albedo : 0.01), else 1;
 *    c = m / a;  v = (pos(sum2 / n - m * m) / n) / (a * a);  var = lum(v).  A pixel without samples has no data: c = 0, var < 0.
 * 2. Feature weight of a tap q for the centre p, f(p, q) = (w_n) * w_p if p is a hit, 1 if it is a miss:
 *      w_n = pos((N_p.x N_q.x + N_p.y N_q.y) + N_p.z N_q.z), squared k times;    e = P_q - P_p;
 *      w_p = 1 / (1 + u * u),  u = |(N_p.x e.x + N_p.y e.y) + N_p.z e.z| / s_p    (distance from the centre's tangent plane)
 * 3. Variance estimate, for every pixel p with samples, over the 7 x 7 window around it (the centre included), using the taps
 *    q of p's class that have samples:  inner 3 x 3 taps, b = (1/4, 1/2, 1/4)_dy * (1/4, 1/2, 1/4)_dx:  G += b * var_q, Gw += b;
 *    all taps, w = 1 * f(p, q), l = lum(c_q):  Mw += w, M1 += w * l, M2 += w * (l * l).   g = G / Gw,  mu = M1 / Mw,
 *    sp = pos(M2 / Mw - mu * mu);   var_p = g if n >= 4, else (g > sp ? g : sp)   (few samples say little about their own
 *    variance -- one sample nothing --, so such a pixel takes at least the spatial variance of its surroundings).
 * 4. Level i = 0 .. levels - 1, spacing 2^i, from the colours and variances of the previous level, for EVERY pixel p:
 *      l_p = lum(c_p);  den = s_l * sqrt(var_p) + 1e-6;  h = (1/16, 1/4, 3/8, 1/4, 1/16)
 *      with data (var_p >= 0): W = 9/64, V = (9/64 * 9/64) * var_p;  without: W = 0, V = 0, var_p read as 0;   S = (0, 0, 0)
 *      for the 24 taps q = p + 2^i (dx, dy) other than the centre that have data and are of p's class:
 *        w = (h_dy * h_dx);  if p is a hit: w = (w * w_n) * w_p;  if p has data: t = (l_p - lum(c_q)) / den, w = w * (1 / (1 + t * t))
 *        W += w;  S += w * (c_q - c_p);  V += (w * w) * var_q
 *      if W > 1e-4:  c_p' = c_p + S / W,  var_p' = V / (W * W)  (a pixel without data has data from here on: it is FILLED);
 *      else p is left as it is.
 * 5. mean_rgb = pos(m + a * (c - c_0)) for a pixel with samples (c_0 = its c of step 1: what the filter did not change comes
 *    back exactly), pos(a * c) for a filled pixel, sum for a pixel that has neither samples nor data. */
typedef struct pt_denoise_params {
    int32_t levels;
    float sigma_luminance, sigma_plane;
    int32_t normal_power_log2;
    int32_t demodulate_albedo;
} pt_denoise_params;
#define PT_DENOISE_MAX_LEVELS 8
/* PT_ERR_INVALID_ARGUMENT: a NULL buffer (sum, sum2, count, params, mean_rgb; the feature buffers if levels > 0), an empty image,
 * a parameter outside what is stated above.  PT_ERR_NO_DEVICE: levels > 0 and `device` is not a usable HIP device (there is no
 * CPU fallback). */
int pt_denoise_host(int device, int32_t width, int32_t height, const float *sum, const float *sum2, const int32_t *count,
                    const float *position, const float *normal, const float *albedo, const int32_t *hit_index,
                    const pt_denoise_params *params, float *mean_rgb, int32_t *count_out, float *kernel_ms);

/* ---- reduced-resolution rendering: feature-guided upsampling ----------------------------------------- */

/* Radiance is what costs: hundreds of path segments per pixel against ONE primary ray for the first-hit features.  So a frame may
 * be traced at (W / s) x (H / s) and shown at W x H: the low-resolution LINEAR mean (what pt_denoise_host returns, or sum / n) is
 * reconstructed at full resolution by a joint bilateral upsample that follows the full-resolution features -- edges and material
 * boundaries stay at output resolution.  The chain of such an image is
 *   pt_denoise_host (or the plain mean) at w x h -> pt_render_features_host at W x H -> pt_upsample_host -> pt_tonemap ->
 *   pt_post_filter_host (optional) -> pt_quantize,  the last three at W x H with count_out.
 * width x height is the OUTPUT size W x H; both must be multiples of s = scale, and w = W / s, h = H / s.  mean_lo (3 floats per
 * pixel) and count_lo are HOST buffers of the w x h image, the feature buffers, mean_rgb and count_out (may be NULL) HOST buffers of
 * the W x H image; the kernels run on HIP device `device`.  kernel_ms (may be NULL) = HIP-event time of the kernel chain.
 *
 * Parameters; a zeroed struct holds the defaults, except that `scale` must be given:
 *   scale               s: 2, 3 or 4
 *   sigma_plane         s_p, in scene units; 0 = 0.1, as the denoiser's    (negative or non-finite: invalid)
 *   normal_power_log2   k; 0 = 7; at most 16    (negative: invalid)
 *   demodulate_albedo   0 or positive = interpolate radiance divided by the albedo; negative = radiance itself
 *
 * The arithmetic, exactly, as for the denoiser: every operation below is ONE correctly rounded float operation in the order
 * written (+ - * /, floor, comparisons, int -> float conversions; nothing fused, no approximations).  lum, pos, HIT / MISS, CLASS and
 * the feature weight f(p, .) = (w_n) * w_p are exactly what pt_denoise_host defines, with s_p = sigma_plane, k = normal_power_log2.
 * Integer divisions truncate.
 * 1. Guide of a low pixel.  The guide of the low pixel Q = (X, Y) is the full-resolution pixel g(Q) = (s X + s / 2, s Y + s / 2); it
 *    always lies inside the image.  Q has DATA if count_lo[Q] > 0.  Per channel a_Q = max(albedo, 0.01) of g(Q) if demodulating and
 *    g(Q) is a hit (albedo > 0.01 ? albedo : 0.01), else 1;  c_Q = m_Q / a_Q  (m = mean_lo).
 * 2. Position in the low grid, for the output pixel p = (x, y); a_p is defined likewise from p's own albedo and class.  A low
 *    pixel's footprint is the s x s output pixels it was jittered over, so  fx = float(2 x + 1 - s) / float(2 s),  fy likewise;
 *    X0 = floor(fx), tx = fx - X0, likewise Y0, ty (X0, Y0 may be -1).  The four taps Q = (X0 + i, Y0 + j), i, j in {0, 1}, are
 *    visited j outer, i inner; the tent weight of a tap is  t = (i ? tx : 1 - tx) * (j ? ty : 1 - ty).
 * 3. Which taps are used?  A tap is USED if it lies inside the low image, has data and g(Q) is of p's class.  Its weight is
 *    o = t for a miss p and o = (t * w_n) * w_p for a hit p: f(p, g(Q)) with p's N, P and g(Q)'s N, P.
 * 4. Combination.  The base b is the c of the used tap with the largest o (the first such tap in visiting order: a later tap
 *    replaces it only if its o is greater).  Over the used taps in visiting order, from 0:  Wt += o,  S += o * (c_Q - b).  If
 *    Wt > 1e-4:  c = b + S / Wt,  mean_rgb = pos(a_p * c),  count_out = 1.
 * 5. Fallback, if Wt <= 1e-4 (no tap usable, or only across an edge): R = (x / s, y / s), the low pixel that contains p.  If R has
 *    data: mean_rgb = m_R as it is, count_out = 1; else mean_rgb = 0, count_out = 0.
 * Taking the heaviest tap as the base makes two properties exact: without demodulation a constant low image comes back as that
 * constant bit for bit (every difference c_Q - b is 0), and where every positively weighted tap of a pixel carries one value the
 * pixel gets exactly that value (taps across a fold, whose guide normals are perpendicular to p's, weigh exactly 0). */
typedef struct pt_upsample_params {
    int32_t scale;
    float sigma_plane;
    int32_t normal_power_log2;
    int32_t demodulate_albedo;
} pt_upsample_params;
#define PT_UPSAMPLE_MAX_SCALE 4
/* PT_ERR_INVALID_ARGUMENT: a NULL buffer (mean_lo, count_lo, the feature buffers, params, mean_rgb), an empty image, width or
 * height not a multiple of scale, a parameter outside what is stated above -- all checked BEFORE the device is looked at.
 * PT_ERR_NO_DEVICE: otherwise, if `device` is not a usable HIP device (there is no CPU fallback). */
int pt_upsample_host(int device, int32_t width, int32_t height, const float *mean_lo, const int32_t *count_lo,
                     const float *position, const float *normal, const float *albedo, const int32_t *hit_index,
                     const pt_upsample_params *params, float *mean_rgb, int32_t *count_out, float *kernel_ms);

/* ---- temporal accumulation (moving camera) ----------------------------------------------------------- */

/* The temporal half the denoiser lacks: the frames of ONE view sequence are accumulated by reprojection.  The stage is
 * accumulator to accumulator: a push takes the accumulators of the current frame (sum, sum2, count, as every render entry point
 * fills them; HOST buffers of the whole width x height image, no row bands) and returns accumulators of the same shape to which
 * the reprojected history of the earlier frames has been ADDED -- history is kept as sums and an effective sample count, so a
 * merge is what rendering more passes would have been, weighted by samples and not by a fixed blend factor.  Everything
 * downstream (pt_denoise_host, pt_resolve, pt_tonemap, the post filters) consumes the result unchanged, and the variance the
 * denoiser derives from sum2 / n - m * m shrinks by itself as the history grows.  Frame i of a sequence renders passes
 * [i * RPP, (i + 1) * RPP) with one seed, so that the frames' samples are independent.
 *
 * A pt_temporal belongs to the scene handle it was created for (which must outlive it) and keeps its history on that handle's
 * device.  A push reads the handle's CAMERA AT THE TIME OF THE CALL (the lens and the camera motion are ignored, as for the features), renders the
 * feature buffers of that view on the device exactly as pt_render_features_host states them (eps from the create call), merges,
 * stores the new history and -- if `denoise` is given -- runs the filter of pt_denoise_host on the merged planes and those
 * features, all in one chain on the device: only the accumulators go up and only the requested outputs come down.  kernel_ms =
 * HIP-event time of that chain.  Not to be called while the handle's camera is being set; calls on one pt_temporal are
 * serialised by the library.
 *
 * Parameters; a zeroed struct holds the defaults:
 *   max_frames       cap of the history's age in frames; 0 = 32; +inf = never capped       (negative or NaN: invalid)
 *   sigma_plane      a history tap farther than this from the pixel's tangent plane is rejected, in scene units; 0 = 0.1
 *   min_normal_dot   ... or whose normal agrees less than this; 0 = 0.9; at most 1   (both: negative or non-finite: invalid)
 *
 * The arithmetic, exactly, as for the denoiser: every operation below is ONE correctly rounded float operation in the order
 * written (+ - * /, floor, comparisons, int <-> float conversions; nothing fused, no approximations).  x . y = (x_x y_x + x_y y_y)
 * + x_z y_z.  State per pixel after a push: Hs[3], Hs2[3] (sums), Hn (their effective sample count, a float: exact only below
 * 2^24), HL (the history's age in frames, a float), and the frame's features P' (position), N' (normal) and class (hit / miss, as
 * the denoiser defines it).  Per object: that frame's camera and the rows i0, i1, i2 of the inverse of the matrix whose columns are
 * its right, up, forward -- computed in double from the float components and rounded to float once:  cross(a, b) = (a_y b_z - a_z
 * b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x);  det = (right_x c_x + right_y c_y) + right_z c_z with c = cross(up, forward);
 * i0 = cross(up, forward) / det,  i1 = cross(forward, right) / det,  i2 = cross(right, up) / det.
 * A push with the current camera, features P, N, class and accumulators s, s2, c computes per pixel p = (x, y) a history part
 * h = (h_s[3], h_s2[3], h_n, h_L), or finds that it has NO HISTORY:
 * 1. First frame (after create or reset): no history.
 * 2. Static camera (the current camera equals the history's bit for bit): h = (Hs, Hs2, Hn, HL) of p itself if Hn > 0, else no
 *    history -- no test, no weight: a sequence that does not move is exactly progressive rendering across calls.  Go to 5.
 * 3. Where was this pixel?  e = P - origin' (the history's camera) for a hit; for a miss e = (u * right + v * up) + forward of the
 *    CURRENT camera with u = x / W - 0.5, v = -y / H + 0.5 as pt_render_features_host states them (a direction: the sky is
 *    reprojected by rotation only).  a = i0 . e, b = i1 . e, g = i2 . e.  Unless g > 0: no history.
 *    fx = (a / g + 0.5) * W,  fy = (0.5 - b / g) * H  (W, H as floats; pixel centres sit at integer coordinates, as the feature
 *    rays).  Unless -1 <= fx < W and -1 <= fy < H (false for a NaN; checked before any conversion to an integer): no history.
 *    x0 = floor(fx), tx = fx - x0, likewise y0, ty.  The four taps q = (x0 + i, y0 + j), i, j in {0, 1}, visited j outer, i inner,
 *    weigh w = (i ? tx : 1 - tx) * (j ? ty : 1 - ty).
 * 4. Which taps count?  A tap q is used if it lies inside the image, Hn_q > 0, it is of p's class, and for hits
 *    N . N'_q >= min_normal_dot and |N . (P'_q - P)| <= sigma_plane (a disoccluded or different surface fails the plane test).
 *    Over the used taps, from 0: Wt += w, A_s += w * Hs_q, A_s2 += w * Hs2_q, A_n += w * Hn_q, A_L += w * HL_q.  Unless
 *    Wt > 1e-3: no history.  Else h = A / Wt, component by component -- interpolating sums and counts with the same weights
 *    makes the history's mean the count-weighted mean of the taps.
 * 5. Cap: if h_L > max_frames: k = max_frames / h_L, and h_s, h_s2, h_n, h_L are each multiplied by k.
 * 6. Merge and store.  With history: Hs = s + h_s, Hs2 = s2 + h_s2, Hn = float(c) + h_n, HL = 1 + h_L.  Without: Hs = s,
 *    Hs2 = s2, Hn = float(c), HL = 1.  P', N', the class and the camera become the current ones.
 * 7. Outputs, with an integer count.  With history: n_i = h_n > 0 ? max(1, int(h_n + 0.5)) : 0 (the conversion truncates),
 *    r = float(n_i) / h_n (1 if n_i = 0);  sum_out = s + h_s * r, sum2_out = s2 + h_s2 * r, count_out = c + n_i.  Without:
 *    sum_out = s, sum2_out = s2, count_out = c.  history_frames = HL.  The history's mean and second moment survive the rounding
 *    of its count; with a static camera and no cap r = 1 and count_out is the exact total.
 * With `denoise`: mean_rgb, mean_count are, bit for bit, what pt_denoise_host returns as mean_rgb, count_out for (sum_out,
 * sum2_out, count_out) and the pt_render_features_host buffers of the same view (levels = 0: the unfiltered mean).  Without it
 * they are left untouched. */
typedef struct pt_temporal pt_temporal;          /* the history of ONE view sequence, resident on the scene's device */
typedef struct pt_temporal_params {
    float max_frames;
    float sigma_plane;
    float min_normal_dot;
} pt_temporal_params;
/* PT_ERR_INVALID_ARGUMENT: a NULL scene or `out`, an empty or too large image, eps not a number.  PT_ERR_NO_DEVICE: a host-only
 * scene (there is no CPU fallback).  The history starts empty: the first push is a first frame. */
int pt_temporal_create(pt_scene *scene, int32_t width, int32_t height, float eps, pt_temporal **out);
/* Every output may be NULL.  PT_ERR_INVALID_ARGUMENT: a NULL handle, input buffer or `params`, a parameter outside what is stated
 * above (those of `denoise` as pt_denoise_host checks them).  A failed call leaves the history as it was. */
int pt_temporal_push_host(pt_temporal *t, const float *sum, const float *sum2, const int32_t *count,
                          const pt_temporal_params *params, const pt_denoise_params *denoise /* NULL: none */,
                          float *sum_out, float *sum2_out, int32_t *count_out, float *history_frames,
                          float *mean_rgb, int32_t *mean_count, float *kernel_ms);
int pt_temporal_reset(pt_temporal *t);           /* forget the history; the next push is a first frame */
void pt_temporal_destroy(pt_temporal *t);

/* ---- device-resident display path: accumulators to image bytes ------------------------------------------- */

/* What a preview or a fly-through needs on the host is 3 bytes per pixel.  A pt_display turns the accumulators of a session or a
 * frame into those bytes WHERE THEY LIE: a present runs, as one chain on the device and behind every slice enqueued so far, the
 * first-hit features (if a stage needs them), the temporal merge, the denoiser, then the tone map and quantization, and copies
 * height * width * 3 bytes (top-down rows, B,G,R, as pt_resolve writes them) to the host.  The bytes are DEFINED by the host
 * chain and equal it bit for bit, for every input:
 *   temporal = 0, denoise.levels = 0   pt_resolve(sum, sum2, count, gamma) of pt_session_read / pt_frame_read
 *   temporal = 0, denoise.levels > 0   pt_render_features_host -> pt_denoise_host -> pt_tonemap -> pt_quantize, with count_out
 *   temporal != 0, denoise.levels = 0  pt_temporal_push_host -> pt_resolve of the merged accumulators
 *   temporal != 0, denoise.levels > 0  pt_temporal_push_host with `denoise` -> pt_tonemap -> pt_quantize, with mean_count
 * Every present with temporal != 0 pushes one frame into the display's own history, exactly as one pt_temporal_push_host call
 * would; a failed present leaves the history as it was.  A present reads the handle's camera at the time of the call (the lens
 * and the camera motion are ignored, as for the features); `eps` of the create call is the features'.
 *
 * How the device can equal std::pow: for gamma > 0, L(m) = (int)(pow(m, gamma) * 255.0f) is a non-decreasing step function of
 * m >= 0, so L(m) is the number of thresholds T_k <= m, T_k being the smallest float with L >= k, and the byte is L(m) & 255
 * (levels above 255 wrap: a mean of 2 gives 349 and the byte 93 at the default gamma).  The host tabulates T_1 .. T_K, K <= 4096,
 * from its own pow by bisection (pt_display_table), checks the 64 floats on either side of every threshold and records a DOUBT
 * BAND [lo_k, hi_k) where they disagree with "below: < k, at or above: >= k"; levels no finite float reaches shorten the table.
 * The kernel only compares.  A pixel with a channel that is negative or NaN, at or above the last threshold, or inside a doubt
 * band is DEFERRED: the kernel puts it on a list, the host finishes it with pt_tonemap's and pt_quantize's own arithmetic. */
typedef struct pt_display pt_display;
typedef struct pt_display_params {
    float gamma;                 /* finite and > 0, else PT_ERR_INVALID_ARGUMENT */
    int32_t temporal;            /* 0: no temporal stage; else merge with this display's history */
    pt_temporal_params temporal_params;
    pt_denoise_params denoise;   /* levels = 0: no filter */
} pt_display_params;
typedef struct pt_display_info {
    float kernel_ms;             /* HIP events around the whole chain */
    int32_t deferred_pixels;     /* pixels finished on the host */
    int32_t table_levels;        /* thresholds in use (<= 4096) */
    int32_t doubt_bands;
} pt_display_info;

/* A display of a session that covers the whole image (row_begin 0, row_end = height, row_stride 0 / 1; anything else:
 * PT_ERR_UNSUPPORTED), or of any frame: a present of a frame gathers first if a band changed, as pt_frame_read does, and then works
 * on the root device's full-frame planes with the root copy's camera.  The session / frame must outlive the display; calls on one
 * display and its session / frame are serialised by the caller. */
int pt_display_create(pt_session *session, float eps, pt_display **out);
int pt_display_create_frame(pt_frame *frame, float eps, pt_display **out);
int pt_display_present(pt_display *d, const pt_display_params *p, uint8_t *bgr, pt_display_info *info /* may be NULL */);
/* A present at s times the session's / frame's size (u->scale = s): the accumulators stay w x h = width x height of the display,
 * the image is W x H = s w x s h, bgr holds H * W * 3 bytes.  One chain on the device: the low-resolution features (if a stage needs
 * them), the temporal merge at w x h on the display's own history (the same history pt_display_present uses), the denoiser at
 * w x h, the features at W x H from the same camera, the upsample, then the tone map and quantization at W x H with the same kernel
 * and deferred list, and W * H * 3 bytes to the host.  The bytes are DEFINED by the host chain and equal it bit for bit:
 *   the w x h mean and count of the row of the table above (levels = 0: sum / n and count, of the accumulators or of the merged
 *   ones; levels > 0: mean_rgb, count_out of pt_denoise_host or mean_rgb, mean_count of pt_temporal_push_host)
 *   -> pt_render_features_host at W x H -> pt_upsample_host with *u -> pt_tonemap -> pt_quantize, with the upsample's count_out.
 * *u is checked as pt_upsample_host checks it, before anything is enqueued: a failed call leaves the history as it was. */
int pt_display_present_scaled(pt_display *d, const pt_display_params *p, const pt_upsample_params *u, uint8_t *bgr,
                              pt_display_info *info /* may be NULL */);
int pt_display_reset(pt_display *d);     /* forget the history: the next present with a temporal stage is a first frame (and the
                                          * next metered present of pt_display_present_graded a first one) */
void pt_display_destroy(pt_display *d);

/* The kernel alone, on a host image: the bytes of pt_tonemap -> pt_quantize for (mean_rgb, count), made on HIP device `device`.
 * PT_ERR_NO_DEVICE if that is not a usable device (there is no CPU fallback). */
int pt_display_bytes_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count,
                          float gamma, uint8_t *bgr, pt_display_info *info /* may be NULL */);
/* The table itself (host only, no device).  *levels = K; thresholds, doubt_lo, doubt_hi (each may be NULL: pass all NULL to query
 * K) get K floats: T_k at [k - 1], and the doubt band of level k, empty (lo == hi) where none is needed. */
int pt_display_table(float gamma, int32_t *levels, float *thresholds, float *doubt_lo, float *doubt_hi);

/* ---- display grading: exposure, saturating tone curves, metered auto-exposure ----------------------------- */

/* The reference's last step, byte = (uint8_t)(int)(pow(m, gamma) * 255), wraps above 1 (a mean of 2 is byte 93), has no exposure
 * and cannot adapt.  Grading is one step BEFORE it, on the linear mean: per channel of a pixel with samples
 *   x = m * e,   g = curve(x),
 * and g takes the mean's place in pt_tonemap -> pt_quantize (host) or in the display kernel's table search (device).  The table
 * of pt_display_table is the ungraded one: it depends on gamma alone, never on the curve or the exposure.
 *
 * The arithmetic, exactly, as for the denoiser: every operation below is ONE correctly rounded float operation in the order
 * written (* / + -, comparisons; nothing fused, no approximations), so host and device compute the same g bit for bit.
 *   PT_CURVE_REFERENCE   g = x                      (with e = 1: today's bytes, wrap included)
 *   PT_CURVE_CLAMP       g = x > 1 ? 1 : x
 *   PT_CURVE_REINHARD    g = x / (1 + x)
 *   PT_CURVE_ACES        a = x * ((2.51 * x) + 0.03),  b = (x * ((2.43 * x) + 0.59)) + 0.14,  g = a / b,  g = g > 1 ? 1 : g
 * (the constants are the floats nearest to the decimals written).  NaN, negative and infinite values get no special case: whatever
 * g comes out goes on; on the device a negative or NaN g defers its pixel to the host, as a negative or NaN mean does, and the
 * host finishes it from the pixel's ungraded mean with these same steps.
 *
 * Metering.  The histogram has 129 uint32 counts.  Of every pixel with count != 0:  l = lum(m) = (0.2126 m_r + 0.7152 m_g) + 0.0722 m_b
 * of the UNGRADED linear mean.  If !(l > 0) -- zero, negative, NaN --: hist[128] += 1 ("dark").  Else idx = bits(l) >> 21 (the
 * exponent and two mantissa bits: quarter-octave bins), bin = idx - 444 clamped to 0 .. 127, hist[bin] += 1.  444 = bits(2^-16) >> 21:
 * the bins cover 2^-16 .. 2^16, +inf lands in bin 127, denormals in bin 0; the lower edge of bin b is the float
 * edge(b) = from_bits((b + 444) << 21).  Integer sums do not depend on the order, so the histogram is exact.
 *
 * Exposure from a histogram.  N = hist[0] + .. + hist[127].  If N = 0: e* = e_prev if there is a previous exposure, else 1.
 * Otherwise b_p = the smallest b with 100 * (hist[0] + .. + hist[b]) >= percentile * N (64-bit integers),  e* = key / edge(b_p),
 * e* = e* < e_min ? e_min : (e* > e_max ? e_max : e*).  Without a previous exposure, or if rate >= 1: e = e*.  Otherwise
 * e = e_prev + (e* - e_prev) * rate.
 *
 * Parameters; a zeroed struct holds the defaults (no grading at all: REFERENCE, e = 1, no metering):
 *   curve           PT_CURVE_*                                                       (anything else: invalid)
 *   exposure        the manual e; 0 = 1                                              (negative or non-finite: invalid)
 *   auto_exposure   0: e = exposure.  Else e comes from the meter and `exposure` is checked but not used
 *   percentile      0 = 50; else 1 .. 100                                            (outside: invalid)
 *   key             0 = 0.18       e_min  0 = 2^-8       e_max  0 = 2^8       rate  0 = 1     (negative or non-finite: invalid)
 *   e_min > e_max (after the defaults): invalid. */
#define PT_CURVE_REFERENCE 0
#define PT_CURVE_CLAMP 1
#define PT_CURVE_REINHARD 2
#define PT_CURVE_ACES 3
#define PT_METER_ENTRIES 129
typedef struct pt_grade_params {
    int32_t curve;
    float exposure;
    int32_t auto_exposure;
    int32_t percentile;
    float key, e_min, e_max, rate;
} pt_grade_params;
typedef struct pt_grade_info {
    float exposure;              /* the e that was used */
    float target;                /* e* (a manual exposure: the same as `exposure`) */
    uint32_t metered, dark;      /* N and hist[128] of the metering (a manual exposure: 0, 0) */
} pt_grade_info;

/* Host only, no device: out_rgb = curve(mean_rgb * exposure) per channel for pixels with count != 0, the others keep their
 * value (out_rgb may be mean_rgb).  The chain of a graded image is ... -> pt_grade_host -> pt_tonemap -> pt_quantize.
 * PT_ERR_INVALID_ARGUMENT: a NULL buffer, an empty image, an unknown curve, an exposure that is not finite and > 0 (0 is NOT
 * a default here: the caller passes the e it means). */
int pt_grade_host(int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure, int32_t curve,
                  float *out_rgb);
/* The meter kernel alone, on a host image: hist[0 .. 128] of (mean_rgb, count), made on HIP device `device`; kernel_ms (may be
 * NULL) = HIP-event time of the kernel.  Buffers and sizes are checked BEFORE the device is looked at; PT_ERR_NO_DEVICE if that
 * is not a usable device (there is no CPU fallback). */
int pt_meter_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count,
                  uint32_t *hist /* PT_METER_ENTRIES */, float *kernel_ms);
/* Host only, pure: the rule above.  has_prev != 0: e_prev is the e of the previous metered present.  On PT_ERR_INVALID_ARGUMENT
 * (a NULL pointer, a parameter outside what is stated above) *e and *e_target are not written. */
int pt_exposure_from_histogram(const uint32_t *hist, const pt_grade_params *params, int32_t has_prev, float e_prev, float *e,
                               float *e_target);

/* pt_display_present (u = NULL) or pt_display_present_scaled (u given) with grading: the same chain, and between its last
 * image stage and the display kernel -- if g->auto_exposure -- the meter and the exposure kernel, all on the session's stream
 * with no host synchronisation inside.  The meter sees the linear mean the display kernel is about to read, at the OUTPUT size
 * (after the upsample if u is given).  The bytes are DEFINED by the host chain and equal it bit for bit: the row of the tables
 * above up to the linear mean and count (a row that ends in pt_resolve: mean = sum / n and count, as pt_denoise_host with
 * levels = 0 gives them), then, if automatic, pt_meter_host -> pt_exposure_from_histogram with the display's previous
 * exposure, then pt_grade_host -> pt_tonemap -> pt_quantize.  With curve = REFERENCE, exposure 0 or 1 and no auto-exposure
 * the bytes are those of the ungraded present.
 * The display keeps the e of its last metered present; like the history it advances only after the bytes have reached the host,
 * so a failed present leaves it as it was, and pt_display_reset forgets it: the next metered present is a first one.  A manual
 * present neither reads nor changes it.  *g is checked before anything is enqueued and before the device is looked at. */
int pt_display_present_graded(pt_display *d, const pt_display_params *p, const pt_upsample_params *u /* NULL: not scaled */,
                              const pt_grade_params *g, uint8_t *bgr, pt_display_info *info /* may be NULL */,
                              pt_grade_info *grade_info /* may be NULL */);
/* pt_display_bytes_host with grading: meter (if automatic; has_prev, e_prev as for pt_exposure_from_histogram), exposure and the
 * graded display kernel as one chain on HIP device `device`, on a host image. */
int pt_display_bytes_graded_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count,
                                 float gamma, const pt_grade_params *g, int32_t has_prev, float e_prev, uint8_t *bgr,
                                 pt_display_info *info /* may be NULL */, pt_grade_info *grade_info /* may be NULL */);

/* ---- bloom: bright-pass glare pyramid before the tone curve ------------------------------------------------ */

/* The saturating curves map everything far above 1 to flat white with a hard edge.  Bloom is one stage BEFORE the grade, mean ->
 * mean, on the linear ungraded mean at the output size: the light above a threshold is spread over its neighbourhood and added
 * back, so the picture says how much brighter than white the light is.  It runs after the last image stage and after the meter
 * and the exposure, and before the grade.
 *
 * The arithmetic, exactly: every line below is ONE correctly rounded float operation in the order written; nothing is fused.
 * c(i, n) = min(max(i, 0), n - 1).
 *
 * Inputs.  m = the pixel's linear mean (a chain row that ends in sums: m = sum / (float)n, as the display chain divides), its
 * count, the exposure e (manual or from the meter), and the parameters threshold T, strength S, levels L.
 *
 * Bright pass, at W x H.  t = T / e.  A pixel with count == 0 contributes B = 0.  Otherwise
 *   l = ((0.2126 m_r) + (0.7152 m_g)) + (0.0722 m_b)          (the meter's luminance)
 *   if !(l > t) or !(l <= FLT_MAX):  B = 0 in all channels
 *   else  s = (l - t) / l,  B_c = m_c * s.
 *
 * Down, k = 1 .. L.  D_0 = B;  w_0 = W, h_0 = H, w_k = (w_{k-1} + 1) >> 1, h_k likewise.
 *   horizontal, at the decimated columns only, for X < w_k and y < h_{k-1}:  p_j = D_{k-1}(c(2X + j, w_{k-1}), y), j = -1 .. 2,
 *     G(X, y) = ((p_0 + p_1) * 0.375) + ((p_{-1} + p_2) * 0.125)
 *   vertical, the same formula on G with rows c(2Y + j, h_{k-1}), gives D_k(X, Y).
 * The taps are (1 3 3 1)/8, centred between samples 2X and 2X + 1, so that the up pass below is aligned with it.
 *
 * Up, k = L-1 .. 0.  U_L = D_L;  V_k = up2(U_{k+1}) at w_k x h_k:
 *   horizontal first, with X = x >> 1:
 *     x even:  g = (U(c(X - 1, w_{k+1}), .) * 0.25) + (U(X, .) * 0.75)
 *     x odd:   g = (U(X, .) * 0.75) + (U(c(X + 1, w_{k+1}), .) * 0.25)
 *   then the same rule vertically, on g.
 *   k >= 1:  U_k = D_k + V_k.      k = 0:  A = V_0  (the pixel's own unblurred bright part is already in m).
 *
 * Output.  wgt = S / (float)L, one division on the host, passed by value.  A pixel with count != 0 gets
 *   out_c = m_c + (A_c * wgt);
 * the others keep their value, as pt_grade_host leaves them.  NaN, negative and infinite channels get no special case beyond the
 * two luminance tests: whatever comes out goes on (a NaN or infinite channel of a pixel whose luminance passes both tests spreads
 * over the 2^L-neighbourhood its taps reach; a NaN's payload is not defined).
 *
 * Parameters; a zeroed struct means no bloom:
 *   strength    0: the stage is not run (the bytes are those of pt_display_present_graded)    (negative or non-finite: invalid)
 *   threshold   0 = 1                                                                        (negative or non-finite: invalid)
 *   levels      0 = 5; else 1 .. PT_BLOOM_MAX_LEVELS                                         (outside: invalid)
 * Any image size from 1 x 1 is valid. */
#define PT_BLOOM_MAX_LEVELS 8
typedef struct pt_bloom_params {
    float threshold;
    float strength;
    int32_t levels;
} pt_bloom_params;

/* The bloom kernels alone, on a host image: out_rgb (may be mean_rgb) = the output above for (mean_rgb, count), made on HIP device
 * `device`; kernel_ms (may be NULL) = HIP-event time of the 2 L kernels.  Buffers, sizes, `exposure` (finite and > 0; 0 is NOT a
 * default here, as in pt_grade_host) and *b are checked BEFORE the device is looked at; PT_ERR_NO_DEVICE afterwards if that is
 * not a usable device (there is no CPU fallback).  With strength == 0 it copies. */
int pt_bloom_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure,
                  const pt_bloom_params *b, float *out_rgb, float *kernel_ms);
/* pt_display_present_graded with bloom: the same chain with the bloom kernels between the exposure kernel and the display kernel,
 * on the session's stream with no host synchronisation inside; the bright pass reads e from the device scalar the display kernel
 * reads.  The bytes are DEFINED by the host chain and equal it bit for bit: the row of the tables above up to the linear mean and
 * count, then, if automatic, pt_meter_host -> pt_exposure_from_histogram on the mean BEFORE bloom, then
 * pt_bloom_host(e) -> pt_grade_host(e, curve) -> pt_tonemap -> pt_quantize.  *b is checked with *g, before anything is enqueued; a
 * failed present leaves the history and the previous exposure as they were.  A deferred pixel carries the bloomed ungraded mean
 * the display kernel read, and the host grades that.  With strength == 0 the call is pt_display_present_graded. */
int pt_display_present_bloom(pt_display *d, const pt_display_params *p, const pt_upsample_params *u /* NULL: not scaled */,
                             const pt_grade_params *g, const pt_bloom_params *b, uint8_t *bgr, pt_display_info *info /* may be NULL */,
                             pt_grade_info *grade_info /* may be NULL */);

/* ---- local exposure: edge-aware dodge and burn before the tone curve ---------------------------------------- */

/* One exposure and one curve serve a picture whose parts differ by orders of magnitude badly: the exposure opens for the dark part
 * and the curve flattens the bright one, or the other way round.  Local exposure is one stage BEFORE the grade and AFTER bloom,
 * mean -> mean, on the linear ungraded mean at the output size: every pixel is multiplied by a gain g that depends on a smooth,
 * edge-stopped base of the luminance around it.  Where the base is brighter than the pivot the pixel is pulled down, where it is
 * darker it is lifted; the detail m / base is untouched, because g depends on the base alone.  The meter sees the picture before
 * bloom and before this stage.
 *
 * The arithmetic, exactly: every line below is ONE correctly rounded float operation in the order written (* / + -, comparisons);
 * nothing is fused, and there is no log, exp or pow -- the operator is rational, for the reason the denoiser's weights are.
 *
 * Inputs.  m = the pixel's linear mean (a chain row that ends in sums: m = sum / (float)n, as the display chain divides; with bloom,
 * bloom's output), its count, the exposure e (manual or from the meter), and the parameters strength c, pivot, levels L, sigma.
 *
 * Luminance plane, at W x H.  A pixel with count == 0 is INVALID.  Otherwise
 *   l = ((0.2126 m_r) + (0.7152 m_g)) + (0.0722 m_b)          (the meter's luminance)
 *   if !(l >= 0) or !(l <= 2^64):  INVALID  (negative, NaN, +inf or too large; 2^64 keeps every sum and product below finite)
 *   else  b_0 = l.
 * An invalid pixel is invalid at every level, is never a tap, gets g = 1 and keeps its value, NaN or infinity included.
 *
 * Base, k = 0 .. L-1: one level of the 5 x 5 B3 spline h = (1 4 6 4 1)/16 at tap spacing 2^k, edge-stopped.  For a valid pixel
 * p = (x, y):  sw = 0, sd = 0, and for dy = -2 .. 2, for dx = -2 .. 2 (in that order), q = (x + dx 2^k, y + dy 2^k); a q outside
 * the image or invalid is skipped; otherwise, with bp = b_k(p), bq = b_k(q):
 *   d  = bq - bp
 *   mn = bq < bp ? bq : bp
 *   s  = (sigma * mn) + 1e-30
 *   r  = d / s
 *   wr = 1 / (1 + (r * r))
 *   w  = (h_dy * h_dx) * wr          (h_dy * h_dx is exact: a multiple of 1/256)
 *   sw = sw + w
 *   sd = sd + (w * d)
 * and then  b_{k+1}(p) = bp + (sd / sw).  The centre tap needs no special case: d = 0 gives r = 0 and wr = 1 exactly, so sw >= 36/256.
 * This is the denoiser's form: a constant plane has every d = 0 and stays constant to the bit.  The range term is relative to
 * the SMALLER of the two values: across an edge of ratio R the weight falls like sigma^2 / (R - 1)^2, so what leaks across, weight
 * times difference, shrinks as the edge grows (a term relative to bp + bq would saturate at sigma^2 and leak more the stronger the
 * edge).  Every b_k is a weighted mean of values in 0 .. 2^64 in which the pixel's own value has at least 36/256 of the weight, so
 * it stays finite and never falls below zero (the kernels mark an invalid pixel by a negative value in the plane of b_k and rely
 * on that), and no step gives inf - inf, inf / inf or 0 / 0: an r beyond FLT_MAX is +-inf, its wr is 0.
 *
 * Gain and output.  A valid pixel gets
 *   a = b_L * e
 *   g = (1 + c) / (1 + ((c * a) / pivot))
 *   out_ch = m_ch * g          per channel;
 * the others keep their value, as pt_grade_host leaves them.  g = 1 where the exposed base equals the pivot, at most 1 + c (a
 * black base), and falls with the base: a bright region is pulled towards pivot (1 + c) / c.
 *
 * Parameters; a zeroed struct means the stage does not run:
 *   strength    c; 0: the stage is not run (the bytes are those of pt_display_present_bloom)   (negative or non-finite: invalid)
 *   pivot       0 = 0.18                                                                       (negative or non-finite: invalid)
 *   levels      0 = 5; else 1 .. PT_LOCAL_MAX_LEVELS                                           (outside: invalid)
 *   sigma       0 = 0.5                                                                        (negative or non-finite: invalid)
 * Any image size from 1 x 1 is valid. */
#define PT_LOCAL_MAX_LEVELS 8
typedef struct pt_local_params {
    float strength;
    float pivot;
    int32_t levels;
    float sigma;
} pt_local_params;

/* The local exposure kernels alone, on a host image: out_rgb (may be mean_rgb) = the output above for (mean_rgb, count), made on
 * HIP device `device`; kernel_ms (may be NULL) = HIP-event time of the L + 2 kernels.  Buffers, sizes, `exposure` (finite and > 0; 0
 * is NOT a default here, as in pt_grade_host) and *l are checked BEFORE the device is looked at; PT_ERR_NO_DEVICE afterwards if that
 * is not a usable device (there is no CPU fallback).  With strength == 0 it copies. */
int pt_local_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure,
                  const pt_local_params *l, float *out_rgb, float *kernel_ms);
/* pt_display_present_bloom with local exposure: the same chain with the local exposure kernels between bloom's and the display
 * kernel, on the session's stream with no host synchronisation inside; the gain reads e from the device scalar the display kernel
 * reads.  The bytes are DEFINED by the host chain and equal it bit for bit: the row of the tables above up to the linear mean and
 * count, then, if automatic, pt_meter_host -> pt_exposure_from_histogram on the mean BEFORE bloom, then
 * pt_bloom_host(e) -> pt_local_host(e) -> pt_grade_host(e, curve) -> pt_tonemap -> pt_quantize, at the output size (after the
 * upsample if u is given).  *b and *l are checked with *g, before anything is enqueued and before the device is looked at; a failed
 * present leaves the history and the previous exposure as they were.  A deferred pixel carries the locally exposed ungraded mean
 * the display kernel read, and the host grades that.  With a zeroed *l the call is pt_display_present_bloom. */
int pt_display_present_local(pt_display *d, const pt_display_params *p, const pt_upsample_params *u /* NULL: not scaled */,
                             const pt_grade_params *g, const pt_bloom_params *b, const pt_local_params *l, uint8_t *bgr,
                             pt_display_info *info /* may be NULL */, pt_grade_info *grade_info /* may be NULL */);

/* ---- colour grading: white balance, saturation, matrix and a .cube 3D LUT ---------------------------------------- */

/* Everything above acts on luminance or per channel; nothing can move a colour.  Colour grading is the grade with two steps more,
 * in two places.  A 3 x 3 MATRIX acts on the linear mean BEFORE the exposure and the curve: white balance gains, saturation and a
 * user matrix, folded into one matrix, belong to scene-referred light, where they are linear.  A 3D LUT with tetrahedral
 * interpolation acts on the curve's OUTPUT g, before the gamma table is searched: a look exported by a grading tool as a .cube file
 * is display-referred, made for values in 0 .. 1.  The stage takes pt_grade_host's place in the chain; per pixel with count != 0 it is
 *   m' = M m,   x = m' * e,   g = curve(x),   out = LUT(g),
 * and out takes g's place in pt_tonemap -> pt_quantize (host) or in the display kernel's table search (device).  The meter, bloom
 * and local exposure read the mean BEFORE the matrix: the metered exposure, the bright pass and the base do not depend on it.
 *
 * The arithmetic, exactly: every line below is ONE correctly rounded float operation in the order written (* + -, comparisons,
 * one float -> int conversion); nothing is fused, and there is no pow, log or exp.
 *
 * Matrix.  Composed on the host in double, M = U S W, each entry rounded to float once:
 *   W = diag(wb)                                         wb = 0 0 0 means 1 1 1
 *   S = s I + (1 - s) 1 (0.2126, 0.7152, 0.0722)         (every row of the second term is the meter's weights, as doubles)
 *       s = saturation if saturation_set != 0 or saturation != 0, else 1: a caller who wants grey passes saturation = 0 with
 *       saturation_set = 1
 *   U = matrix, row-major;                               all nine zero means the identity
 *   in this order, in double:  X_ij = ((i == j ? s : 0) + ((1 - s) * lum_j)) * w_j,   M_ij = ((U_i0 * X_0j) + (U_i1 * X_1j)) + (U_i2 * X_2j),
 *   then (float)M_ij.  With nothing set every M_ij is 1 or +0 exactly.
 * Applied to the mean pt_grade_host would read (after bloom and local exposure):
 *   m'_r = ((M00 * m_r) + (M01 * m_g)) + (M02 * m_b)
 *   m'_g = ((M10 * m_r) + (M11 * m_g)) + (M12 * m_b)
 *   m'_b = ((M20 * m_r) + (M21 * m_g)) + (M22 * m_b)
 * If M is the identity BIT FOR BIT (1 on the diagonal, +0 elsewhere) the three lines are skipped: 1 * x + 0 * y is not x for NaN or
 * infinite inputs, and the bytes are then pt_grade_host's.
 *
 * LUT of size N, 2 <= N <= PT_LUT_MAX_SIZE; vertices c(i_r, i_g, i_b), three floats each, at index ((i_b N) + i_g) N + i_r: the
 * red index runs fastest, the order of a .cube file.  Per channel ch of g:
 *   x = !(g_ch >= 0) ? 0 : (g_ch > 1 ? 1 : g_ch)         (NaN and negatives -> 0)
 *   s = x * (float)(N - 1)
 *   i = (int)s;   if (i > N - 2) i = N - 2
 *   f = s - (float)i                                      (x = 1 gives i = N - 2, f = 1 exactly)
 * The tetrahedron, by comparisons in this order (ties have one answer); its path names the axes in the order f1 >= f2 >= f3:
 *   f_r >= f_g:   f_g >= f_b -> r,g,b     else f_r >= f_b -> r,b,g     else -> b,r,g
 *   otherwise:    f_r >= f_b -> g,r,b     else f_g >= f_b -> g,b,r     else -> b,g,r
 * Vertices:  A = c(i),  B = A's index + 1 on the first axis,  C = B's index + 1 on the second axis,  D = c(i_r + 1, i_g + 1, i_b + 1).
 * Per output channel:
 *   out = ((A + (f1 * (B - A))) + (f2 * (C - B))) + (f3 * (D - C))
 * At a vertex (all f = 0) out = A to the bit (entries whose differences are finite; a -0 comes out as +0); a constant LUT returns its constant to the bit; along any path
 * out is piecewise linear and continuous.  A negative or NaN out defers the pixel on the device, as a negative or NaN g does; the
 * host finishes a deferred pixel from the mean the kernel read -- the one before the matrix -- with these same steps.
 *
 * Parameters; a zeroed struct means the stage does not run (the bytes are those without it):
 *   wb           three gains, each finite and >= 0; all zero = 1 1 1                              (else: invalid)
 *   saturation   finite and >= 0; see s above                                                    (else: invalid)
 *   matrix       nine finite numbers; all zero = identity                                        (else: invalid)
 *   lut          NULL: no LUT; else a pt_lut that outlives the call */
#define PT_LUT_MAX_SIZE 65
typedef struct pt_lut pt_lut;                    /* an immutable 3D LUT in host memory */
typedef struct pt_colour_params {
    float wb[3];
    float saturation;
    int32_t saturation_set;
    float matrix[9];
    const pt_lut *lut;
} pt_colour_params;

/* Host only, no device.  pt_lut_create copies n^3 vertices of three floats (red index fastest); pt_lut_load_cube reads a .cube file:
 * blank lines, lines that start with '#', TITLE "...", LUT_3D_SIZE N, DOMAIN_MIN 0 0 0, DOMAIN_MAX 1 1 1 and exactly N^3 data lines
 * of three numbers read with strtof, with LF or CR LF line ends.  PT_ERR_UNSUPPORTED: LUT_1D_SIZE, any other domain, N outside
 * 2 .. PT_LUT_MAX_SIZE.  PT_ERR_INVALID_ARGUMENT: a NULL pointer, too few or too many data lines, a token that does not parse, a value
 * that is not finite, a missing or repeated size line.  PT_ERR_IO: the file cannot be opened.  A failed call writes nothing to *out,
 * and pt_last_error names the line.  Every LUT made carries a generation number of its own: a display uploads a LUT again only
 * when the one it is given is not the one it holds. */
int pt_lut_create(int32_t n, const float *rgb, pt_lut **out);
int pt_lut_load_cube(const char *path, pt_lut **out);
int pt_lut_size(const pt_lut *lut, int32_t *n);
void pt_lut_destroy(pt_lut *lut);

/* Host only, pure: M of *c as stated above, row-major.  On PT_ERR_INVALID_ARGUMENT out is not written. */
int pt_colour_matrix(const pt_colour_params *c, float out[9]);
/* Host only, no device: out_rgb = LUT(curve((M mean_rgb) * exposure)) for pixels with count != 0, the others keep their value
 * (out_rgb may be mean_rgb).  The chain of an image with the stage is ... -> pt_colour_host -> pt_tonemap -> pt_quantize.  Checked as
 * pt_grade_host checks, and *c as above; with a zeroed *c it is pt_grade_host. */
int pt_colour_host(int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure, int32_t curve,
                   const pt_colour_params *c, float *out_rgb);
/* pt_display_bytes_graded_host with the colour stage: meter (if automatic, on the mean before the matrix), exposure and the colour
 * display kernel as one chain on HIP device `device`, on a host image.  Everything is checked before the device is looked at. */
int pt_display_bytes_colour_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count,
                                 float gamma, const pt_grade_params *g, const pt_colour_params *c, int32_t has_prev, float e_prev,
                                 uint8_t *bgr, pt_display_info *info /* may be NULL */, pt_grade_info *grade_info /* may be NULL */);
/* pt_display_present_local with the colour stage: the same chain with the colour display kernel in the graded one's place; the
 * kernel reads the mean once and writes 3 bytes.  The bytes are DEFINED by the host chain and equal it bit for bit: the row of the
 * tables above up to the linear mean and count, then, if automatic, pt_meter_host -> pt_exposure_from_histogram on the mean BEFORE
 * bloom, then pt_bloom_host(e) -> pt_local_host(e) -> pt_colour_host(e, curve) -> pt_tonemap -> pt_quantize, at the output size.  *c is
 * checked with *g, before anything is enqueued and before the device is looked at; a failed present leaves the history and the
 * previous exposure as they were.  The display keeps a device copy of the LUT and uploads again only when the generation of the
 * pt_lut it is given differs.  With a zeroed *c the call is pt_display_present_local. */
int pt_display_present_colour(pt_display *d, const pt_display_params *p, const pt_upsample_params *u /* NULL: not scaled */,
                              const pt_grade_params *g, const pt_bloom_params *b, const pt_local_params *l, const pt_colour_params *c,
                              uint8_t *bgr, pt_display_info *info /* may be NULL */, pt_grade_info *grade_info /* may be NULL */);

/* ---- lens optics: radial distortion, lateral chromatic aberration, vignetting ------------------------------------ */

/* pt_camera and pt_lens form the ray; nothing above bends a straight line, splits an edge into colour fringes or darkens the
 * corners, as the glass of a real lens does.  Optics is one stage, (mean, count) -> (mean', count'), on the linear mean at the
 * OUTPUT size: after the denoiser, the temporal merge and the upsample, and BEFORE the meter, bloom, local exposure and the grade or
 * colour stage, which all read mean' and count' in place of mean and count -- the sensor meters what the lens delivers.  The
 * first-hit features, the temporal reprojection and the upsampler do not see the stage.  It is a gather: each output channel is
 * resampled from four taps at a position of its own.
 *
 * The arithmetic, exactly: every line below is ONE correctly rounded float operation in the order written (* / + -, comparisons,
 * int <-> float conversions); nothing is fused, and there is no pow, log, exp or trigonometry -- the stage is rational.
 *
 * Geometry, for output pixel (x, y) of W x H:
 *   cx = 0.5 * (float)(W - 1),   cy = 0.5 * (float)(H - 1)            (the centre)
 *   px = (float)x - cx,          py = (float)y - cy
 *   hh = 0.5 * (float)H,         u = px / hh,   v = py / hh            (normalised by half the height)
 *   r2 = (u * u) + (v * v)
 *   f  = 1 + (r2 * (k1 + (k2 * r2)))                                   (k1 < 0: barrel; k1 > 0: pincushion)
 * The magnification of channel ch, composed on the host and rounded once:  mag = (1 - ca, 1, 1 + ca)  for r, g, b.  The source
 * position of channel ch:
 *   s  = f * mag_ch
 *   sx = cx + (px * s),   sy = cy + (py * s)
 *   sx = !(sx >= 0) ? 0 : (sx > (float)(W - 1) ? (float)(W - 1) : sx),   sy likewise against H - 1      (NaN -> 0; the edge repeats)
 *
 * Bilinear resample of channel ch at (sx, sy):
 *   x0 = (int)sx,   fx = sx - (float)x0,   x1 = x0 + 1, and x1 = W - 1 if it exceeds that;   y0, fy, y1 likewise
 *   the taps in the order (x0,y0), (x1,y0), (x0,y1), (x1,y1), each with  w = wx * wy,  where wx = 1 - fx for x0 and fx for x1,
 *   wy = 1 - fy for y0 and fy for y1
 *   a tap with w == 0 or with count == 0 is skipped: its value is never read, so a NaN in an unsampled pixel cannot leak
 *   otherwise, with m = the tap's mean of channel ch (a chain row that ends in sums: m = sum / (float)count, as the display divides):
 *     the FIRST tap kept:   ref = m,   sw = w,   sd = 0
 *     every later one:      sw = sw + w
 *                           sd = sd + (w * (m - ref))
 *   no tap kept: the channel is EMPTY;  else  val_ch = ref + (sd / sw).
 * This is the weighted mean sum(w m) / sum(w) of the taps kept, taken about the first of them -- the form of the denoiser's and of
 * local exposure's sums (b + sd / sw), for their reason: rounded products w * m of EQUAL values do not add up to that value times the
 * rounded sum of w (of random c, fx, fy in 0 .. 1 a third come back an ulp off from sum(w c) / sum(w)), while differences of equal
 * values are 0.
 *
 * Vignette, from the OUTPUT pixel's r2:
 *   q    = 1 + (vig * r2)
 *   gain = 1 / (q * q)            (cos^4 of the field angle whose tangent is sqrt(vig) r: the natural fall-off, without a root)
 *   out_ch = val_ch * gain
 *
 * Count.  If any channel is empty, out = 0 0 0 and count' = 0; otherwise count' = 1 (the denoiser's count_out convention).
 *
 * Properties (the tests rely on them):
 *   - k1 = k2 = ca = 0:  f = 1 and mag = 1, so s = 1;  px = x - cx is exact (multiples of 0.5 below 2^22) and cx + px gives back
 *     x exactly, for W and H below 2^22: sx == x and sy == y.  Then fx = fy = 0, the one tap with a weight is the pixel itself,
 *     ref = m, sd = 0, and m + (0 / 1) = m: the resample returns m to the bit (a -0 comes out as +0), and a pixel with count == 0
 *     comes out empty, whatever its rgb holds.
 *   - vig = 0:  q = 1 and gain = 1 exactly.
 *   - an image that is constant over its valid pixels stays constant to the bit under the resample, whatever taps are skipped:
 *     every m - ref is 0, so sd = 0 and val = ref + 0.
 *
 * Parameters; a zeroed struct means the stage does not run, and the bytes and counts are those of the chain without it:
 *   k1, k2      finite, |k| <= 4                                                               (else: invalid)
 *   ca          finite, |ca| <= 0.25                                                           (else: invalid)
 *   vignette    finite, 0 .. 64                                                                (else: invalid)
 * Any image size from 1 x 1 is valid. */
typedef struct pt_optics_params {
    float k1, k2;
    float ca;
    float vignette;
} pt_optics_params;

/* The optics kernel alone, on a host image: (out_rgb, out_count) = the output above for (mean_rgb, count), made on HIP device
 * `device`; kernel_ms (may be NULL) = HIP-event time of the kernel.  The stage is a gather: out_rgb must not be mean_rgb and
 * out_count must not be count.  Buffers, sizes and *o are checked BEFORE the device is looked at; PT_ERR_NO_DEVICE afterwards if
 * that is not a usable device (there is no CPU fallback).  With a zeroed *o it copies mean_rgb and count. */
int pt_optics_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, const pt_optics_params *o,
                   float *out_rgb, int32_t *out_count, float *kernel_ms);
/* pt_display_present_colour with the optics stage: the same chain with the optics kernel enqueued on the session's stream AHEAD of
 * the meter, with no host synchronisation inside; the meter, bloom, local exposure and the display kernel read the planes it
 * wrote.  The bytes are DEFINED by the host chain and equal it bit for bit: the row of the tables above up to the linear mean and
 * count at the output size (after the upsample if u is given), then pt_optics_host, then, if automatic, pt_meter_host ->
 * pt_exposure_from_histogram on mean' and count', then pt_bloom_host(e) -> pt_local_host(e) -> pt_colour_host(e, curve) ->
 * pt_tonemap -> pt_quantize with count'.  *o is checked with *g, before anything is enqueued and before the device is looked at; a
 * failed present leaves the history and the previous exposure as they were.  A deferred pixel carries the mean AFTER optics (and
 * bloom and local exposure), which the host finishes.  The display owns two more planes, rgb and count at the output size,
 * allocated by the first present with the stage.  With a zeroed *o the call is pt_display_present_colour. */
int pt_display_present_optics(pt_display *d, const pt_display_params *p, const pt_upsample_params *u /* NULL: not scaled */,
                              const pt_grade_params *g, const pt_bloom_params *b, const pt_local_params *l, const pt_colour_params *c,
                              const pt_optics_params *o, uint8_t *bgr, pt_display_info *info /* may be NULL */,
                              pt_grade_info *grade_info /* may be NULL */);

/* ---- sharpening: a contrast-adaptive sharpen of the luminance before the grade ------------------------------------ */

/* The denoiser, the temporal merge, the upsample and the optics resample each buy their speed or their look with softness, and no
 * stage above gives acuity back.  Sharpening is one stage, mean -> mean (count unchanged), on the linear mean at the OUTPUT size,
 * AFTER bloom and local exposure and IMMEDIATELY BEFORE the grade or the colour stage: the meter, bloom and local exposure do not
 * see it; the matrix, the exposure, the curve and the LUT act on what it wrote.  Every pixel is multiplied by ONE gain, computed
 * from a negative-lobe cross filter of the LUMINANCE whose lobe is as strong as the ring's headroom to black and to white allows.
 * The filter works in a range-compressed domain y = a / (1 + a) of the exposed luminance a = l e, so that it can act on
 * scene-linear light: a plain unsharp mask on HDR values rings for many pixels round every emitter, and has no "white" to measure
 * headroom against.
 *
 * The arithmetic, exactly: every line below is ONE correctly rounded float operation in the order written (* / + -, comparisons);
 * nothing is fused, and there is no pow, log, exp or root -- the stage is rational, for the reason the denoiser's weights are.
 * min(p, q) is (q < p ? q : p) and max(p, q) is (q > p ? q : p).
 *
 * Inputs.  m = the pixel's linear mean (a chain row that ends in sums: m = sum / (float)n, as the display chain divides; behind bloom
 * or local exposure, their output), its count, the exposure e (manual or from the meter), and the parameters strength and limit.
 *
 * Compressed luminance plane, at W x H.  A pixel with count == 0 is INVALID.  Otherwise
 *   l = ((0.2126 m_r) + (0.7152 m_g)) + (0.0722 m_b)          (the meter's luminance)
 *   a = l * e
 *   if !(a >= 0) or !(a <= 65536):  INVALID  (negative, NaN, infinite, or too bright to compress distinctly from 1)
 *   else  y = a / (1 + a),
 * so 0 <= y <= Y1, where Y1 = (float)(65536.0 / 65537.0) < 1.  An invalid pixel keeps its value, NaN or infinity included, and is
 * never a tap.
 *
 * Sharpen, for a valid pixel with compressed luminance c.  The ring is b, d, f, h: the pixels above (y - 1), left (x - 1), right
 * (x + 1) and below (y + 1), in that order; a ring pixel outside the image or invalid takes the value c.
 *   mn   = min(min(b, d), min(f, h));   mx = max(max(b, d), max(f, h))
 *   hmin = mx > 0 ? mn / (4 * mx) : 0
 *   hmax = (1 - mx) / ((4 * mn) - 4)            (<= 0; the denominator is <= -4 (1 - Y1) < 0)
 *   lobe = max(-hmin, hmax);  lobe = min(lobe, 0);  lobe = max(lobe, -limit);  lobe = lobe * strength
 *   den  = 1 + (4 * lobe)                        (>= 1 - 4 limit >= 0.25)
 *   sd   = (((b - c) + (d - c)) + (f - c)) + (h - c)
 *   y'   = c + ((lobe * sd) / den)
 *   y'   = !(y' >= 0) ? 0 : (y' > Y1 ? Y1 : y')
 * In the reals this is (c + lobe (b + d + f + h)) / (1 + 4 lobe).  It is taken about the centre for the reason the denoiser's and
 * local exposure's sums are: differences of EQUAL values are 0, and rounded products of equal values do not sum to that value.
 *
 * Gain and output.
 *   l0 = c  / (1 - c)
 *   l1 = y' / (1 - y')
 *   g  = l0 > 0 ? l1 / l0 : 1
 *   out_ch = m_ch * g          per channel.
 * Both luminances go through the same expression, so y' == c gives l1 == l0 bit for bit and g = 1 exactly: a pixel whose ring
 * equals it (a constant region, a 1 x 1 image, a pixel whose neighbours are all outside or invalid) comes back to the bit.  One
 * gain serves the three channels, so the ratios out_r : out_g : out_b are those of m.  For a finite mean that is not negative the
 * output is finite and not negative, and l1 <= Y1 / (1 - Y1).
 *
 * Parameters; a zeroed struct means the stage does not run:
 *   strength    0: the stage is not run (the bytes are those of pt_display_present_optics); else in (0, 1]
 *                                                                                  (negative, above 1 or non-finite: invalid)
 *   limit       the largest lobe; 0 = 0.1875; else in (0, 0.1875]                  (negative, above 0.1875 or non-finite: invalid)
 * Any image size from 1 x 1 is valid. */
typedef struct pt_sharpen_params {
    float strength;
    float limit;
} pt_sharpen_params;

/* The sharpening kernels alone, on a host image: out_rgb (may be mean_rgb) = the output above for (mean_rgb, count), made on HIP
 * device `device`; kernel_ms (may be NULL) = HIP-event time of the two kernels.  Buffers, sizes, `exposure` (finite and > 0; 0 is NOT
 * a default here, as in pt_local_host) and *s are checked BEFORE the device is looked at; PT_ERR_NO_DEVICE afterwards if that is not
 * a usable device (there is no CPU fallback).  With strength == 0 it copies. */
int pt_sharpen_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure,
                    const pt_sharpen_params *s, float *out_rgb, float *kernel_ms);
/* pt_display_present_optics with sharpening: the same chain with the two sharpening kernels between local exposure's and the
 * display kernel, on the session's stream with no host synchronisation inside; the gain reads e from the device scalar the display
 * kernel reads.  The bytes are DEFINED by the host chain and equal it bit for bit: ... -> pt_optics_host -> meter ->
 * pt_bloom_host(e) -> pt_local_host(e) -> pt_sharpen_host(e) -> pt_colour_host(e, curve) -> pt_tonemap -> pt_quantize, at the
 * output size.  The metered exposure does not depend on the stage.  *s is checked with *g, before anything is enqueued and before
 * the device is looked at; a failed present leaves the history and the previous exposure as they were.  A deferred pixel carries the
 * sharpened mean, which the host finishes.  The display owns one more plane, 4 bytes a pixel at the output size, and a plane of
 * means where no stage of its own wrote the image the stage reads, allocated by the first present with the stage.  With a zeroed *s
 * the call is pt_display_present_optics. */
int pt_display_present_sharpen(pt_display *d, const pt_display_params *p, const pt_upsample_params *u /* NULL: not scaled */,
                               const pt_grade_params *g, const pt_bloom_params *b, const pt_local_params *l, const pt_colour_params *c,
                               const pt_optics_params *o, const pt_sharpen_params *s, uint8_t *bgr, pt_display_info *info /* may be NULL */,
                               pt_grade_info *grade_info /* may be NULL */);

/* ---- film grain and dithered quantization: the display kernel's last step ------------------------------------------ */

/* Every stage above makes the picture smoother, and the chain's last step is the reference's bare truncation to 8 bits: smooth
 * gradients band.  Grain and dither are ONE stage with two parts, at the very end of the chain: they act on g, the value BEHIND matrix
 * -> exposure -> curve -> LUT (pt_colour_host's output, or pt_grade_host's), per channel, and take the place of pt_tonemap ->
 * pt_quantize.  No earlier stage sees that value, so on the device both live inside the display kernel: no plane is added.
 *
 * The arithmetic, exactly: every line below is ONE correctly rounded float operation in the order written (* / + -, comparisons,
 * floor, int <-> float conversions) or integer arithmetic; nothing is fused, and there is no pow, log, exp or root beyond the
 * threshold table's own, which is built once per gamma (pt_display_table).
 *
 * Random words.  Philox4x32-10 (Random123's rounds and constants) under key (seed, 0x50544831 "PTH1"), the integrator's key.  The
 * counter's fourth word is not zero; the integrator's always is, so no stream is shared with a render of the same seed.
 *   dither of pixel (x, y):          counter (x, y, frame, 1); words 0, 1, 2 serve r, g, b
 *   grain lattice point (ix, iy):    counter (ix, iy, frame, 2); word 0
 *   tri(w) = (float)((int)(w & 0xFFFF) + (int)(w >> 16) - 65535) * 2^-16
 * tri is a triangular variate in (-1, 1) with mean 0: the integer lies in -65535 .. 65535 and is exact in a float, the product too.
 *
 * Grain, for pixel (x, y) with count != 0 and strength != 0 (with strength == 0 no word is drawn and g' = g).  With s = size:
 *   fx = (float)x / s,   ix = (int)fx,   tx = fx - (float)ix;     fy, iy, ty likewise from y
 *   v00 = tri(lattice(ix, iy)),  v10 = tri(lattice(ix + 1, iy)),  v01 = tri(lattice(ix, iy + 1)),  v11 = tri(lattice(ix + 1, iy + 1))
 *   a = v00 + (tx * (v10 - v00)),   b = v01 + (tx * (v11 - v01)),   n = a + (ty * (b - a))
 *   sn = strength * n
 * At size == 1, tx = ty = 0 and n = v00 to the bit (the other three values are finite and multiplied by 0; they are not drawn).  One n
 * serves the three channels: the grain is monochrome.  A channel takes grain only if 0 < g && g < 1 (both false for NaN):
 *   w  = (g * (1 - g)) * 4
 *   g' = g + (sn * w);   g' = g' < 0 ? 0 : (g' > 1 ? 1 : g')
 * Every other channel keeps its BITS: black, clipped white, emitters, the reference curve's wrapped values above 1, negatives and NaN
 * pass unchanged.  The weight is 1 at mid-grey and falls to 0 at both ends, as film's does.
 *
 * Dither, per channel of g'.  T[1 .. levels] are the thresholds of pt_display_table(gamma), T[0] stands for 0.  The table COVERS g' if
 * g' >= 0 (false for NaN), g' < T[levels] and g' lies in no doubt band; then k, the number of thresholds <= g', is below levels, so
 * T[k + 1] is a threshold in use.  A covered channel with dither != 0:
 *   lo = T[k] (0 for k == 0),   hi = T[k + 1]                   (lo <= g' < hi)
 *   f  = (g' - lo) / (hi - lo)                                   (0 <= f <= 1)
 *   t  = f + (dither * tri(word of the channel))                 (-1 < t < 2)
 *   j  = (int)floor(t)                                            (-1, 0 or 1)
 *   k' = k + j;   if (k' < 0 || (k' >> 8) != (k >> 8)) k' = k    (black stays at or above 0; byte 255 and the wrapped levels stay in their block of 256)
 *   byte = k' & 255
 * A covered channel with dither == 0 is byte = k & 255, and a channel the table does not cover is (uint8_t)(int)(pow(g', gamma) * 255),
 * pt_tonemap's and pt_quantize's own steps, whatever dither is.  A pixel with count == 0 is three zero bytes.
 *
 * The mean is kept relative to the truncation: with dither == 1 and U1, U2 the two uniform halves of the word, t = f + U1 + U2 - 1;
 * E[floor(a + U)] = a for any a and a uniform U in [0, 1), applied twice E[j] = f + 1/2 - 1:  E[k'] = k + f - 1/2, and the variance
 * about that mean is 1/4 whatever f is -- the property triangular dither is chosen for: neither the mean error nor the noise power
 * shows the signal.  (The halves are 16-bit, so both hold to 2^-16.)
 *
 * Parameters; a zeroed struct means the stage does not run, and the bytes are those of pt_tonemap -> pt_quantize:
 *   strength    finite, 0 .. 1; 0 = no grain                                                        (else: invalid)
 *   size        the lattice pitch in pixels: finite, 0 (= 1) or 1 .. 8                               (else: invalid)
 *   dither      finite, 0 .. 1, in levels; 0 = none, 1 = full triangular dither                     (else: invalid)
 *   seed, frame any; frame is the noise's third coordinate: advance it once per presented frame
 * The stage runs if strength > 0 or dither > 0.  Any image size from 1 x 1 is valid. */
typedef struct pt_grain_params {
    float    strength;  /* 0 .. 1; 0 = no grain                      */
    float    size;      /* 1 .. 8 lattice pitch in pixels; 0 = 1     */
    float    dither;    /* 0 .. 1 of one level, triangular; 0 = none */
    uint32_t seed;
    uint32_t frame;     /* the noise's third coordinate              */
} pt_grain_params;

/* Host only, no device: the last step of every host chain with the stage, in the place of pt_tonemap -> pt_quantize:
 * ... -> pt_colour_host(e, curve) (or pt_grade_host) -> pt_grain_quantize.  graded_rgb is g; bgr gets B, G, R bytes, zero for pixels with
 * count == 0.  It uses the threshold table the device is given (pt_display_table(gamma), built on first use of a gamma).  Checked in
 * this order: NULL buffers and empty sizes, the image size, gamma (finite and > 0), *n as above.  With a zeroed *n the bytes are those
 * of pt_tonemap -> pt_quantize for every input. */
int pt_grain_quantize(int32_t width, int32_t height, const float *graded_rgb, const int32_t *count, float gamma, const pt_grain_params *n,
                      uint8_t *bgr);
/* pt_display_bytes_colour_host with the stage: meter (if automatic), exposure and the grain display kernel as one chain on HIP device
 * `device`, on a host image.  Everything is checked before the device is looked at.  With a zeroed *n it is
 * pt_display_bytes_colour_host. */
int pt_display_bytes_grain_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float gamma,
                                const pt_grade_params *g, const pt_colour_params *c, const pt_grain_params *n, int32_t has_prev,
                                float e_prev, uint8_t *bgr, pt_display_info *info /* may be NULL */, pt_grade_info *grade_info /* may be NULL */);
/* pt_display_present_sharpen with the stage: the same chain with the grain display kernel in the graded or the colour kernel's place;
 * it reads and writes what they do.  The bytes are DEFINED by the host chain and equal it bit for bit: ... -> pt_sharpen_host(e) ->
 * pt_colour_host(e, curve) -> pt_grain_quantize, at the output size.  *n is checked with *g, before anything is enqueued and before the
 * device is looked at; a failed present leaves the history and the previous exposure as they were.  A deferred pixel still carries the
 * mean before the matrix: the host redoes matrix -> exposure -> curve -> LUT -> grain -> dither for it from its index, seed and frame.
 * With a zeroed *n the call is pt_display_present_sharpen. */
int pt_display_present_grain(pt_display *d, const pt_display_params *p, const pt_upsample_params *u /* NULL: not scaled */,
                             const pt_grade_params *g, const pt_bloom_params *b, const pt_local_params *l, const pt_colour_params *c,
                             const pt_optics_params *o, const pt_sharpen_params *s, const pt_grain_params *n, uint8_t *bgr,
                             pt_display_info *info /* may be NULL */, pt_grade_info *grade_info /* may be NULL */);

/* ---- scene-linear output: PFM and Radiance .hdr from the display chain --------------------------------------------- */

/* Every output above is 24-bit bytes behind the display curve.  This stage encodes the LINEAR mean the display kernel would read -- the
 * image after optics, bloom, local exposure and sharpening, and before the colour matrix, exposure, curve, LUT and grain -- as the body
 * of a float picture file, on the device where it lies.  It reads that image and writes a buffer of its own: no stage sees what it
 * wrote, and the bytes of the BMP are the same with and without it.
 *
 * The input of a pixel is its mean m = (r, g, b) and its count.  With exposed != 0 every channel is first m * e, ONE float multiply, e
 * being the exposure the present used (metered or manual); with exposed == 0 it is m, bits untouched.  A pixel with count == 0 is
 * all-zero bytes in both formats, whatever its mean holds.
 *
 * PT_LINEAR_PFM: 12 bytes per pixel, the three floats little-endian r, g, b with their BITS unchanged (NaN payloads, -0, inf and
 * negatives are kept), rows BOTTOM-UP as PFM has them: the pixel (x, y) of the image lies at byte 12 * ((height - 1 - y) * width + x).
 * The buffer is the file's body as it stands; pt_write_pfm prepends "PF\n<W> <H>\n-1.0\n" (the negative scale says little-endian).
 *
 * PT_LINEAR_RGBE: 4 bytes per pixel R, G, B, E, rows top-down: a FLAT (not run-length encoded) Radiance picture, which pt_write_hdr
 * gives the header "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y <H> +X <W>\n".  Per pixel, in integer arithmetic, comparisons and one exact
 * multiply per channel -- no frexp, ldexp or log:
 *   c'    = (c > 0) ? (c < 2^126 ? c : 2^126) : 0     per channel: NaN, -0 and negatives give 0, +inf gives 2^126
 *   v     = max(r', g', b');   be = (bits(v) >> 23) & 255
 *   if (be < 27) the pixel is 0, 0, 0, 0               (v < 2^-100, subnormals among them)
 *   scale = the float whose bits are (261 - be) << 23  (2^(8 - e) with e = be - 126; its exponent field lies in 8 .. 234: a normal float)
 *   byte_c = (int)(c' * scale)                         (the product is exact, or below 1 and truncated to 0; it is always below 256)
 *   E     = be + 2                                     (29 .. 255)
 * The largest channel's byte lies in 128 .. 255.  This is not Radiance's own m * 256 / v, from which it differs in rare last-step
 * roundings; what holds for every channel, and what a reader may rely on, is
 *   | (byte + 0.5) * 2^(E - 136) - c' | <= 2^(E - 137).
 * Flat scanlines are legal in a Radiance picture, and a reader cannot take one of these pixels for a run-length marker: the marker of the
 * new encoding is a pixel with R = G = 2 and bit 7 of B clear, and here a pixel with R = G = 2 has its largest byte, at least 128, in B;
 * the marker of the old one is R = G = B = 1, and no pixel here has all three below 128 unless it is 0, 0, 0, 0.
 *
 * format 0 means the stage does not run; any other value than PT_LINEAR_PFM and PT_LINEAR_RGBE is invalid, and so is an exposed other
 * than 0 or 1.  Any image size from 1 x 1 is valid. */
#define PT_LINEAR_PFM 1
#define PT_LINEAR_RGBE 2
typedef struct pt_linear_params {
    int32_t format;     /* 0 = stage off, PT_LINEAR_PFM 1, PT_LINEAR_RGBE 2 */
    int32_t exposed;    /* 0: m as it is; 1: m * e                           */
} pt_linear_params;

/* The size of the body in bytes: 12 or 4 per pixel.  0 for a format that is neither of the two, or a size that is empty or too large. */
size_t pt_linear_bytes(int32_t width, int32_t height, int32_t format);
/* Host only, no device: THE DEFINITION of the bytes.  mean_rgb is the mean (r, g, b per pixel, rows top-down), out has room for
 * pt_linear_bytes.  `exposure` is read only with exposed != 0.  Checked in this order: NULL buffers and empty sizes, the image size,
 * *lin (format 1 or 2 -- 0 encodes nothing and is refused here --, exposed 0 or 1), and with exposed != 0 the exposure (finite and > 0). */
int pt_linear_encode(int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure,
                     const pt_linear_params *lin, uint8_t *out);
/* The kernel alone on a host image, on HIP device `device`; the bytes are pt_linear_encode's.  Everything is checked, as there, before
 * the device is looked at; PT_ERR_NO_DEVICE afterwards if that is not a usable device (there is no CPU fallback).  info->kernel_ms is the
 * HIP-event time of the kernel; deferred_pixels is 0: the kernel finishes every pixel. */
int pt_linear_encode_device_host(int device, int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float exposure,
                                 const pt_linear_params *lin, uint8_t *out, pt_display_info *info /* may be NULL */);
/* pt_display_present_grain with the stage: the same chain, plus one encode kernel on the image the display kernel reads, enqueued
 * immediately before it inside the timed chain.  ONE present makes both outputs, and a present with a temporal stage pushes the history
 * exactly once.  `linear` gets pt_linear_bytes at the output size, DEFINED by the host chain: ... -> pt_sharpen_host(e) ->
 * pt_linear_encode(e).  g may be NULL for a chain with no grade at all (the bytes of pt_display_present / _scaled): then b, l, c, o, s
 * and n must be NULL too and exposed must be 0, else PT_ERR_INVALID_ARGUMENT.  bgr may be NULL: the display kernel and its copy are
 * skipped.  *lin is checked with the other blocks, before anything is enqueued and before the device is looked at; a failed present
 * leaves the history and the previous exposure as they were.  With format 0 `linear` is not written and may be NULL, bgr may not, and
 * the call is pt_display_present_grain (or, with g NULL, pt_display_present_scaled / pt_display_present). */
int pt_display_present_linear(pt_display *d, const pt_display_params *p, const pt_upsample_params *u /* NULL: not scaled */,
                              const pt_grade_params *g, const pt_bloom_params *b, const pt_local_params *l, const pt_colour_params *c,
                              const pt_optics_params *o, const pt_sharpen_params *s, const pt_grain_params *n, const pt_linear_params *lin,
                              uint8_t *bgr /* may be NULL */, uint8_t *linear, pt_display_info *info /* may be NULL */,
                              pt_grade_info *grade_info /* may be NULL */);
/* The header stated above, then the body (pt_linear_bytes of it).  PT_ERR_INVALID_ARGUMENT: a NULL pointer, an empty or too large size;
 * PT_ERR_IO, with the reason in pt_last_error: the file cannot be opened or written. */
int pt_write_pfm(const char *path, int32_t width, int32_t height, const uint8_t *body);
int pt_write_hdr(const char *path, int32_t width, int32_t height, const uint8_t *body);

/* main.cpp:179-182 alone, on the host: rgb = pow(mean_rgb, gamma) * 255 per channel for pixels with count != 0, the others keep
 * their value.  With mean_rgb = sum / n it gives the image of pt_resolve_float bit for bit. */
int pt_tonemap(int32_t width, int32_t height, const float *mean_rgb, const int32_t *count, float gamma, float *rgb);

/* ---- resolve + image output (host side, as in the reference) --------------------------------------- */

/* main.cpp:162-201: per-pixel mean, gamma tonemap *255, float->uint8 truncation (bitmap_image.hpp:194-206),
 * dispersion statistics.  bgr: height*width*3 bytes, top-down rows, B,G,R order; pixels without samples stay 0.
 * dispersion[0..2] = max, min, average exactly as they are embedded in the reference's output file name. */
int pt_resolve(int32_t width, int32_t height, const float *sum, const float *sum2, const int32_t *count,
               float gamma, uint8_t *bgr, float *dispersion);

/* The same in three steps, for the optional post filters (-GAUSS / -MEDIAN, main.cpp:187-192):
 *   pt_resolve_float     main.cpp:162-185: statistics + the tonemapped FLOAT image (rgb: height*width*3, r,g,b order;
 *                        pixels without samples keep their raw sums, as color_map does)
 *   pt_post_filter_host  GaussBlur (main.cpp:11-33) if gauss != 0, then MedianFilter (main.cpp:49-80) if median != 0,
 *                        on HIP device `device`, in place on the host image; median <= 11.  The image is expected to hold
 *                        neither NaN nor -0.0: the reference reads its "median" from a sorted window, where the place of a
 *                        NaN is undefined and which of two equal zeros lands at the chosen rank is unspecified
 *   pt_quantize          main.cpp:193-201: float -> uint8 truncation, only for pixels with samples */
int pt_resolve_float(int32_t width, int32_t height, const float *sum, const float *sum2, const int32_t *count,
                     float gamma, float *rgb, float *dispersion);
int pt_post_filter_host(int device, int32_t width, int32_t height, float *rgb, int32_t gauss, int32_t median);
int pt_quantize(int32_t width, int32_t height, const float *rgb, const int32_t *count, uint8_t *bgr);

/* bitmap_image::save_image (bitmap_image.hpp:431-478): 54-byte header, bottom-up rows padded to 4 bytes. */
int pt_write_bmp(const char *path, int32_t width, int32_t height, const uint8_t *bgr);

/* ---- diagnostics ---------------------------------------------------------------------------------- */

/* The culling hierarchy built for `eps` and the handle's current camera and lens (host side; works on device < 0 scenes).  A
 * camera (with its lens) whose origins lie within the default envelope (every |component| <= max(20, largest |vertex coordinate|)) shares the
 * camera-free hierarchy; a farther one gets margins for its larger envelope.  counts[4] = clusters, sphere
 * records, barycentric records, triangles handled by the barycentric class.  Pass NULL tables to query counts only.
 * clusters: 16 words each (centre[3], r2, then as uint32 bit patterns first_tri, n_tri, kind, data_off, n_levels,
 * level_off[7]: the sphere tree of a small-triangle cluster, see path-tracing_amd/csrc/pt_scene.hpp);
 * spheres: 4 floats each (centre[3], r2); bary: 12 floats each; constants: k1, k2, a_max, m0, t_guard. */
int pt_scene_cull_tables(pt_scene *scene, float eps, int32_t *counts, float *clusters, float *spheres, float *bary,
                         float *constants);

/* The order in which the hierarchy lists the triangles ("slots": the table builder groups triangles spatially, so the
 * hierarchy does not depend on the file order).  counts[4] = slots, box-tree nodes, inner nodes among them (the others are leaves of 8 slots each), clusters;
 * slot_triangle[k] = original triangle index of slot k, or -1 for a padding slot; bvh_nodes = the box tree of a big
 * scene, 64 bytes per node (path-tracing_amd/csrc/pt_scene.hpp: BvhNode).  Pass NULL to skip either.
 * In pt_scene_cull_tables the cluster fields first_tri / n_tri are slot ranges. */
int pt_scene_cull_layout(pt_scene *scene, float eps, int32_t *counts, int32_t *slot_triangle, void *bvh_nodes);

/* The kernels' tables pack indices into bit fields: (ray, slot) work items hold a slot in 24 bits; a box-tree node keeps its
 * base in 20 bits of BvhNode::meta (bits 12-31; bit 11 is the leaf flag) -- an inner node's first child, so fewer than 2^20
 * nodes, or a leaf's first slot / 8 in the GLOBAL slot order, so with a box tree fewer than 2^23 slots --; a sphere tree has at
 * most 8 levels; and the box tree, whose depth is variable, at most PT_MAX_BVH_DEPTH levels (the walk's stack slack is sized for
 * that).  A hierarchy beyond any of these is refused with PT_ERR_UNSUPPORTED when it is built (first render with an eps,
 * pt_scene_cull_tables / _layout), never truncated; this is the check itself, for counts.  bvh_depth = levels of the box tree
 * (root = 1; 0 = no box tree). */
#define PT_MAX_BVH_DEPTH 9
int pt_table_limits_check(uint64_t n_slots, uint64_t n_bvh_nodes, int32_t n_levels);
int pt_table_limits_check_tree(uint64_t n_slots, uint64_t n_bvh_nodes, int32_t n_levels, int32_t bvh_depth);

/* Host seconds spent on this scene's model so far: seconds[0] = parsing + per-triangle tables (pt_scene_load_obj /
 * pt_scene_create), seconds[1] = building culling hierarchies (one per eps, shared by all per-device copies). */
int pt_scene_timings(const pt_scene *scene, double *seconds);

/* Page-locked host memory for accumulator buffers: transfers to and from it run at PCIe speed without the runtime's
 * staging copies (a first pageable transfer in a fresh process cost 0.1 s for a 1080p band here).  Optional: every entry
 * point also accepts ordinary (pageable) memory.  Returns NULL on failure; pt_host_free(NULL) is a no-op. */
void *pt_host_alloc(size_t bytes);
void pt_host_free(void *p);

/* ---- environment lighting: an HDR panorama as a light source ------------------------------------------------------- */

/* A scene handle may carry an ENVIRONMENT: a high-dynamic-range radiance map over the whole sphere.  A ray that hits nothing adds
 * throughput x L(direction) to its pixel -- one contribution like every other: sum, sum of squares, count -- and its path ends.  That
 * holds for primary rays too, so the map is also the background.  Unlike the skybox (pt_scene_set_skybox_bmp: 8-bit texels, the path
 * throughput not applied, the reference's rule) it lights the scene.  Without an environment every output is what it was.
 *
 * An environment belongs to the handle, as the skybox does: pt_scene_clone_to_device and pt_frame_create inherit it.  A handle has a
 * skybox OR an environment: setting one while the other is set is PT_ERR_INVALID_ARGUMENT.  It works with every view (camera-free,
 * camera, lens, motion, lens + motion, the projections), with statistics, on small and box-tree scenes.  Launches are planned as
 * under a skybox (path regeneration, the same tiles and chunks).  The first-hit feature pass does not look at it: a miss pixel's
 * features are what they are under a skybox.
 *
 * THE MAP.  The device does not look up the panorama.  It is resampled once, on the host, into an OCTAHEDRAL map of N x N texels
 * (r, g, b), 8 <= N <= 4096, stored with a one-texel apron so that the bilinear lookup never wraps an index:
 *   texel (-1, j) = texel (0, N-1-j)        texel (N, j) = texel (N-1, N-1-j)
 *   texel (i, -1) = texel (N-1-i, 0)        texel (i, N) = texel (N-1-i, N-1)
 * and the four corners by the two rules in turn (the octahedral fold: a point just outside an edge is the point mirrored about that
 * edge's midpoint).  pt_scene_set_environment_map takes the N x N x 3 interior, row j after row j - 1, and builds the apron.
 *
 * THE LOOKUP of unit direction d = (dx, dy, dz), y being the pole axis; every operation is a float operation rounded once, in the order
 * written, nothing fused:
 *   s  = (|dx| + |dy|) + |dz|;   px = dx / s;   pz = dz / s
 *   if dy < 0:  qx = (1 - |pz|) with the sign bit of px,  qz = (1 - |px|) with the sign bit of pz   (both from the unfolded px, pz)
 *   else        qx = px, qz = pz                                                                    (dy = -0 is not < 0)
 *   fx = (qx * 0.5 + 0.5) * N - 0.5;   x0 = floor(fx) clamped to -1 .. N-1 (a NaN goes to -1);   ax = fx - x0
 *   fy, y0, ay likewise from qz
 *   L  = (T(x0, y0) * (1 - ax) + T(x0+1, y0) * ax) * (1 - ay) + (T(x0, y0+1) * (1 - ax) + T(x0+1, y0+1) * ax) * ay     per channel
 * No trigonometry and no double precision; pt_environment_lookup is this on the host, and the kernels run the same code.
 *
 * THE CONVERSION of an equirectangular picture, w x h x 3 floats, rows top-down, at most 16384 x 8192, every sample finite and >= 0, into
 * the map; all in double, rounded to float once at the end.  With k = clamp(ceil(w / N), 1, 8), texel (i, j) is the mean over the
 * k x k sub-cell centres  qx = 2 (i + (a + 0.5) / k) / N - 1,  qz = 2 (j + (b + 0.5) / k) / N - 1  of the picture looked up at:
 *   dy = 1 - |qx| - |qz|;  (dx, dz) = (qx, qz) if dy >= 0, else ((1 - |qz|) with qx's sign, (1 - |qx|) with qz's sign);  u = d / |d|
 *   rotation about +y by r = rotate_y_degrees:  vx = cos r * ux + sin r * uz,  vy = uy,  vz = -sin r * ux + cos r * uz
 *   the skybox's own convention:  theta = acos(vy) / pi down the rows,  phi = atan2(vz, -vx) / (2 pi) + 0.5 along the columns
 *   fx = phi * w,  fy = theta * h;  x0 = floor(fx), ax = fx - x0, likewise y0, ay;  columns x0, x0 + 1 WRAP, rows y0, y0 + 1 are CLAMPED
 *   (P(x0, y0) (1 - ax) + P(x0+1, y0) ax) (1 - ay) + (P(x0, y0+1) (1 - ax) + P(x0+1, y0+1) ax) ay
 * and the mean is multiplied by gain.  The same panorama as skybox and as environment has the same orientation; a picture rendered with
 * PT_PROJECTION_EQUIRECT by the camera at the origin with forward (-1, 0, 0) and up (0, 1, 0) is in the picture's own frame (column
 * w / 2 lies in direction -x, columns grow from -x towards +z).  Default N (size 0): the smallest power of two >= h, clamped to 8 .. 2048.
 *
 * FILES.  The format is chosen by content.  Radiance: first line "#?RADIANCE" or "#?RGBE", a header line "FORMAT=32-bit_rle_rgbe",
 * an empty line, the resolution "-Y h +X w" (no other orientation); scanlines flat (what pt_write_hdr writes) or in the new-style
 * run-length coding (2, 2, w >> 8, w & 255, then each channel as runs: a count above 128 repeats the next byte count - 128 times,
 * a count of 1 .. 128 copies that many bytes).  A pixel decodes to (byte + 0.5) * 2^(E - 136) per channel, the inverse stated for
 * PT_LINEAR_RGBE; the pixel 0, 0, 0, 0 is black.  PFM: "PF", width, height, scale, one whitespace byte, rows bottom-up; little-endian
 * if the scale is negative, big-endian if positive; its magnitude is not applied.  PT_ERR_IO: the file cannot be read.  PT_ERR_PARSE:
 * anything else than these, a truncated file or bytes after the last row, a run that overruns its scanline or has length 0, another
 * orientation, "Pf", a non-finite or negative sample, a size above 16384 x 8192.
 *
 * PT_ERR_INVALID_ARGUMENT: NULL pointers, gain not finite or < 0, rotate_y_degrees not finite, a size other than 0 and outside
 * 8 .. 4096, a handle with a skybox.  A sample of a picture or a map handed over in memory that is not finite or negative is
 * PT_ERR_PARSE as in a file.  The conversion runs on one host thread and takes a double-precision acos, atan2 and root per
 * sub-sample, N^2 k^2 of them: a fraction of a second for a 2048 x 1024 picture (N = 1024, k = 2), on the order of ten seconds for
 * 8192 x 4096 at the default N = 2048 (k = 4); -ENV_SIZE / size trades that time for resolution.  params may be NULL: gain 1, no rotation, the default size.  A failed call leaves the handle as it was. */
typedef struct pt_environment_params {
    float gain;
    float rotate_y_degrees;
    int32_t size; /* 0 = default */
} pt_environment_params;

/* NULL or "" removes the environment. */
int pt_scene_set_environment_file(pt_scene *scene, const char *path, const pt_environment_params *params);
int pt_scene_set_environment_equirect(pt_scene *scene, int32_t w, int32_t h, const float *rgb, const pt_environment_params *params);
/* An octahedral map given directly: n x n x 3. */
int pt_scene_set_environment_map(pt_scene *scene, int32_t n, const float *rgb);
/* *n = the map's size, 0 without an environment; rgb (may be NULL) gets its n x n x 3 floats. */
int pt_scene_get_environment(const pt_scene *scene, int32_t *n, float *rgb);
/* The same on a frame: every device's copy of the frame's scene takes the map, which is read and converted once; a refused call
 * changes none of them.  pt_frame_get_environment answers for the root device's copy. */
int pt_frame_set_environment_file(pt_frame *frame, const char *path, const pt_environment_params *params);
int pt_frame_set_environment_equirect(pt_frame *frame, int32_t w, int32_t h, const float *rgb, const pt_environment_params *params);
int pt_frame_set_environment_map(pt_frame *frame, int32_t n, const float *rgb);
int pt_frame_get_environment(pt_frame *frame, int32_t *n, float *rgb);
/* The conversion alone, on the host: map_rgb gets n x n x 3 floats (n in 8 .. 4096; params->size is checked and not used). */
int pt_environment_from_equirect(int32_t w, int32_t h, const float *rgb, const pt_environment_params *params, int32_t n, float *map_rgb);
/* The lookup alone, on the host: rgb[3 i ..] = L(directions[3 i ..]). */
int pt_environment_lookup(int32_t n, const float *map_rgb, int32_t n_dirs, const float *directions, float *rgb);

/* ---- dielectric materials: refraction and Fresnel reflection (glass) ------------------------------------------------ */

/* A scene handle may carry a list of DIELECTRICS.  It marks some of the scene's materials, addressed by index as usemtl addresses
 * them, as smooth dielectrics: each entry has the material's index, a refractive index ior in 0.125 .. 8 (ior < 1: an air pocket seen
 * from inside the denser medium; ior == 1 is allowed) and a transmission tint, each component in 0 .. 1.  A marked material is a
 * dielectric and nothing else: the integrator does not look at its MTL lobes (Kd, Ks, Ns).  Without a list every output is what it was,
 * and the launches go to the kernels they went to.
 *
 * The list belongs to the handle, as a skybox or an environment does: pt_scene_clone_to_device and pt_frame_create inherit it.  It
 * works with every view, with a skybox, an environment or neither, with statistics, adaptive sampling and pass windows, in bands and
 * frames, on small and box-tree scenes; launches are planned as without the list (the same tiles and chunks).  The diagnostic builds
 * (phase timers, block profile) have no dielectric kernels: a render of a handle with a list is PT_ERR_UNSUPPORTED there.
 * The first-hit feature pass, the temporal reprojection and every display stage are unchanged: a dielectric pixel's features are what
 * its material's MTL fields give without the list.
 *
 * THE SHADING STEP of a segment whose ray (unit direction d, origin o) hits a triangle of a dielectric material at distance t.  N is
 * the triangle's stored unit normal, p = o + d * t (per component, one product and one sum), col the path's throughput, eps the
 * render's eps.  Every operation is a float operation rounded once, in the order written; nothing is fused; the root is correctly
 * rounded, the divisions are IEEE divisions.  inv_ior = 1.0f / ior is formed once on the host.
 *   c  = (N.x * d.x + N.y * d.y) + N.z * d.z
 *   if c < 0:  n = N,   ci = -c,  eta = inv_ior        (entering)
 *   else:      n = -N,  ci = c,   eta = ior            (leaving)
 *   ci = ci < 1 ? ci : 1
 *   s2 = (eta * eta) * (1 - ci * ci)
 *   if !(s2 < 1):  F = 1                               (total internal reflection)
 *   else:          ct = sqrt(1 - s2)
 *                  rs = (eta * ci - ct) / (eta * ci + ct)
 *                  rp = (ci - eta * ct) / (ci + eta * ct)
 *                  F  = 0.5 * (rs * rs + rp * rp)      (unpolarised Fresnel reflectance)
 *   u = ((w3 >> 9) << 1 | 1) * 2^-24                   (w3: the fourth word of the segment's own Philox call, whose first three
 *                                                       words serve the lobes; u is the unit float every lobe uses)
 *   if u < F:  r = d + n * (2 * ci),                 origin = p + n * eps,  col unchanged            (reflected)
 *   else:      r = d * eta + n * (eta * ci - ct),    origin = p - n * eps,  col *= (tr, tg, tb)      (transmitted)
 *   per component: r.x = d.x + n.x * (2 * ci), r.x = d.x * eta + n.x * (eta * ci - ct), origin.x = p.x + n.x * eps (or -), likewise y, z.
 *   direction = r / |r| as every scattered ray is normalised: r * (1 / sqrt((r.x * r.x + r.y * r.y) + r.z * r.z)); depth + 1.
 * The transmitted direction is the reference's own Refract (main.cpp:35-47) with eta in place of its constant.  A dielectric hit
 * never contributes.  On a path's last segment (depth + 1 == max_ray_reflections) nothing of this is computed, as for the other
 * scattering lobes, and the Philox call is made under the condition it is made under without the list.  There is no eta^2 radiance
 * scaling and no absorption along the interior path: the tint is applied per transmission.
 *
 * PT_ERR_INVALID_ARGUMENT: a NULL handle, a NULL list with n > 0, n < 0, a material index outside the scene, an index listed twice,
 * ior not finite or outside 0.125 .. 8, a tint component not finite or outside 0 .. 1, a material with an emissive lobe.  A setter
 * validates, builds and uploads first and swaps last: a refused call leaves the handle as it was.  A host-only scene (device < 0)
 * accepts and returns the list. */
typedef struct pt_dielectric {
    int32_t material;
    float ior;
    float tint[3];
} pt_dielectric;

/* NULL or n == 0 clears the list. */
int pt_scene_set_dielectrics(pt_scene *scene, const pt_dielectric *list, int32_t n);
/* *n = the number of entries (0 without a list); list (may be NULL) gets them, in the order given. */
int pt_scene_get_dielectrics(const pt_scene *scene, pt_dielectric *list, int32_t *n);
/* The same on a frame: every device's copy of the frame's scene takes the list; a refused call changes none of them.
 * pt_frame_get_dielectrics answers for the root device's copy. */
int pt_frame_set_dielectrics(pt_frame *frame, const pt_dielectric *list, int32_t n);
int pt_frame_get_dielectrics(pt_frame *frame, pt_dielectric *list, int32_t *n);

/* ---- albedo textures: texture coordinates, map_Kd and texture lists ------------------------------------------------- */

/* A scene handle may carry TEXTURE COORDINATES, three (u, v) pairs per triangle in the order of its vertices -- 6 x n_tri floats,
 * u0 v0 u1 v1 u2 v2 per triangle, triangles in the order the scene holds them -- and, with them, a list of TEXTURES.  An entry of the
 * list gives one material, addressed by index as usemtl addresses it, a picture of width x height texels: linear RGB floats, three
 * per texel, rows top-down (row 0 is the top of the picture, where v = 1), each finite and >= 0, and a filter.  Without a list every
 * output is what it was and the launches go to the kernels they went to; coordinates alone change nothing.
 *
 * Both belong to the handle, as the dielectrics do: pt_scene_clone_to_device and pt_frame_create inherit them.  A list works with
 * every view, with a skybox, an environment or neither, with dielectrics on other materials, with statistics, adaptive sampling and
 * pass windows, in bands and frames, on small and box-tree scenes; launches are planned as without the list (the same tiles and
 * chunks; the cull tables, ray origins and directions are untouched).  The diagnostic builds (phase timers, block profile) have no
 * texture kernels: a render of a handle with a list is PT_ERR_UNSUPPORTED there.
 *
 * THE SHADING STEP of a segment whose ray (unit direction d, origin o) hits triangle T (vertices v0, v1, v2 as the scene stores
 * them, corner coordinates (u0, v0') (u1, v1') (u2, v2')) of a textured material at distance t, after the lobe has been chosen as
 * without the list (unit_float(w0) - chance0 > 0 picks the second lobe; a one-lobe material draws nothing).  Every operation is a
 * float operation rounded once, in the order written; nothing is fused; the divisions are IEEE divisions.
 *   If the chosen lobe is the EMISSIVE or the DIFFUSE one:  col *= texel(T, p)  per channel (one rounding each), where col is the
 *   path's throughput entering the step and p = o + d * t (per component, one product and one sum).  Then the material's step runs
 *   unchanged on that throughput.  The GLOSSY lobe is not textured; a dielectric is not (a material cannot be in both lists).  On a
 *   path's last segment (depth + 1 == max_ray_reflections) only the emissive case computes anything.  No random number is drawn and
 *   none moves.
 * BARYCENTRICS of p, from a per-triangle RECORD of eight floats (a1.x a1.y a1.z c1 a2.x a2.y a2.z c2) that the host forms once per
 * triangle from its vertices, in plain float, every operation rounded once, nothing fused, component-wise differences first:
 *   e1 = v1 - v0,  e2 = v2 - v0
 *   d11 = (e1.x * e1.x + e1.y * e1.y) + e1.z * e1.z,   d12 likewise of e1, e2,   d22 of e2, e2
 *   den = d11 * d22 - d12 * d12
 *   den == 0 (a collinear triangle):  the record is all zero;   else, per component k,
 *     a1.k = (e1.k * d22 - e2.k * d12) / den,     a2.k = (e2.k * d11 - e1.k * d12) / den
 *     c1 = -((a1.x * v0.x + a1.y * v0.y) + a1.z * v0.z),     c2 likewise of a2
 * and at a hit
 *   b1 = ((a1.x * p.x + a1.y * p.y) + a1.z * p.z) + c1,    b2 = ((a2.x * p.x + a2.y * p.y) + a2.z * p.z) + c2
 *   (so den == 0 gives b1 = b2 = 0; a record that overflowed gives NaN or inf coordinates, which the wrap below sends to 0)
 *   b0 = (1 - b1) - b2
 *   u = (b0 * u0 + b1 * u1) + b2 * u2,    v = (b0 * v0' + b1 * v1') + b2 * v2'
 * LOOKUP of (u, v) in a width x height texture.  Repeat wrap on both axes: wrap(x) = x - floor(x) if that lies in [0, 1), else 0
 * -- so NaN and +-inf read as 0, and so does a negative x so small that the difference rounds to 1 (-1e-9); a magnitude of 2^23 or
 * more is its own floor and reads as 0 as well.  v points up, as OBJ has it: picture row = height - 1 - y.  Per axis of n texels,
 * with f = wrap(.) and x = f * n (in [0, n]):
 *   PT_TEXTURE_NEAREST   i = min(int(x), n - 1); the texel (i_u, i_v).
 *   PT_TEXTURE_BILINEAR  texel centres lie at (i + 0.5) / n:  c = x - 0.5,  i = floor(c) (-1 .. n - 1),  t = c - i;  the lower
 *                        texel is i, or n - 1 for i = -1; the upper one is i + 1, or 0 for i + 1 = n.  With lerp(a, b, t) =
 *                        a + (b - a) * t:  texel = lerp(lerp(t00, t10, tu), lerp(t01, t11, tu), tv)  per channel, where t10 is the
 *                        upper texel in u and t01 the upper one in v.  At a texel centre this is the texel; a constant texture
 *                        gives its constant everywhere.
 * Every float (u, v) therefore reads inside the texture and yields no NaN the texels do not hold: wrap(NaN) = wrap(+-inf) = 0 reads,
 * nearest, the bottom-left texel (0, 0) and, bilinear, the equal-weight mix of the four corner texels.  There are no mip maps (the
 * integrator has no ray footprints; the sample count does the filtering), no normal, specular or emission maps (map_Ke), no clamp or
 * mirror wrap and no texture transforms.
 *
 * THE FIRST-HIT FEATURE PASS of a handle with a list writes albedo = Kd * texel(T, p) per channel (one rounding), with p and the
 * lookup as above, for a pixel whose first hit is a triangle of a textured material, whatever its lobes; position, normal and hit
 * index are what they are without the list.  The denoiser and the upsampler therefore demodulate by the textured albedo.
 *
 * PT_ERR_INVALID_ARGUMENT: a NULL handle; a NULL list with n > 0, n < 0; a material index outside the scene or listed twice; width
 * or height < 1 or above PT_TEXTURE_MAX_SIDE, or more than 2^28 texels in one list; NULL texels; a texel that is not finite or is
 * negative; an unknown filter; a material that is a dielectric of the handle (pt_scene_set_dielectrics refuses a textured material
 * in turn); a list on a handle without texture coordinates; clearing the coordinates while a list is set; coordinates for a scene
 * without triangles.  Coordinates may hold any float.  A setter validates, builds and uploads first and swaps last: a refused call
 * leaves every handle as it was.  A host-only scene (device < 0) accepts and returns both. */
#define PT_TEXTURE_NEAREST 0
#define PT_TEXTURE_BILINEAR 1
#define PT_TEXTURE_MAX_SIDE 8192
typedef struct pt_texture {
    int32_t material;
    int32_t width, height;
    int32_t filter;      /* PT_TEXTURE_NEAREST or PT_TEXTURE_BILINEAR */
    const float *rgb;    /* width * height * 3; the setter copies them */
} pt_texture;

/* uv: 6 * n_tri floats (n_tri as pt_scene_counts gives it); NULL clears.  pt_scene_load_obj gives a loaded scene the OBJ's own: the
 * vt of each face corner, (0, 0) for a corner without one (a vt index beyond the vt lines read so far is PT_ERR_PARSE; in a file without
 * any vt line the index means nothing, as to the reference, and the corner gets (0, 0); a negative -- OBJ's relative -- or zero vt index is
 * not supported and reads as no index: (0, 0)). */
int pt_scene_set_texcoords(pt_scene *scene, const float *uv);
/* *has = 1 and uv (may be NULL) gets the 6 * n_tri floats, or *has = 0. */
int pt_scene_get_texcoords(const pt_scene *scene, float *uv, int32_t *has);
/* NULL or n == 0 clears the list. */
int pt_scene_set_textures(pt_scene *scene, const pt_texture *list, int32_t n);
/* *n = the number of entries; list (may be NULL) gets them in the order given, each rgb pointing at the handle's own copy of the
 * texels, valid until the list is replaced or the handle destroyed. */
int pt_scene_get_textures(const pt_scene *scene, pt_texture *list, int32_t *n);
/* The same on a frame: every device's copy of the frame's scene; a refused call changes none.  The getters answer for the root's. */
int pt_frame_set_texcoords(pt_frame *frame, const float *uv);
int pt_frame_get_texcoords(pt_frame *frame, float *uv, int32_t *has);
int pt_frame_set_textures(pt_frame *frame, const pt_texture *list, int32_t n);
int pt_frame_get_textures(pt_frame *frame, pt_texture *list, int32_t *n);
/* The file name the model's MTL gives material `material` in a map_Kd line (the last token of the line), "" if it has none or the
 * scene was made from arrays; the pointer stays valid as long as the scene.  The library applies nothing by itself (the reference
 * ignores the line): see pt_render -TEXTURE mtl.  PT_ERR_INVALID_ARGUMENT: NULL, or an index outside the scene. */
int pt_scene_get_map_kd(const pt_scene *scene, int32_t material, const char **name);
/* The barycentrics' records the kernels read, as stated above: records gets 8 * n_tri floats, triangles in the scene's order.  They
 * depend on the vertices alone; a host-only scene answers too. */
int pt_scene_get_texture_records(const pt_scene *scene, float *records);
/* Reads a 24-bit BMP (the skybox's reader) into linear floats for a pt_texture: texel = table[byte], table[b] = (float)pow(b / 255.0,
 * gamma) in the host's double pow (gamma == 1: b / 255.0 rounded to float), rows top-down, R G B.  gamma <= 0 or not finite: 2.2.
 * Call once with rgb == NULL for *width and *height, then with room for width * height * 3 floats.  PT_ERR_IO: the file cannot be
 * opened; PT_ERR_PARSE: not a 24-bit BMP, or a side above PT_TEXTURE_MAX_SIDE. */
int pt_texture_load_bmp(const char *path, float gamma, int32_t *width, int32_t *height, float *rgb);
/* The lookup alone, on the host: out_rgb[3 i ..] = texel at (uv[2 i], uv[2 i + 1]) of the width x height texture rgb.  indices (may
 * be NULL) gets, four per lookup, the texel indices (row * width + column, rows top-down) read: t00, t10, t01, t11 (nearest: the
 * one texel four times). */
int pt_texture_lookup(int32_t width, int32_t height, const float *rgb, int32_t filter, int32_t n, const float *uv, float *out_rgb, int32_t *indices);

/* ---- smooth shading: per-corner shading normals ------------------------------------------------------------------- */

/* A scene handle may carry SHADING NORMALS: nine floats per triangle -- n0, n1, n2 for its three corners in the order of its vertices
 * -- triangles in the order the scene holds them.  Without them every output is what it was and the launches go to the kernels they
 * went to.  They belong to the handle, as the dielectrics and the textures do: pt_scene_clone_to_device and pt_frame_create inherit
 * them.  They work with every view, with a skybox, an environment or neither, with dielectrics and textures, with statistics,
 * adaptive sampling and pass windows, in bands and frames, on small and box-tree scenes; launches are planned as without them (the
 * same tiles and chunks).  Only directions change: ray origins, the geometry and the cull tables are untouched.  The diagnostic builds
 * (phase timers, block profile) have no smooth kernels: a render of a handle with shading normals is PT_ERR_UNSUPPORTED there.
 *
 * Every operation below is a float operation rounded once, in the order written; nothing is fused; normalize3(v) is
 * v * (1 / sqrt((v.x * v.x + v.y * v.y) + v.z * v.z)) with the correctly rounded root and division every scattered ray is normalised with.
 *
 * THE SHADING NORMAL Ns at a hit on triangle T at point p = o + d * t, with stored plane normal N:
 *   b1, b2 from T's barycentric record exactly as the albedo textures state them (BARYCENTRICS above), not clamped;  b0 = (1 - b1) - b2
 *   m = (b0 * n0 + b1 * n1) + b2 * n2  per component,      l = (m.x * m.x + m.y * m.y) + m.z * m.z
 *   l not finite or not > 0:  Ns = N          (all-zero normals are the documented "use N"; so are corners that cancel)
 *   else                      Ns = normalize3(m)
 *   ((Ns.x * N.x + Ns.y * N.y) + Ns.z * N.z) < 0:  Ns = -Ns  (exact)
 * THE SHADING STEP.  The lobe is chosen and the texel step runs as without the normals (it shares the record).  The EMISSIVE lobe is
 * unchanged: it tests facing against N.  The GLOSSY lobe (reflection), the DIFFUSE lobe (hemisphere flip and cosine factor) and the
 * DIELECTRIC step (c, entering, Fresnel, both directions) run with Ns wherever they use the normal without shading normals.  The
 * next ray's ORIGIN is still p + N * oe, with the oe the step chose: +eps, or +-eps for a dielectric.  The origin never uses Ns.
 * FALLBACK.  Let r be the step's new direction after its final normalize3.  If !(((r.x * N.x + r.y * N.y) + r.z * N.z) * oe > 0) --
 * the direction leaves on the other side of the stored plane from the origin's offset -- the whole step is the step made with
 * Ns = N instead: the step of a handle without shading normals, bit for bit.  No random number is drawn or moved; the same w1 .. w3
 * are used.  On a path's last segment nothing new is computed.
 * THE FIRST-HIT FEATURE PASS of a handle with shading normals writes normal = Ns of the first hit, after the flip and before any
 * fallback; position, hit index and albedo (Kd x texel with a texture list) are what they are without.
 *
 * Not built: normal maps, and per-material smoothing groups (the OBJ's `s` lines).
 *
 * PT_ERR_INVALID_ARGUMENT: a NULL handle; a component that is not finite; normals for a scene without triangles.  Zeros are allowed.
 * A setter validates and uploads first and swaps last: a refused call leaves every handle as it was.  A host-only scene (device < 0)
 * accepts and returns them. */
/* n9: 9 * n_tri floats (n_tri as pt_scene_counts gives it); NULL clears. */
int pt_scene_set_shading_normals(pt_scene *scene, const float *n9);
/* *has = 1 and n9 (may be NULL) gets the 9 * n_tri floats, or *has = 0. */
int pt_scene_get_shading_normals(const pt_scene *scene, float *n9, int32_t *has);
/* What pt_scene_load_obj kept of the file: the vn of each face corner as the file gives it (not normalised), the face's stored normal
 * for a corner without a vn index (none, zero or negative).  *has = 0 for a scene made from arrays.  The library applies nothing by
 * itself: a loaded scene renders as before until the caller passes normals to pt_scene_set_shading_normals.  A vn index beyond the
 * vn lines read so far is PT_ERR_PARSE, on every corner. */
int pt_scene_get_vertex_normals(const pt_scene *scene, float *n9, int32_t *has);
/* The same on a frame: every device's copy of the frame's scene; a refused call changes none.  The getter answers for the root's. */
int pt_frame_set_shading_normals(pt_frame *frame, const float *n9);
int pt_frame_get_shading_normals(pt_frame *frame, float *n9, int32_t *has);
/* The normal generator, on the host: out gets 9 floats per triangle from vertices (9 per triangle: v0, v1, v2).  Corners whose positions
 * are bit-identical are one vertex.  A corner's normal is the sum, over the triangles at its vertex whose geometric face normal g
 * satisfies f . g >= cos(crease_degrees) for the corner's own face normal f (its own face always counts), of g times the triangle's
 * interior angle at that vertex (acos of the clamped cosine), normalised; accumulated in double, rounded to float last.  A degenerate
 * triangle (no area, or a vertex that is not finite) contributes nothing and receives zeros; so does a corner whose sum has no
 * length.  Checked to a tolerance, not bit for bit.  PT_ERR_INVALID_ARGUMENT: NULL, n_tri < 0, a crease outside 0 .. 180. */
#define PT_SMOOTH_DEFAULT_CREASE 60.0f
int pt_smooth_normals(int32_t n_tri, const float *vertices, float crease_degrees, float *out);
/* pt_scene_load_obj with flags.  PT_LOAD_GEOMETRIC_PLANES: every face's plane comes from the cross product c of its edges (what a face
 * without a vn index gets), not from the vn its first corner names -- the reference takes the plane from that vn, which tilts the planes
 * of a file with true vertex normals.  The vn still chooses the side: where the first corner names a vn and (c . vn) < 0 (float, the
 * three products summed left to right), the plane is made from -c, so a face whose winding disagrees with its normals (the lamp of
 * models/Tor.obj) faces the way the file says, as it does without the flag.  A face without a vn index keeps c.  Flags 0 is
 * pt_scene_load_obj.  An unknown flag is PT_ERR_INVALID_ARGUMENT. */
#define PT_LOAD_GEOMETRIC_PLANES 1u
int pt_scene_load_obj_ex(const char *model_dir, const char *model_name, int device, uint32_t flags, pt_scene **out);
/* The interpolation alone, on the host, for n points on one triangle: vertices = v0, v1, v2 (9 floats), plane_normal = N (3), normals =
 * n0, n1, n2 (9); out[3 i ..] = Ns at points[3 i ..] as stated above (the record is formed from the vertices as the textures state
 * it); interpolated (may be NULL) gets 1 where Ns came from m and 0 where it is N. */
int pt_shading_normal_at(const float *vertices, const float *plane_normal, const float *normals, int32_t n, const float *points, float *out,
                         int32_t *interpolated);

/* ---- rough specular: a GGX glossy lobe ------------------------------------------------------------------------------ */

/* A scene handle may carry a ROUGHNESS LIST: entries (material, alpha).  Where a ray hits a listed material and the glossy lobe is
 * chosen, the new direction is the reflection about a microfacet normal drawn from the GGX distribution of the normals visible from
 * the incoming direction (Heitz 2018, "Sampling the GGX distribution of visible normals"), and the throughput factor is Ks x G1(l)
 * with the separable Smith term of the new direction l.  A material that is not listed keeps the mirror reflect(d, N), bit for bit;
 * without a list every output is what it was and the launches go to the kernels they went to.  The list belongs to the handle, as the
 * dielectrics do: pt_scene_clone_to_device and pt_frame_create inherit it.  It works with every view, miss shader, dielectrics,
 * textures and shading normals, with statistics, adaptive sampling and pass windows, in bands and frames, on small and box-tree
 * scenes; launches are planned as without it.  Only the glossy lobe's direction and factor change: the lobe choice, the condition
 * under which the segment's random words are drawn, the emissive and the diffuse lobe, dielectrics, texel steps, ray origins, the
 * geometry and the cull tables are untouched, and so are the first-hit feature pass and the denoiser.  The diagnostic builds (phase
 * timers, block profile) have no rough kernels: a render of a handle with a list is PT_ERR_UNSUPPORTED there.
 *
 * THE STEP, for a ray of unit direction d that hit a listed material of roughness alpha at p, with the words w1, w2 of the segment
 * (the glossy lobe leaves them unused; no other word is used or moves) and n = the normal the glossy lobe would use: the stored N, or
 * Ns under shading normals.  Every operation is a float operation rounded once, in the order written; nothing is fused; sqrt and /
 * are correctly rounded; dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z; normalize3 as above; unit_float(w) = float(((w >> 9) << 1)
 * | 1) * 2^-24; sincos is the portable one of the diffuse lobe (double +, -, * only).
 *   c = dot(n, d);   c > 0: n = -n  (exact: n is turned to the side the ray came from)
 *   the tangent frame of Duff et al. 2017:  s = copysign(1, n.z);   a = -1 / (s + n.z);   b = (n.x * n.y) * a
 *     t1 = (1 + ((s * n.x) * n.x) * a,  s * b,  -(s * n.x));     t2 = (b,  s + (n.y * n.y) * a,  -n.y)
 *   v = -d in (t1, t2, n):  v.x = -dot(t1, d),  v.y = -dot(t2, d),  v.z = |c|
 *   stretched:  e = normalize3(alpha * v.x, alpha * v.y, v.z)
 *   q = e.x * e.x + e.y * e.y;   q >= 2^-40:  iq = 1 / sqrt(q),  T1 = (-(e.y * iq), e.x * iq, 0);   else T1 = (1, 0, 0)
 *   T2 = (-(e.z * T1.y),  e.z * T1.x,  e.x * T1.y - e.y * T1.x)
 *   u1 = unit_float(w1), u2 = unit_float(w2);   r = sqrt(u1);   (sn, cs) = sincos((2 * 3.141593f) * u2);   p1 = r * cs,  p2 = r * sn
 *   the hemisphere warp:  w = 0.5 * (1 + e.z);   p2 = (1 - w) * sqrt(max(1 - p1 * p1, 0)) + w * p2
 *   p3 = sqrt(max((1 - p1 * p1) - p2 * p2, 0))
 *   m.x = (p1 * T1.x + p2 * T2.x) + p3 * e.x;   m.y = (p1 * T1.y + p2 * T2.y) + p3 * e.y;   m.z = p2 * T2.z + p3 * e.z
 *   the stretch undone:  h = normalize3(alpha * m.x, alpha * m.y, max(m.z, 0))      (the microfacet normal in (t1, t2, n))
 *   H = (h.x * t1 + h.y * t2) + h.z * n  per component;   dh = dot(H, d)
 *   l = normalize3(d - H * dh * 2)  per component, as the mirror's:  d.x - (H.x * dh) * 2
 *   nl = dot(n, l);   nl > 0:  a2 = alpha * alpha,  g = (2 * nl) / (nl + sqrt(a2 + (1 - a2) * (nl * nl))),  G1 = min(g, 1);   else G1 = 0
 *   (max(x, 0) is x > 0 ? x : 0 and min(g, 1) is g < 1 ? g : 1.)
 * The new direction is l, the throughput is multiplied by Ks * G1 per channel, and the next ray's origin is p + N * eps with the
 * stored N, as the mirror's.  G1 = 0 gives a zero throughput, which ends the path by the rule that ends every path.  Under shading
 * normals the existing rule holds as it is: the step with Ns and the step with N are both made from the same words, and the fallback
 * test on the first one's direction selects.
 *
 * Not built: rough dielectrics, anisotropy, a Fresnel term on Ks, roughness textures.
 *
 * PT_ERR_INVALID_ARGUMENT: a NULL handle; a negative count; a material outside the model; a material listed twice; an alpha that is
 * not finite or outside PT_ROUGH_ALPHA_MIN .. PT_ROUGH_ALPHA_MAX; a material without a glossy lobe (Ns == 0, Ks == 0, or emissive); a
 * material the handle's dielectric list holds -- and pt_scene_set_dielectrics refuses a material of the roughness list in turn.  A
 * setter validates, builds and uploads first and swaps last: a refused call leaves every handle as it was.  A host-only scene
 * (device < 0) accepts and returns a list. */
#define PT_ROUGH_ALPHA_MIN 0.0009765625f /* 2^-10 */
#define PT_ROUGH_ALPHA_MAX 1.0f
typedef struct pt_rough {
    int32_t material;
    float alpha;
} pt_rough;
/* n == 0 (or list == NULL) clears. */
int pt_scene_set_roughness(pt_scene *scene, const pt_rough *list, int32_t n);
/* *n = the number of entries; list (may be NULL) gets them in the order given. */
int pt_scene_get_roughness(const pt_scene *scene, pt_rough *list, int32_t *n);
/* The same on a frame: every device's copy of the frame's scene; a refused call changes none.  The getter answers for the root's. */
int pt_frame_set_roughness(pt_frame *frame, const pt_rough *list, int32_t n);
int pt_frame_get_roughness(pt_frame *frame, pt_rough *list, int32_t *n);
/* What pt_scene_load_obj kept of the MTL: pr[m] = the value of material m's `Pr` line as the file gives it (not clamped), or -1 where
 * it has none (or one that is not a finite number, or the scene was made from arrays).  pr: n_mat floats.  The library applies
 * nothing by itself. */
int pt_scene_get_mtl_roughness(const pt_scene *scene, float *pr);
/* THE STEP alone, on the host, for n rays: normals, directions (3 n floats, unit length), alpha, w1, w2 (n each) give
 * out_directions (3 n: l), out_g1 (n) and, where out_microfacet is not NULL, h (3 n).  An alpha outside the range is refused. */
int pt_rough_step(int32_t n, const float *normals, const float *directions, const float *alpha, const uint32_t *w1, const uint32_t *w2,
                  float *out_directions, float *out_g1, float *out_microfacet);

/* ---- direct lighting: a shadow ray to the emitters at every diffuse hit ----------------------------------------------- */

/* A scene handle may have DIRECT LIGHTING switched on (next-event estimation).  Without it a path finds light only when its scattered
 * ray happens to strike an emissive triangle; with it every scattering diffuse hit also sends one shadow ray to a sampled point of a
 * light, and the emitters that ray has sampled are not counted a second time when the diffuse lobe's own ray reaches one.  The
 * switch belongs to the handle, as the roughness list does: pt_scene_clone_to_device and pt_frame_create inherit it and the table.  It
 * works with every view, miss shader, dielectrics, textures, shading normals and roughness, with statistics, adaptive sampling and
 * pass windows, in bands and frames, on small and box-tree scenes; launches are planned as without it.  Without the switch every
 * output is what it was and the launches go to the kernels they went to.  The first-hit feature pass, the denoiser, the temporal
 * merge, the upsampler and the display chain read sum / count as before.  The diagnostic builds (phase timers, block profile) have
 * no direct kernels: a render of a handle with the switch on is PT_ERR_UNSUPPORTED there.
 *
 * PER-PATH ACCOUNTING.  Under direct lighting a path collects its radiance in L = (Lr, Lg, Lb), which starts at +0; every term is
 * added channel by channel in the order the terms occur.  Every traced path updates the accumulators exactly once, when it ends --
 * a miss, an emitter, a material without lobes, the depth cap or a throughput of zero --: sum += L, sum2 += L * L, count += 1.  count
 * is then the number of paths traced and sum / count the unbiased pixel estimate (without the switch, count is the number of
 * contributing paths and sum / count a conditional mean).  A pixel's paths still end in pass order.
 *
 * THE LIGHT TABLE.  A light is a triangle of non-zero area whose material is the single emissive lobe (Ke != 0); lights are kept in the
 * original triangle order.  Per light: v0;  e1 = v1 - v0 and e2 = v2 - v0 as float differences;  Nl, the stored plane normal;  Le, the
 * material's Kd (what the emissive lobe multiplies the throughput by);  the triangle's original index;  cdf.  area_i = 0.5 * sqrt((cx *
 * cx + cy * cy) + cz * cz) in double with c = e1 x e2 formed in double from the float edges (c.x = e1.y * e2.z - e1.z * e2.y, and so
 * on); a triangle whose area is not > 0 is no light.  The areas are summed in double in table order, total first; then cum_i likewise,
 * cdf_i = float(cum_i / total), the last entry forced to 1.0f, and A = float(total).
 *
 * THE DIRECT TERM, at a hit where the diffuse lobe is chosen by a ray that scatters (depth + 1 < mrr), after the texel step and
 * before the throughput takes the lobe's factor.  Every operation is a float operation rounded once, in the order written; nothing is
 * fused; sqrt and / are correctly rounded; dot, normalize3 and unit_float as above.
 *   (l0, l1, l2, l3) = philox(pixel, pass, depth, 3): the fourth counter word is 3.  Every other call of the integrator -- the segment's
 *     words, the jitter and the lens (depth 0xFFFFFFFF), the shutter time (0xFFFFFFFE) -- has 0 there, and the display's dither and
 *     grain, which run under the same key, have 1 and 2 (pt_grain), so 1 is not free and these words are used by nothing else; the segment's own w0 .. w3 stay as
 *     they are and no other random number moves.
 *   i = the first light with unit_float(l0) < cdf_i
 *   u1 = unit_float(l1), u2 = unit_float(l2);   u1 + u2 > 1:  u1 = 1 - u1, u2 = 1 - u2  (exact for multiples of 2^-24)
 *   P = (v0 + e1 * u1) + e2 * u2  per component
 *   O = p + N * eps, the origin the next ray gets;   w = P - O;   r2 = (w.x * w.x + w.y * w.y) + w.z * w.z;   omega = normalize3(w)
 *   cn = dot(N, omega);   cs = dot(n, omega) with n = Ns of the hit point under shading normals (flipped onto N's side; N where the
 *     triangle has no usable Ns), else N;   cl = -dot(Nl, omega)
 *   no term and no shadow ray unless r2 > 0, cn > 0, cs > 0 and cl > 0
 *   g = (((cs * |omega.z|) * cl) * A) / (3.141593f * r2)
 *     (two factors on purpose: the diffuse lobe draws its direction cosine-weighted about the scene's z axis -- not about the normal --,
 *     turns it onto the normal's side and multiplies by n . omega, so the function it integrates is Kd (n . omega) |omega.z| / pi per
 *     solid angle, and the direct term has to integrate the same function or the two estimators disagree.  For a wall that faces along
 *     z this is Kd cos^2 / pi; for any other wall cs * cs is a different function, and the agreement test of tests/test_direct_host.py
 *     tells the two apart)
 *   term_c = ((T_c * Kd_c) * Le_c) * g  with T the throughput entering the lobe
 *   The term is added to L if and only if the closest hit of the ray (O, omega), found by the same search with the same eps, is light
 *   i's triangle.  No distance bound, no tolerance: a point on a shared edge that resolves to the neighbour counts as occluded.
 * NO DOUBLE COUNTING: a path carries one bit.  A diffuse step under direct lighting sets it (whether or not it had a term); a primary
 * ray clears it and so does every other scattering step (mirror, GGX, dielectric).  An emitter hit adds throughput x Kd to L only
 * when the bit is clear; the path ends there either way.  The skybox and the environment add to L as before, whatever the bit: they
 * are not sampled.  Glossy, rough and dielectric steps get no direct term.
 * Statistics under the switch: samples_traced, segments and misses count path segments only (no shadow ray); contributing counts the
 * terms added to any L.
 *
 * Not built: multiple importance sampling, sampling by power, direct terms for the GGX lobe, textured emitters.
 * (Sampling the environment and Russian roulette are switches of their own: environment sampling and Russian roulette, below.)
 *
 * PT_ERR_INVALID_ARGUMENT: a NULL handle; switching on for a scene without a light; switching on while an emissive material is in the
 * handle's texture list -- and pt_scene_set_textures refuses such a material in turn while the switch is on.  A setter builds and
 * uploads first and swaps last: a refused call leaves every handle as it was.  A host-only scene (device < 0) accepts the switch. */
typedef struct pt_light {
    float v0[3];
    float cdf;
    float e1[3];
    int32_t triangle; /* original index */
    float e2[3];
    float pad0;
    float normal[3]; /* Nl */
    float pad1;
    float le[3];
    float pad2;
} pt_light;
int pt_scene_set_direct_lighting(pt_scene *scene, int32_t on);
int pt_scene_get_direct_lighting(const pt_scene *scene, int32_t *on);
/* The light table the switch uses (or would use): *n = the number of lights, lights (may be NULL) gets them, *area (may be NULL) = A. */
int pt_scene_get_lights(const pt_scene *scene, pt_light *lights, int32_t *n, float *area);
/* The same on a frame: every device's copy of the frame's scene; a refused call changes none.  The getters answer for the root's. */
int pt_frame_set_direct_lighting(pt_frame *frame, int32_t on);
int pt_frame_get_direct_lighting(pt_frame *frame, int32_t *on);
int pt_frame_get_lights(pt_frame *frame, pt_light *lights, int32_t *n, float *area);
/* THE DIRECT TERM alone, on the host, without the visibility, for n hits: origins (O), normals (N), shading_normals (n), throughput
 * (T), kd (3 n floats each) and the words l0, l1, l2 (n each) give out_light (the table index i), out_points (P), out_directions
 * (omega), out_terms (3 n each; zero without a term) and out_has_term (n). */
int pt_direct_term(int32_t n, const pt_light *lights, int32_t n_lights, float area, const float *origins, const float *normals,
                   const float *shading_normals, const float *throughput, const float *kd, const uint32_t *l0, const uint32_t *l1,
                   const uint32_t *l2, int32_t *out_light, float *out_points, float *out_directions, float *out_terms, int32_t *out_has_term);

/* ---- environment sampling: shadow rays to the HDR environment ----------------------------------------------------------- */

/* A scene handle that has an environment (pt_scene_set_environment_*) may have ENVIRONMENT SAMPLING switched on.  Every scattering
 * diffuse hit then sends one shadow ray: with probability `share` to a direction drawn from the environment in proportion to its
 * radiance, otherwise to a point of the scene's emitters exactly as direct lighting does.  A diffuse-lobe ray that afterwards escapes
 * to the environment, or reaches an emitter, adds nothing: the bit of NO DOUBLE COUNTING above covers the miss too.  Accounting is
 * per path, as under direct lighting.  The switch belongs to the handle and is independent of pt_scene_set_direct_lighting, whose
 * value and refusals stay as they are; with both on this one picks the kernels.  Clones and a frame's copies inherit it with its
 * table.  It works with every view, dielectrics, textures, shading normals and roughness, with statistics, adaptive sampling and
 * pass windows, in bands and frames, on small and box-tree scenes; launches are planned as without it.  Without the switch every
 * output is what it was and the launches go to the kernels they went to.  The diagnostic builds (phase timers, block profile) have no
 * such kernels: a render of a handle with the switch on is PT_ERR_UNSUPPORTED there.
 *
 * THE TABLE is built on the host in double from the handle's N x N octahedral map, whenever the switch is set or the environment of
 * a switched-on handle is replaced.  S = min(N, 256); the table has S x S cells over the map's square q = (qx, qz) in [-1, 1]^2, cell
 * c = cj * S + ci with ci along qx.  k = max(2, ceil(2 N / S)).  For sub-point (si, sj), 0 <= si, sj < k, of cell (ci, cj):
 *   qx = 2 ((ci + (si + 0.5) / k) / S) - 1,  qz likewise with cj, sj;   py = 1 - |qx| - |qz|
 *   py >= 0: px = qx, pz = qz;  else px = copysign(1 - |qz|, qx), pz = copysign(1 - |qx|, qz)   (the unfold pt_environment_from_equirect uses)
 *   len = sqrt(px px + py py + pz pz);   L = THE LOOKUP (float) at direction (float(px / len), float(py / len), float(pz / len))
 *   f = ((0.2126 max(L.r, 0) + 0.7152 max(L.g, 0)) + 0.0722 max(L.b, 0)) / ((len len) len)
 * f is summed over sj (outer) and si (inner); W_c = (4 / S^2) (sum / (k k)).  1 / |p|^3 is the exact Jacobian d omega / dq of the map
 * (p . (dp/dpx x dp/dpz) = -(|px| + py + |pz|) = -1 on the octahedron; the fold is a reflection in q and leaves it unchanged).
 * Phi_env = the sum of W_c in cell order; a map whose Phi_env is zero or not finite is refused.  Every cell then gets at least
 * Phi_env / S^2 / 16, so every cell has positive probability (a texel whose bilinear footprint reaches into a dark cell is still
 * sampled); P_c = W_c / (the sum of the floored W in cell order).
 * The alias table (Walker / Vose) of p_c = P_c S^2: the cells with p_c < 1 go on a stack `small` and the others on a stack `large`,
 * both in ascending cell order.  While neither is empty: s = pop(small), l = pop(large); accept_s = float(p_s), alias_s = l;
 * p_l = (p_l + p_s) - 1; l is pushed on small if p_l < 1, else on large.  Every cell never given an alias has accept 1 and is its own
 * alias.  pdf_self_c = float(P_c S^2 / 4), the probability per unit area of q; pdf_alias_c = pdf_self of the alias.  The probability
 * the table gives cell c, (accept_c + the sum of (1 - accept_j) over the other cells j whose alias is c) / S^2, differs from P_c by
 * the float rounding of those accepts: at most (1 + m_c) 2^-25 / S^2, m_c being the number of such j.
 *
 * SHARE.  A scene without emitters (an empty light table) has share = 1.  Otherwise the default is Phi_env / (Phi_env + Phi_em) with
 * Phi_em = 3.14159265358979323846 x the sum over THE LIGHT TABLE, in table order, of area_i ((0.2126 Le.r + 0.7152 Le.g) + 0.0722 Le.b),
 * all in double, rounded to float and clamped to [0.125, 0.875]; or the caller's value, 0 < share < 1.
 *
 * THE SAMPLE AND THE TERM, at a hit where the direct term would be formed.  Float operations rounded once in the order written,
 * nothing fused, sqrt and / correctly rounded.
 *   (l0, l1, l2, l3) = philox(pixel, pass, depth, 3) as under direct lighting.  The environment is chosen if and only if
 *     unit_float(l3) < share.  Otherwise THE DIRECT TERM is formed from l0, l1, l2 and each channel is divided by (1.0f - share).
 *   (e0, e1, e2, e3) = philox(pixel, pass, depth, 4), drawn where the environment is chosen.  No other random number moves.
 *   d = (uint64(e0) * S^2) >> 32;   unit_float(e1) < accept_d:  c = d, pdf_q = pdf_self_d;   else  c = alias_d, pdf_q = pdf_alias_d
 *   cj = c / S, ci = c - cj S;   cw = 2.0f / float(S)
 *   qx = (float(ci) + unit_float(e2)) * cw - 1.0f;   qz = (float(cj) + unit_float(e3)) * cw - 1.0f
 *   py = (1.0f - |qx|) - |qz|;   py >= 0: px = qx, pz = qz;  else px = copysign(1.0f - |qz|, qx), pz = copysign(1.0f - |qx|, qz)
 *   len = sqrt((px * px + py * py) + pz * pz);   w = normalize3(p);   pdf_w = pdf_q * ((len * len) * len)
 *   cn = dot(N, w);   cs = dot(n, w), n as in THE DIRECT TERM
 *   no term and no shadow ray unless cn > 0, cs > 0 and 0 < pdf_w < infinity
 *   L = THE LOOKUP at w, taken when the sample is drawn
 *   g = (cs * |w.z|) / ((3.141593f * pdf_w) * share);   term_c = ((T_c * Kd_c) * L_c) * g
 *   The shadow ray leaves O = p + N * eps; the term is added if and only if its closest hit is a miss.
 * Statistics as under direct lighting.  Not built: multiple importance sampling with the diffuse lobe, a term for the GGX lobe,
 * sampling emitters by power.
 *
 * PT_ERR_INVALID_ARGUMENT: a NULL handle; a handle without an environment; a map whose Phi_env is zero or not finite; a share outside
 * (0, 1) on a scene with emitters, or a share other than 0 or 1 on one without; an emissive material in the handle's texture list.
 * While the switch is on, pt_scene_set_environment_* rebuilds the table within the same call and changes nothing if the new map is
 * refused; removing the environment, setting a skybox and giving an emissive material a texture are refused.  A refused call leaves
 * every handle as it was. */
typedef struct pt_env_sampling {
    float share; /* 0 = the default */
} pt_env_sampling;
typedef struct pt_env_sample_record {
    float accept;
    int32_t alias;
    float pdf_self;
    float pdf_alias;
} pt_env_sample_record;
/* params NULL: the switch is cleared. */
int pt_scene_set_environment_sampling(pt_scene *scene, const pt_env_sampling *params);
/* *on = 0 or 1; params (may be NULL) gets what the setter was given. */
int pt_scene_get_environment_sampling(const pt_scene *scene, int32_t *on, pt_env_sampling *params);
/* The table the switch uses (or would use with the default share): *cells = S, records (may be NULL) gets S x S of them, *share (may be
 * NULL) the share in use.  A handle without an environment has *cells = 0. */
int pt_scene_get_environment_sampling_table(const pt_scene *scene, pt_env_sample_record *records, int32_t *cells, float *share);
/* The same on a frame: every device's copy of the frame's scene; a refused call changes none.  The getters answer for the root's. */
int pt_frame_set_environment_sampling(pt_frame *frame, const pt_env_sampling *params);
int pt_frame_get_environment_sampling(pt_frame *frame, int32_t *on, pt_env_sampling *params);
int pt_frame_get_environment_sampling_table(pt_frame *frame, pt_env_sample_record *records, int32_t *cells, float *share);
/* THE SAMPLE AND THE TERM alone, on the host, without the visibility, for n hits: a table of cells x cells records, the share, the
 * map_n x map_n x 3 map, normals (N), shading_normals (n), throughput (T), kd (3 n floats each) and the words e0 .. e3 (n each) give
 * out_cell (c), out_directions (w, 3 n), out_pdf (pdf_w), out_terms (3 n; zero without a term) and out_has_term (n). */
int pt_envdirect_term(int32_t n, const pt_env_sample_record *records, int32_t cells, float share, int32_t map_n, const float *map_rgb,
                      const float *normals, const float *shading_normals, const float *throughput, const float *kd, const uint32_t *e0,
                      const uint32_t *e1, const uint32_t *e2, const uint32_t *e3, int32_t *out_cell, float *out_directions, float *out_pdf,
                      float *out_terms, int32_t *out_has_term);

/* ---- Russian roulette: unbiased path termination under per-path accounting ------------------------------------------------- */

/* A scene handle that has direct lighting or environment sampling on may have RUSSIAN ROULETTE set: two parameters, `start`, an
 * integer >= 1, and `floor`, a float in [2^-10, 1].  From its start on, every scattering step ends a path with a probability that
 * follows its throughput and divides the survivors by the probability of surviving, so sum / count stays the unbiased estimate of
 * what the same handle renders without it at the same mrr, while the depth cap can be raised until it no longer matters.  The
 * parameters belong to the handle: pt_scene_clone_to_device and pt_frame_create inherit them.  It works with everything the two
 * switches work with; launches are planned as without it (tiles, pass chunks), and the closed-room wide and 8 x 8 kernels regenerate
 * paths as the skybox kernels do.  Without it every output is what it was and the launches go to the kernels they went to.  The
 * diagnostic builds (phase timers, block profile) have no such kernels: PT_ERR_UNSUPPORTED there.
 *
 * THE STEP runs at the end of a scattering step -- diffuse, mirror, GGX or dielectric alike --, after the throughput T has taken the
 * lobe's factor (tr *= fr; tg *= fg; tb *= fb) and before depth is incremented, if and only if depth + 1 >= start and a next ray will
 * be traced (depth + 1 < mrr: the condition the scattering step itself is under).  Float operations rounded once in the order written,
 * nothing fused, / correctly rounded:
 *   m = max(max(|tr|, |tg|), |tb|), a NaN propagating  (absolute values: a material may carry any Kd)
 *   !(m < 1.0f): the path survives unchanged  (a NaN lands here)
 *   p = m < floor ? floor : m
 *   (w0, ..) = philox(pixel, pass, depth, 5), depth as it is before the increment: the fourth counter word is 5 (0: the segment's, the
 *     jitter's and the shutter's words; 1, 2: the display's dither and grain; 3: the direct term; 4: environment sampling).  The call
 *     need only be made where the word is used, and no other random number moves.
 *   unit_float(w0) < p:  tr = tr / p; tg = tg / p; tb = tb / p  (three divisions, not a reciprocal)
 *   else:                tr = tg = tb = 0
 * A path with throughput zero is over: its L goes to the accumulators once, as PER-PATH ACCOUNTING says -- with the verdict of a
 * shadow ray the same hit left pending, where there is one.  The direct term of the same hit was formed from the throughput before
 * the lobe's factor and is not touched.  With start >= mrr the step never runs and the frame is the frame without roulette, bit for
 * bit.  Statistics as under direct lighting.
 *
 * Not built: multiple importance sampling, a survival probability from anything but the throughput (luminance, an estimate of the
 * radiance ahead), path splitting.
 *
 * PT_ERR_INVALID_ARGUMENT: a NULL handle; start < 0; a floor outside [2^-10, 1] or not finite (with start > 0); a handle with neither
 * direct lighting nor environment sampling on.  start == 0 clears (the floor is then not looked at).  While roulette is set, switching
 * off the last of the two switches is refused: clear the roulette first.  A refused call leaves every handle as it was. */
#define PT_ROULETTE_DEFAULT_FLOOR 0.0625f
int pt_scene_set_roulette(pt_scene *scene, int32_t start, float floor);
/* *start = 0 (not set) or the start; *floor (may be NULL) the floor, 0 where not set. */
int pt_scene_get_roulette(const pt_scene *scene, int32_t *start, float *floor);
/* The same on a frame: every device's copy of the frame's scene; a refused call changes none.  The getter answers for the root's. */
int pt_frame_set_roulette(pt_frame *frame, int32_t start, float floor);
int pt_frame_get_roulette(pt_frame *frame, int32_t *start, float *floor);
/* THE STEP alone, on the host, for n paths: throughput (3 n floats) and the words w0 (n) under `floor` give out_throughput (3 n) and
 * out_survives (n: 1 unless the step ended the path). */
int pt_roulette_step(int32_t n, float floor, const float *throughput, const uint32_t *w0, float *out_throughput, int32_t *out_survives);

/* ---- misc ------------------------------------------------------------------------------------------- */
int pt_abi_version(void);
int pt_device_count(void);
const char *pt_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PT_HIP_H */
