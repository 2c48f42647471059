"""MI355X radiance integrator: thin ctypes binding of libpt_hip.so (include/pt_hip.h).

The product is the C ABI; this module only loads it for the Python-side harnesses (tests, bench.py, smoke).
There is no CPU fallback: if the shared library is missing, or no HIP device is usable, calls raise.

The directory name contains a hyphen, so import it with
    importlib.import_module("path-tracing_amd")
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC_DIR = os.path.join(_HERE, "csrc")
# PT_HIP_LIB selects another build of the same ABI (kernel-variant experiments); the default is the in-tree library.
LIB_PATH = os.environ.get("PT_HIP_LIB") or os.path.join(_HERE, "lib", "libpt_hip.so")

PT_OK = 0
PT_ERR_INVALID_ARGUMENT, PT_ERR_UNSUPPORTED = 1, 7
STATUS_NAMES = {0: "PT_OK", 1: "PT_ERR_INVALID_ARGUMENT", 2: "PT_ERR_IO", 3: "PT_ERR_PARSE", 4: "PT_ERR_NO_DEVICE",
                5: "PT_ERR_HIP", 6: "PT_ERR_OUT_OF_MEMORY", 7: "PT_ERR_UNSUPPORTED"}
PT_ABI_VERSION = 5
RNG_COUNTER, RNG_REFERENCE_STREAM = 0, 1
# test-only builds of the same ABI (csrc/Makefile): never loaded by the product path
VERIFY_LIB_PATH = os.path.join(_HERE, "lib", "libpt_verify.so")
TESTHOOKS_LIB_PATH = os.path.join(_HERE, "lib", "libpt_testhooks.so")

# every symbol include/pt_hip.h declares
ABI_SYMBOLS = ["pt_scene_load_obj", "pt_scene_create", "pt_scene_counts", "pt_scene_get_triangles",
               "pt_scene_get_materials", "pt_scene_destroy", "pt_render_device", "pt_render_host", "pt_trace_rays_host",
               "pt_session_create", "pt_session_render", "pt_session_wait", "pt_session_read", "pt_session_clear", "pt_session_destroy",
               "pt_scene_cull_tables", "pt_scene_cull_layout", "pt_scene_set_skybox_bmp", "pt_resolve", "pt_resolve_float",
               "pt_post_filter_host", "pt_quantize",
               "pt_write_bmp", "pt_host_alloc", "pt_host_free", "pt_abi_version", "pt_device_count", "pt_last_error",
               "pt_scene_clone_to_device", "pt_scene_timings", "pt_table_limits_check", "pt_rccl_available",
               "pt_frame_create", "pt_frame_info", "pt_frame_render", "pt_frame_gather", "pt_frame_wait", "pt_frame_read",
               "pt_frame_clear", "pt_frame_destroy", "pt_frame_band_kernel_ms", "pt_scene_skybox_size", "pt_table_limits_check_tree",
               "pt_band_rows", "pt_session_create_strided", "pt_frame_row_stride",
               "pt_camera_look_at", "pt_scene_set_camera", "pt_scene_get_camera", "pt_frame_set_camera",
               "pt_scene_set_lens", "pt_scene_get_lens", "pt_frame_set_lens",
               "pt_scene_set_camera_motion", "pt_scene_get_camera_motion", "pt_frame_set_camera_motion",
               "pt_projection_make", "pt_camera_ortho", "pt_scene_set_projection", "pt_scene_get_projection", "pt_frame_set_projection",
               "pt_render_features_host", "pt_denoise_host", "pt_tonemap",
               "pt_temporal_create", "pt_temporal_push_host", "pt_temporal_reset", "pt_temporal_destroy",
               "pt_display_create", "pt_display_create_frame", "pt_display_present", "pt_display_reset", "pt_display_destroy",
               "pt_display_bytes_host", "pt_display_table",
               "pt_upsample_host", "pt_display_present_scaled",
               "pt_grade_host", "pt_meter_host", "pt_exposure_from_histogram", "pt_display_present_graded",
               "pt_display_bytes_graded_host",
               "pt_bloom_host", "pt_display_present_bloom",
               "pt_local_host", "pt_display_present_local",
               "pt_lut_create", "pt_lut_load_cube", "pt_lut_size", "pt_lut_destroy", "pt_colour_matrix", "pt_colour_host",
               "pt_display_bytes_colour_host", "pt_display_present_colour",
               "pt_optics_host", "pt_display_present_optics",
               "pt_sharpen_host", "pt_display_present_sharpen",
               "pt_grain_quantize", "pt_display_bytes_grain_host", "pt_display_present_grain",
               "pt_linear_bytes", "pt_linear_encode", "pt_linear_encode_device_host", "pt_display_present_linear", "pt_write_pfm",
               "pt_write_hdr",
               "pt_scene_set_environment_file", "pt_scene_set_environment_equirect", "pt_scene_set_environment_map",
               "pt_scene_get_environment", "pt_environment_from_equirect", "pt_environment_lookup",
               "pt_frame_set_environment_file", "pt_frame_set_environment_equirect", "pt_frame_set_environment_map",
               "pt_frame_get_environment",
               "pt_scene_set_dielectrics", "pt_scene_get_dielectrics", "pt_frame_set_dielectrics", "pt_frame_get_dielectrics",
               "pt_scene_set_texcoords", "pt_scene_get_texcoords", "pt_scene_set_textures", "pt_scene_get_textures",
               "pt_frame_set_texcoords", "pt_frame_get_texcoords", "pt_frame_set_textures", "pt_frame_get_textures",
               "pt_scene_get_map_kd", "pt_texture_load_bmp", "pt_texture_lookup", "pt_scene_get_texture_records",
               "pt_scene_set_shading_normals", "pt_scene_get_shading_normals", "pt_scene_get_vertex_normals",
               "pt_frame_set_shading_normals", "pt_frame_get_shading_normals", "pt_smooth_normals", "pt_scene_load_obj_ex",
               "pt_shading_normal_at",
               "pt_scene_set_roughness", "pt_scene_get_roughness", "pt_frame_set_roughness", "pt_frame_get_roughness",
               "pt_scene_get_mtl_roughness", "pt_rough_step",
               "pt_scene_set_direct_lighting", "pt_scene_get_direct_lighting", "pt_scene_get_lights", "pt_frame_set_direct_lighting",
               "pt_frame_get_direct_lighting", "pt_frame_get_lights", "pt_direct_term",
               "pt_scene_set_environment_sampling", "pt_scene_get_environment_sampling", "pt_scene_get_environment_sampling_table",
               "pt_frame_set_environment_sampling", "pt_frame_get_environment_sampling", "pt_frame_get_environment_sampling_table",
               "pt_envdirect_term",
               "pt_scene_set_roulette", "pt_scene_get_roulette", "pt_frame_set_roulette", "pt_frame_get_roulette", "pt_roulette_step"]
FRAME_REHEARSE, FRAME_SELF_COLLECTIVE = 1, 2
BIG_SCENE_TRIANGLES = 1024     # csrc/pt_scene.hpp: kBigSceneTriangles -- scenes above it take the box-tree path (tests/test_abi_host.py compares)
TRANSPORT_NAMES = {0: "none", 1: "rccl", 2: "device_copies"}


class PtError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


class RenderParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("row_begin", C.c_int32), ("row_end", C.c_int32),
                ("pass_begin", C.c_int32), ("pass_count", C.c_int32), ("max_ray_reflections", C.c_int32),
                ("eps", C.c_float), ("error", C.c_float), ("seed", C.c_uint32), ("rng_policy", C.c_int32), ("row_stride", C.c_int32)]


class RenderStats(C.Structure):
    _fields_ = [("samples_traced", C.c_uint64), ("segments", C.c_uint64), ("contributing", C.c_uint64),
                ("exact_tests", C.c_uint64), ("misses", C.c_uint64), ("wave_segments", C.c_uint64),
                ("wave_node_rounds", C.c_uint64), ("wave_exact_iterations", C.c_uint64), ("kernel_ms", C.c_float),
                ("n_triangles", C.c_int32), ("n_chunks", C.c_int32), ("partial_commit_rounds", C.c_int32),
                ("verify_checked", C.c_uint64), ("verify_mismatches", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Camera(C.Structure):
    """pt_camera: primary rays start at `origin`; pixel (x, y) looks along normalize((u right + v up) + forward) with
    u = (x + jx) / W - 0.5, v = -(y + jy) / H + 0.5 (main.cpp:126-128).  REFERENCE_CAMERA is the reference's fixed view."""
    _fields_ = [("origin", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3), ("forward", C.c_float * 3)]

    @classmethod
    def of(cls, origin, right, up, forward):
        return cls((C.c_float * 3)(*origin), (C.c_float * 3)(*right), (C.c_float * 3)(*up), (C.c_float * 3)(*forward))

    def as_array(self):
        """4 x 3 float32: origin, right, up, forward."""
        return np.array([list(self.origin), list(self.right), list(self.up), list(self.forward)], np.float32)

    def __eq__(self, other):
        return isinstance(other, Camera) and np.array_equal(self.as_array().view(np.uint32), other.as_array().view(np.uint32))

    def __repr__(self):
        return "Camera(origin=%s, right=%s, up=%s, forward=%s)" % tuple(tuple(r) for r in self.as_array().tolist())


REFERENCE_CAMERA = ((0.0, 0.0, -20.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))   # main.cpp:126-129
REFERENCE_FOV_Y = 53.13010235415598   # 2 atan(0.5) in degrees: the reference's vertical (and horizontal) field of view


class Lens(C.Structure):
    """pt_lens: a thin lens of aperture `radius` focused at `focus_distance` along the camera's forward axis (pt_hip.h states
    the primary ray it gives exactly).  radius 0 is a pinhole."""
    _fields_ = [("radius", C.c_float), ("focus_distance", C.c_float)]

    def __eq__(self, other):
        return isinstance(other, Lens) and np.array_equal(np.array([self.radius, self.focus_distance], np.float32).view(np.uint32),
                                                          np.array([other.radius, other.focus_distance], np.float32).view(np.uint32))

    def __repr__(self):
        return "Lens(radius=%r, focus_distance=%r)" % (self.radius, self.focus_distance)


PROJECTION_PERSPECTIVE, PROJECTION_ORTHOGRAPHIC, PROJECTION_FISHEYE, PROJECTION_EQUIRECTANGULAR = 0, 1, 2, 3
PROJECTION_KINDS = {"perspective": 0, "ortho": 1, "orthographic": 1, "fisheye": 2, "equirect": 3, "equirectangular": 3}


class Projection(C.Structure):
    """pt_projection: how a pixel becomes a primary ray (pt_hip.h states each kind exactly).  span_x / span_y: the angles, in
    radians, the image's width / height cover under a fisheye or an equirectangular projection."""
    _fields_ = [("kind", C.c_int32), ("span_x", C.c_float), ("span_y", C.c_float)]

    def __eq__(self, other):
        return isinstance(other, Projection) and self.kind == other.kind and np.array_equal(
            np.array([self.span_x, self.span_y], np.float32).view(np.uint32), np.array([other.span_x, other.span_y], np.float32).view(np.uint32))

    def __repr__(self):
        return "Projection(kind=%r, span_x=%r, span_y=%r)" % (self.kind, self.span_x, self.span_y)


class DenoiseParams(C.Structure):
    """pt_denoise_params: a zeroed struct holds the defaults, except that `levels` says how much is filtered (0 = nothing)."""
    _fields_ = [("levels", C.c_int32), ("sigma_luminance", C.c_float), ("sigma_plane", C.c_float), ("normal_power_log2", C.c_int32),
                ("demodulate_albedo", C.c_int32)]


DENOISE_MAX_LEVELS = 8


class UpsampleParams(C.Structure):
    """pt_upsample_params: scale 2, 3 or 4; the other fields zeroed hold the defaults (sigma_plane 0.1, normal_power_log2 7,
    demodulation on)."""
    _fields_ = [("scale", C.c_int32), ("sigma_plane", C.c_float), ("normal_power_log2", C.c_int32), ("demodulate_albedo", C.c_int32)]


UPSAMPLE_MAX_SCALE = 4


class TemporalParams(C.Structure):
    """pt_temporal_params: a zeroed struct holds the defaults (max_frames 32, sigma_plane 0.1, min_normal_dot 0.9)."""
    _fields_ = [("max_frames", C.c_float), ("sigma_plane", C.c_float), ("min_normal_dot", C.c_float)]


class DisplayParams(C.Structure):
    """pt_display_params: gamma, whether the display's temporal stage runs (and its parameters), the filter (levels 0 = none)."""
    _fields_ = [("gamma", C.c_float), ("temporal", C.c_int32), ("temporal_params", TemporalParams), ("denoise", DenoiseParams)]


class DisplayInfo(C.Structure):
    """pt_display_info: the chain's milliseconds, the pixels the host finished, the table's levels and doubt bands."""
    _fields_ = [("kernel_ms", C.c_float), ("deferred_pixels", C.c_int32), ("table_levels", C.c_int32), ("doubt_bands", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


DISPLAY_MAX_LEVELS = 4096
CURVE_REFERENCE, CURVE_CLAMP, CURVE_REINHARD, CURVE_ACES = 0, 1, 2, 3
CURVES = {"reference": CURVE_REFERENCE, "clamp": CURVE_CLAMP, "reinhard": CURVE_REINHARD, "aces": CURVE_ACES}
METER_ENTRIES = 129


class GradeParams(C.Structure):
    """pt_grade_params: the tone curve, the manual exposure (0 = 1) or auto_exposure with its metering rule; a zeroed struct is no
    grading at all, and zeroed metering fields hold the defaults (percentile 50, key 0.18, e_min 2^-8, e_max 2^8, rate 1)."""
    _fields_ = [("curve", C.c_int32), ("exposure", C.c_float), ("auto_exposure", C.c_int32), ("percentile", C.c_int32),
                ("key", C.c_float), ("e_min", C.c_float), ("e_max", C.c_float), ("rate", C.c_float)]


class GradeInfo(C.Structure):
    """pt_grade_info: the exposure used, the meter's target e*, the metered and the dark pixels."""
    _fields_ = [("exposure", C.c_float), ("target", C.c_float), ("metered", C.c_uint32), ("dark", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def _grade_params(grade):
    """A GradeParams, or a dict of its fields (curve may be a name: "clamp") -> a GradeParams."""
    if isinstance(grade, dict):
        curve = grade.get("curve", CURVE_REFERENCE)
        return GradeParams(CURVES[curve] if isinstance(curve, str) else curve, grade.get("exposure", 0.0), 1 if grade.get("auto_exposure") else 0,
                           grade.get("percentile", 0), grade.get("key", 0.0), grade.get("e_min", 0.0), grade.get("e_max", 0.0),
                           grade.get("rate", 0.0))
    return grade


BLOOM_MAX_LEVELS = 8


class BloomParams(C.Structure):
    """pt_bloom_params: a zeroed struct is no bloom (strength 0); threshold 0 = 1, levels 0 = 5 (1 .. 8)."""
    _fields_ = [("threshold", C.c_float), ("strength", C.c_float), ("levels", C.c_int32)]


def _bloom_params(bloom):
    """A BloomParams, or a dict of its fields ({"strength": 0.5}) -> a BloomParams."""
    if isinstance(bloom, dict):
        return BloomParams(bloom.get("threshold", 0.0), bloom.get("strength", 0.0), bloom.get("levels", 0))
    return bloom


LOCAL_MAX_LEVELS = 8


class LocalParams(C.Structure):
    """pt_local_params: a zeroed struct is no local exposure (strength 0); pivot 0 = 0.18, levels 0 = 5 (1 .. 8), sigma 0 = 0.5."""
    _fields_ = [("strength", C.c_float), ("pivot", C.c_float), ("levels", C.c_int32), ("sigma", C.c_float)]


def _local_params(local):
    """A LocalParams, or a dict of its fields ({"strength": 1.0}) -> a LocalParams."""
    if isinstance(local, dict):
        return LocalParams(local.get("strength", 0.0), local.get("pivot", 0.0), local.get("levels", 0), local.get("sigma", 0.0))
    return local


LUT_MAX_SIZE = 65


class ColourParams(C.Structure):
    """pt_colour_params: a zeroed struct is no colour stage; wb 0 0 0 = 1 1 1, saturation 0 = 1 unless saturation_set, matrix all
    zero = identity, lut NULL = none."""
    _fields_ = [("wb", C.c_float * 3), ("saturation", C.c_float), ("saturation_set", C.c_int32), ("matrix", C.c_float * 9), ("lut", C.c_void_p)]


class Lut:
    """pt_lut: an immutable 3D LUT in host memory (tetrahedral interpolation on the tone curve's output)."""

    def __init__(self, handle, library=None):
        self._h, self._L = handle, library or lib()

    @classmethod
    def load_cube(cls, path, library=None):
        """pt_lut_load_cube: a .cube file with LUT_3D_SIZE 2 .. 65 and the domain 0 .. 1."""
        L = library or lib()
        h = C.c_void_p()
        _check(L.pt_lut_load_cube(os.fsencode(path), C.byref(h)), L)
        return cls(h, L)

    @classmethod
    def create(cls, array, library=None):
        """pt_lut_create: array [N, N, N, 3] indexed [blue, green, red] (the red index runs fastest, the order of a .cube file)."""
        L = library or lib()
        a = np.ascontiguousarray(array, np.float32)
        if a.ndim != 4 or a.shape[3] != 3 or not (a.shape[0] == a.shape[1] == a.shape[2]):
            raise ValueError("Lut.create: the array must be [N, N, N, 3]")
        h = C.c_void_p()
        _check(L.pt_lut_create(a.shape[0], _fp(a), C.byref(h)), L)
        return cls(h, L)

    @property
    def size(self):
        n = C.c_int32()
        _check(self._L.pt_lut_size(self._h, C.byref(n)), self._L)
        return n.value

    def close(self):
        if self._h:
            self._L.pt_lut_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _colour_params(colour):
    """A ColourParams, or a dict of its fields ({"wb": (1.1, 1, 0.9), "saturation": 0.8, "matrix": 3 x 3, "lut": Lut}) -> a ColourParams.
    A saturation given in a dict is meant as given: 0 is grey."""
    if isinstance(colour, dict):
        unknown = set(colour) - {"wb", "saturation", "matrix", "lut"}
        if unknown:
            raise ValueError(f"colour: unknown fields {sorted(unknown)}")
        prm = ColourParams()
        if colour.get("wb") is not None:
            prm.wb = (C.c_float * 3)(*[float(v) for v in colour["wb"]])
        if colour.get("saturation") is not None:
            prm.saturation, prm.saturation_set = float(colour["saturation"]), 1
        if colour.get("matrix") is not None:
            prm.matrix = (C.c_float * 9)(*[float(v) for v in np.asarray(colour["matrix"], np.float64).reshape(9)])
        lut = colour.get("lut")
        if lut is not None:
            prm.lut = lut._h if isinstance(lut, Lut) else lut
            prm._keep = lut   # the LUT outlives the parameters
        return prm
    return colour


class OpticsParams(C.Structure):
    """pt_optics_params: a zeroed struct is no optics stage; k1, k2 in -4 .. 4, ca in -0.25 .. 0.25, vignette in 0 .. 64."""
    _fields_ = [("k1", C.c_float), ("k2", C.c_float), ("ca", C.c_float), ("vignette", C.c_float)]


SHARPEN_MAX_LIMIT = 0.1875


class SharpenParams(C.Structure):
    """pt_sharpen_params: a zeroed struct is no sharpening (strength 0); strength in (0, 1], limit 0 = 0.1875, else in (0, 0.1875]."""
    _fields_ = [("strength", C.c_float), ("limit", C.c_float)]


def _sharpen_params(sharpen):
    """A SharpenParams, or a dict of its fields ({"strength": 0.5, "limit": 0.1}) -> a SharpenParams."""
    if isinstance(sharpen, dict):
        unknown = set(sharpen) - {"strength", "limit"}
        if unknown:
            raise ValueError(f"sharpen: unknown fields {sorted(unknown)}")
        return SharpenParams(sharpen.get("strength", 0.0), sharpen.get("limit", 0.0))
    return sharpen


GRAIN_MAX_SIZE = 8.0


class GrainParams(C.Structure):
    """pt_grain_params: a zeroed struct is no grain and no dither; strength in 0 .. 1, size 0 (= 1) or 1 .. 8 pixels, dither in
    0 .. 1 levels, seed and frame any uint32 (frame: the noise's third coordinate)."""
    _fields_ = [("strength", C.c_float), ("size", C.c_float), ("dither", C.c_float), ("seed", C.c_uint32), ("frame", C.c_uint32)]


def _grain_params(grain):
    """A GrainParams, or a dict of its fields ({"strength": 0.2, "size": 1.5, "dither": 1.0, "seed": 7, "frame": 0}) -> a GrainParams."""
    if isinstance(grain, dict):
        unknown = set(grain) - {"strength", "size", "dither", "seed", "frame"}
        if unknown:
            raise ValueError(f"grain: unknown fields {sorted(unknown)}")
        return GrainParams(grain.get("strength", 0.0), grain.get("size", 0.0), grain.get("dither", 0.0), int(grain.get("seed", 0)) & 0xFFFFFFFF,
                           int(grain.get("frame", 0)) & 0xFFFFFFFF)
    return grain


class LinearParams(C.Structure):
    """pt_linear_params: format 0 (no linear output), LINEAR_PFM or LINEAR_RGBE; exposed 1 multiplies the mean by the present's exposure."""
    _fields_ = [("format", C.c_int32), ("exposed", C.c_int32)]


LINEAR_PFM, LINEAR_RGBE = 1, 2
LINEAR_FORMATS = {"pfm": LINEAR_PFM, "hdr": LINEAR_RGBE}


def _linear_params(linear=None, format=None, exposed=False):
    """A LinearParams from one, from a dict of its fields ({"format": "hdr", "exposed": False}), or from the two values; a format may
    be "pfm", "hdr" or the number the library is to judge."""
    if isinstance(linear, LinearParams):
        return linear
    if isinstance(linear, dict):
        unknown = set(linear) - {"format", "exposed"}
        if unknown:
            raise ValueError(f"linear: unknown fields {sorted(unknown)}")
        format, exposed = linear.get("format", "pfm"), linear.get("exposed", False)
    if isinstance(format, str):
        if format not in LINEAR_FORMATS:
            raise ValueError(f"linear: format must be one of {sorted(LINEAR_FORMATS)}")
        format = LINEAR_FORMATS[format]
    return LinearParams(int(format), int(exposed))


def _optics_params(optics):
    """An OpticsParams, or a dict of its fields ({"k1": -0.1, "ca": 0.01, "vignette": 1.0}) -> an OpticsParams."""
    if isinstance(optics, dict):
        unknown = set(optics) - {"k1", "k2", "ca", "vignette"}
        if unknown:
            raise ValueError(f"optics: unknown fields {sorted(unknown)}")
        return OpticsParams(optics.get("k1", 0.0), optics.get("k2", 0.0), optics.get("ca", 0.0), optics.get("vignette", 0.0))
    return optics


def _lens_arg(radius, focus_distance):
    """(radius, focus_distance), a Lens, or None -> a pointer argument for pt_scene_set_lens / pt_frame_set_lens."""
    if radius is None:
        return None
    if isinstance(radius, Lens):
        return C.byref(radius)
    if focus_distance is None:
        raise TypeError("set_lens(radius, focus_distance): the focus distance is missing")
    return C.byref(Lens(radius, focus_distance))


def look_at(eye, target, up=(0.0, 1.0, 0.0), fov_y=REFERENCE_FOV_Y, aspect=0.0, library=None):
    """pt_camera_look_at: a Camera at `eye` looking at `target`; fov_y in degrees; aspect = W / H for square pixels, 0 for the
    reference's mapping (both image axes span fov_y)."""
    L = library or lib()
    f3 = C.c_float * 3
    cam = Camera()
    _check(L.pt_camera_look_at(f3(*eye), f3(*target), f3(*up), fov_y, aspect, C.byref(cam)), L)
    return cam


def _projection_kind(kind):
    if isinstance(kind, str):
        if kind not in PROJECTION_KINDS:
            raise ValueError(f"projection: unknown kind {kind!r} (one of {sorted(PROJECTION_KINDS)})")
        return PROJECTION_KINDS[kind]
    return int(kind)


def projection(kind, fov_y=0.0, aspect=0.0, library=None):
    """pt_projection_make: a Projection of `kind` (a PROJECTION_* number or "perspective", "ortho", "fisheye", "equirect").
    fov_y, in degrees, is the angle across the image height of a fisheye or an equirectangular view and aspect = W / H the ratio of
    the angle across its width to it; an equirectangular view with fov_y <= 0 is the full sphere."""
    L = library or lib()
    p = Projection()
    _check(L.pt_projection_make(_projection_kind(kind), fov_y, aspect, C.byref(p)), L)
    return p


def ortho_camera(eye, target, up=(0.0, 1.0, 0.0), view_height=20.0, aspect=0.0, library=None):
    """pt_camera_ortho: a Camera for an orthographic view at `eye` looking at `target`, whose image is view_height scene units high
    and view_height * aspect wide (aspect 0: as high as wide)."""
    L = library or lib()
    f3 = C.c_float * 3
    cam = Camera()
    _check(L.pt_camera_ortho(f3(*eye), f3(*target), f3(*up), view_height, aspect, C.byref(cam)), L)
    return cam


class EnvironmentParams(C.Structure):
    """pt_environment_params: gain, rotation about +y in degrees, N of the octahedral map (0 = the default for the picture)."""
    _fields_ = [("gain", C.c_float), ("rotate_y_degrees", C.c_float), ("size", C.c_int32)]


def environment_from_equirect(picture, size, gain=1.0, rotate=0.0, library=None):
    """pt_environment_from_equirect: an (h, w, 3) equirectangular picture -> the (size, size, 3) octahedral map, on the host."""
    L = library or lib()
    pic = np.ascontiguousarray(picture, np.float32)
    if pic.ndim != 3 or pic.shape[2] != 3:
        raise ValueError("environment_from_equirect: picture must be (h, w, 3)")
    out = np.zeros((max(int(size), 0), max(int(size), 0), 3), np.float32)
    prm = EnvironmentParams(gain, rotate, 0)
    _check(L.pt_environment_from_equirect(pic.shape[1], pic.shape[0], _fp(pic), C.byref(prm), int(size), _fp(out)), L)
    return out


def environment_lookup(env_map, directions, library=None):
    """pt_environment_lookup: the radiance an (n, n, 3) octahedral map holds for each unit direction, [..., 3] -> [..., 3]."""
    L = library or lib()
    m = np.ascontiguousarray(env_map, np.float32)
    if m.ndim != 3 or m.shape[0] != m.shape[1] or m.shape[2] != 3:
        raise ValueError("environment_lookup: env_map must be (n, n, 3)")
    d = np.ascontiguousarray(directions, np.float32)
    out = np.zeros(d.shape, np.float32)
    _check(L.pt_environment_lookup(m.shape[0], _fp(m), d.size // 3, _fp(d), _fp(out)), L)
    return out


class Dielectric(C.Structure):
    """pt_dielectric: a material's index, its refractive index and its transmission tint."""
    _fields_ = [("material", C.c_int32), ("ior", C.c_float), ("tint", C.c_float * 3)]

    def __repr__(self):
        return f"dielectric({self.material}, {self.ior!r}, tint={tuple(self.tint)!r})"


def dielectric(material, ior, tint=(1.0, 1.0, 1.0)):
    """One entry of a handle's dielectrics (-GLASS m:ior[:r:g:b]): material `material` is smooth glass of refractive index `ior`
    whose transmitted light is multiplied by `tint`."""
    return Dielectric(int(material), float(ior), (C.c_float * 3)(*tint))


ROUGH_ALPHA_MIN, ROUGH_ALPHA_MAX = 2.0 ** -10, 1.0


class Rough(C.Structure):
    """pt_rough: a material's index and the roughness alpha of its glossy lobe."""
    _fields_ = [("material", C.c_int32), ("alpha", C.c_float)]

    def __repr__(self):
        return f"rough({self.material}, {self.alpha!r})"


def rough(material, alpha):
    """One entry of a handle's roughness list (-ROUGH m:alpha): the glossy lobe of material `material` is a GGX lobe of roughness
    `alpha` in 2^-10 .. 1 instead of a mirror."""
    return Rough(int(material), float(alpha))


def rough_step(normals, directions, alpha, w1, w2, library=None, want_microfacet=False):
    """pt_rough_step, the host's own evaluation of the rough glossy step: for unit normals [n, 3], unit incoming directions [n, 3],
    alpha [n] (or one value) and the random words w1, w2 [n] the new directions [n, 3] and G1 [n]; with want_microfacet also the
    microfacet normal [n, 3] in the frame (t1, t2, n)."""
    L = library or lib()
    n_ = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, np.float32), (len(n_),)))
    u1, u2 = np.ascontiguousarray(w1, np.uint32).reshape(-1), np.ascontiguousarray(w2, np.uint32).reshape(-1)
    if not (len(d) == len(n_) == len(u1) == len(u2)):
        raise ValueError("rough_step: arrays of one length")
    out, g1, h = np.zeros((len(n_), 3), np.float32), np.zeros(len(n_), np.float32), np.zeros((len(n_), 3), np.float32)
    up = C.POINTER(C.c_uint32)
    _check(L.pt_rough_step(len(n_), _fp(n_), _fp(d), _fp(a), u1.ctypes.data_as(up), u2.ctypes.data_as(up), _fp(out), _fp(g1), _fp(h)), L)
    return (out, g1, h) if want_microfacet else (out, g1)


# pt_light, the record of a handle's light table (pt_hip.h: direct lighting), as a numpy dtype: 80 bytes
LIGHT_DTYPE = np.dtype([("v0", np.float32, 3), ("cdf", np.float32), ("e1", np.float32, 3), ("triangle", np.int32), ("e2", np.float32, 3),
                        ("pad0", np.float32), ("normal", np.float32, 3), ("pad1", np.float32), ("le", np.float32, 3), ("pad2", np.float32)])


def direct_term(lights, area, origins, normals, shading_normals, throughput, kd, l0, l1, l2, library=None):
    """pt_direct_term, the host's own evaluation of the direct term without the visibility: for a light table (`lights` of LIGHT_DTYPE,
    `area` = A), next origins O [n, 3], stored normals N, shading normals n, throughputs T and albedos Kd [n, 3] and the words l0, l1,
    l2 [n]: the chosen light's table index [n], the point P [n, 3], the unit direction [n, 3], the term [n, 3] and whether there is one [n]."""
    L = library or lib()
    lt = np.ascontiguousarray(lights, LIGHT_DTYPE)
    arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (origins, normals, shading_normals, throughput, kd)]
    words = [np.ascontiguousarray(w, np.uint32).reshape(-1) for w in (l0, l1, l2)]
    n = len(arrs[0])
    if any(len(a) != n for a in arrs + words):
        raise ValueError("direct_term: arrays of one length")
    idx, has = np.zeros(n, np.int32), np.zeros(n, np.int32)
    pts, dirs, terms = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    up, ip = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    _check(L.pt_direct_term(n, lt.ctypes.data_as(C.c_void_p), len(lt), C.c_float(area), *[_fp(a) for a in arrs], *[w.ctypes.data_as(up) for w in words],
                            idx.ctypes.data_as(ip), _fp(pts), _fp(dirs), _fp(terms), has.ctypes.data_as(ip)), L)
    return idx, pts, dirs, terms, has.astype(bool)


# pt_env_sample_record, one cell of a handle's environment sampling table (pt_hip.h: environment sampling), as a numpy dtype: 16 bytes
ENV_SAMPLE_DTYPE = np.dtype([("accept", np.float32), ("alias", np.int32), ("pdf_self", np.float32), ("pdf_alias", np.float32)])


def envdirect_term(records, share, env_map, normals, shading_normals, throughput, kd, e0, e1, e2, e3, library=None):
    """pt_envdirect_term, the host's own evaluation of the environment sample and its term without the visibility: for a table
    (`records` of ENV_SAMPLE_DTYPE, [S, S] or [S * S]), the share, the (N, N, 3) map, stored normals N, shading normals n, throughputs T
    and albedos Kd [n, 3] and the words e0 .. e3 [n]: the chosen cell [n], the unit direction [n, 3], its density per solid angle [n],
    the term [n, 3] and whether there is one [n]."""
    L = library or lib()
    rec = np.ascontiguousarray(records, ENV_SAMPLE_DTYPE).reshape(-1)
    cells = int(round(len(rec) ** 0.5))
    if cells * cells != len(rec):
        raise ValueError("envdirect_term: a table of S x S records")
    m = np.ascontiguousarray(env_map, np.float32)
    if m.ndim != 3 or m.shape[0] != m.shape[1] or m.shape[2] != 3:
        raise ValueError("envdirect_term: an (n, n, 3) map")
    arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (normals, shading_normals, throughput, kd)]
    words = [np.ascontiguousarray(w, np.uint32).reshape(-1) for w in (e0, e1, e2, e3)]
    n = len(arrs[0])
    if any(len(a) != n for a in arrs + words):
        raise ValueError("envdirect_term: arrays of one length")
    cell, has = np.zeros(n, np.int32), np.zeros(n, np.int32)
    dirs, pdf, terms = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    up, ip = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    _check(L.pt_envdirect_term(n, rec.ctypes.data_as(C.c_void_p), cells, C.c_float(share), m.shape[0], _fp(m), *[_fp(a) for a in arrs],
                               *[w.ctypes.data_as(up) for w in words], cell.ctypes.data_as(ip), _fp(dirs), _fp(pdf), _fp(terms), has.ctypes.data_as(ip)), L)
    return cell, dirs, pdf, terms, has.astype(bool)


ROULETTE_DEFAULT_FLOOR = 1.0 / 16.0   # pt_hip.h: PT_ROULETTE_DEFAULT_FLOOR


def roulette_step(throughput, w0, floor=ROULETTE_DEFAULT_FLOOR, library=None):
    """pt_roulette_step, the host's own evaluation of the roulette step (pt_hip.h: Russian roulette): throughputs T [n, 3] and the
    words w0 [n] under `floor` give the throughputs after the step [n, 3] and whether each path survives [n]."""
    L = library or lib()
    t = np.ascontiguousarray(throughput, np.float32).reshape(-1, 3)
    w = np.ascontiguousarray(w0, np.uint32).reshape(-1)
    if len(t) != len(w):
        raise ValueError("roulette_step: arrays of one length")
    out, alive = np.zeros_like(t), np.zeros(len(t), np.int32)
    _check(L.pt_roulette_step(len(t), C.c_float(floor), _fp(t), w.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(out),
                              alive.ctypes.data_as(C.POINTER(C.c_int32))), L)
    return out, alive.astype(bool)


TEXTURE_NEAREST, TEXTURE_BILINEAR = 0, 1
TEXTURE_MAX_SIDE = 8192
_TEXTURE_FILTERS = {"nearest": TEXTURE_NEAREST, "bilinear": TEXTURE_BILINEAR}


def _texture_filter(filter):
    if isinstance(filter, str):
        if filter not in _TEXTURE_FILTERS:
            raise ValueError(f"texture filter {filter!r}: nearest or bilinear")
        return _TEXTURE_FILTERS[filter]
    return int(filter)


class TextureEntry(C.Structure):
    """pt_texture: a material's index, the picture's size, the filter and a pointer to width * height * 3 floats."""
    _fields_ = [("material", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("filter", C.c_int32), ("rgb", C.POINTER(C.c_float))]


class Texture:
    """One entry of a handle's textures: `texels` is (height, width, 3) linear RGB, row 0 the top of the picture."""

    def __init__(self, material, texels, filter=TEXTURE_BILINEAR):
        t = np.ascontiguousarray(texels, np.float32)
        if t.ndim != 3 or t.shape[2] != 3:
            raise ValueError("texture: texels must be (height, width, 3)")
        self.material, self.texels, self.filter = int(material), t, _texture_filter(filter)

    def __repr__(self):
        return f"texture({self.material}, {self.texels.shape[1]} x {self.texels.shape[0]}, filter={self.filter})"


def texture(material, texels, filter="bilinear"):
    """One entry of a handle's textures (-TEXTURE m:file[:filter]): material `material` takes the (height, width, 3) picture `texels`."""
    return Texture(material, texels, filter)


def load_texture_bmp(path, gamma=2.2, library=None):
    """pt_texture_load_bmp: a 24-bit BMP as (height, width, 3) linear floats, bytes decoded as pow(b / 255, gamma)."""
    L = library or lib()
    w, h = C.c_int32(), C.c_int32()
    _check(L.pt_texture_load_bmp(os.fsencode(path), gamma, C.byref(w), C.byref(h), None), L)
    out = np.zeros((h.value, w.value, 3), np.float32)
    _check(L.pt_texture_load_bmp(os.fsencode(path), gamma, C.byref(w), C.byref(h), _fp(out)), L)
    return out


def texture_lookup(texels, uv, filter="bilinear", library=None, want_indices=False):
    """pt_texture_lookup, the host's own lookup: the texel of the (height, width, 3) picture at each (u, v) of `uv` [n, 2]; with
    want_indices also the four texel indices (row * width + column) each lookup read."""
    L = library or lib()
    t = np.ascontiguousarray(texels, np.float32)
    q = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    out = np.zeros((len(q), 3), np.float32)
    idx = np.zeros((len(q), 4), np.int32)
    _check(L.pt_texture_lookup(t.shape[1], t.shape[0], _fp(t), _texture_filter(filter), len(q), _fp(q), _fp(out), _ip(idx)), L)
    return (out, idx) if want_indices else out


LOAD_GEOMETRIC_PLANES = 1
SMOOTH_DEFAULT_CREASE = 60.0


def smooth_normals(vertices, crease=SMOOTH_DEFAULT_CREASE, library=None):
    """pt_smooth_normals, the normal generator: (n_tri, 3, 3) unit normals per corner from the triangles' vertices (n_tri, 3, 3) -- or
    a scene's 14-float triangle records -- welded where positions are bit-identical, smoothed across faces within `crease` degrees,
    weighted by the angle at the vertex; zeros for a degenerate triangle."""
    L = library or lib()
    v = np.ascontiguousarray(vertices, np.float32)
    if v.ndim == 2 and v.shape[1] == 14:
        v = np.ascontiguousarray(v[:, 4:13])
    v = v.reshape(-1, 9)
    out = np.zeros((len(v), 3, 3), np.float32)
    _check(L.pt_smooth_normals(len(v), _fp(v), crease, _fp(out)), L)
    return out


def shading_normal_at(vertices, plane_normal, normals, points, library=None, want_interpolated=False):
    """pt_shading_normal_at, the host's own interpolation: Ns [n, 3] at `points` [n, 3] on the triangle `vertices` (3, 3) with stored
    normal `plane_normal` and corner normals `normals` (3, 3); with want_interpolated also whether each came from the corners."""
    L = library or lib()
    v = np.ascontiguousarray(vertices, np.float32).reshape(9)
    N = np.ascontiguousarray(plane_normal, np.float32).reshape(3)
    n9 = np.ascontiguousarray(normals, np.float32).reshape(9)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    out = np.zeros((len(p), 3), np.float32)
    own = np.zeros(len(p), np.int32)
    _check(L.pt_shading_normal_at(_fp(v), _fp(N), _fp(n9), len(p), _fp(p), _fp(out), _ip(own)), L)
    return (out, own.astype(bool)) if want_interpolated else out


def _projection_arg(projection_, library):
    """A Projection, a kind (number or name) or None -> a pointer argument for pt_scene_set_projection / pt_frame_set_projection."""
    if projection_ is None:
        return None
    if not isinstance(projection_, Projection):
        projection_ = projection(projection_, library=library)
    return C.byref(projection_)


def build(force=False):
    """Compile libpt_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC_DIR, "clean", "-s"])
    # the product library + the test / diagnostic builds.  Eight jobs where the machine has them: every library is ten kernel objects of one
    # to five minutes each, and at four jobs the build took as long as the slowest library's objects in a row.
    jobs = max(1, min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
    subprocess.check_call(["make", "-C", CSRC_DIR, "-s", f"-j{jobs}"])
    return LIB_PATH


_lib = None


def _share_torch_hip_runtime():
    """PyTorch's ROCm wheels bundle their own libamdhip64.so.7.  A process that ends up with two HIP runtimes (the
    system one pulled in by libpt_hip.so, then torch's) loses the GPU in whichever initialises second -- torch reported
    "No HIP GPUs are available" when it was imported after this library.  If torch is installed, load its copy first
    (located without importing torch): the dynamic linker then resolves libpt_hip.so's libamdhip64.so.7 to it, as
    it already does when torch is imported first, and the order of imports stops mattering."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("PT_HIP_SYSTEM_RUNTIME"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library(path):
    """Load one build of the ABI (the product library by default; tests also load the verification / test-hook builds)."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} is missing: run `make -C {CSRC_DIR}` (there is no CPU fallback)")
    _share_torch_hip_runtime()
    L = C.CDLL(path)
    fp, ip, vp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p
    L.pt_scene_load_obj.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(vp)]
    L.pt_scene_create.argtypes = [fp, ip, C.c_int32, fp, C.c_int32, C.c_int, C.POINTER(vp)]
    L.pt_scene_counts.argtypes = [vp, ip, ip]
    L.pt_scene_get_triangles.argtypes = [vp, fp, ip]
    L.pt_scene_get_materials.argtypes = [vp, fp]
    L.pt_scene_destroy.argtypes = [vp]
    L.pt_scene_destroy.restype = None
    L.pt_render_device.argtypes = [vp, C.POINTER(RenderParams), vp, vp, vp, vp, C.POINTER(RenderStats)]
    L.pt_render_host.argtypes = [vp, C.POINTER(RenderParams), fp, fp, ip, C.POINTER(RenderStats)]
    L.pt_session_create.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.pt_session_create_strided.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.pt_band_rows.restype = C.c_int32
    L.pt_band_rows.argtypes = [C.POINTER(RenderParams)]
    L.pt_session_render.argtypes = [vp, C.POINTER(RenderParams), C.POINTER(RenderStats)]
    L.pt_session_read.argtypes = [vp, fp, fp, ip]
    L.pt_session_wait.argtypes = [vp]
    L.pt_session_clear.argtypes = [vp]
    L.pt_session_destroy.argtypes = [vp]
    L.pt_session_destroy.restype = None
    L.pt_trace_rays_host.argtypes = [vp, C.c_int32, fp, fp, C.c_float, ip, fp]
    L.pt_scene_cull_tables.argtypes = [vp, C.c_float, ip, fp, fp, fp, fp]
    L.pt_scene_cull_layout.argtypes = [vp, C.c_float, ip, ip, vp]
    L.pt_scene_set_skybox_bmp.argtypes = [vp, C.c_char_p]
    L.pt_resolve.argtypes = [C.c_int32, C.c_int32, fp, fp, ip, C.c_float, C.POINTER(C.c_uint8), fp]
    L.pt_resolve_float.argtypes = [C.c_int32, C.c_int32, fp, fp, ip, C.c_float, fp, fp]
    L.pt_post_filter_host.argtypes = [C.c_int, C.c_int32, C.c_int32, fp, C.c_int32, C.c_int32]
    L.pt_quantize.argtypes = [C.c_int32, C.c_int32, fp, ip, C.POINTER(C.c_uint8)]
    L.pt_write_bmp.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]
    L.pt_last_error.restype = C.c_char_p
    L.pt_host_alloc.restype = C.c_void_p
    L.pt_host_alloc.argtypes = [C.c_size_t]
    L.pt_host_free.argtypes = [C.c_void_p]
    L.pt_host_free.restype = None
    L.pt_scene_clone_to_device.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.pt_scene_timings.argtypes = [vp, C.POINTER(C.c_double)]
    L.pt_table_limits_check.argtypes = [C.c_uint64, C.c_uint64, C.c_int32]
    L.pt_rccl_available.argtypes = [ip]
    L.pt_frame_create.argtypes = [vp, ip, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(vp)]
    L.pt_frame_info.argtypes = [vp, ip, ip, ip, ip]
    L.pt_frame_render.argtypes = [vp, C.POINTER(RenderParams), C.POINTER(RenderStats)]
    L.pt_frame_gather.argtypes = [vp]
    L.pt_frame_wait.argtypes = [vp]
    L.pt_frame_read.argtypes = [vp, fp, fp, ip]
    L.pt_frame_clear.argtypes = [vp]
    L.pt_frame_destroy.argtypes = [vp]
    L.pt_frame_destroy.restype = None
    L.pt_frame_band_kernel_ms.argtypes = [vp, fp]
    L.pt_frame_row_stride.argtypes = [vp, ip]
    L.pt_scene_skybox_size.argtypes = [vp, ip, ip]
    L.pt_table_limits_check_tree.argtypes = [C.c_uint64, C.c_uint64, C.c_int32, C.c_int32]
    L.pt_camera_look_at.argtypes = [fp, fp, fp, C.c_float, C.c_float, C.POINTER(Camera)]
    L.pt_scene_set_camera.argtypes = [vp, C.POINTER(Camera)]
    L.pt_scene_get_camera.argtypes = [vp, C.POINTER(Camera), ip]
    L.pt_frame_set_camera.argtypes = [vp, C.POINTER(Camera)]
    L.pt_scene_set_lens.argtypes = [vp, C.POINTER(Lens)]
    L.pt_scene_get_lens.argtypes = [vp, C.POINTER(Lens), ip]
    L.pt_frame_set_lens.argtypes = [vp, C.POINTER(Lens)]
    L.pt_scene_set_camera_motion.argtypes = [vp, C.POINTER(Camera)]
    L.pt_scene_get_camera_motion.argtypes = [vp, C.POINTER(Camera), ip]
    L.pt_frame_set_camera_motion.argtypes = [vp, C.POINTER(Camera)]
    L.pt_projection_make.argtypes = [C.c_int32, C.c_float, C.c_float, C.POINTER(Projection)]
    L.pt_camera_ortho.argtypes = [fp, fp, fp, C.c_float, C.c_float, C.POINTER(Camera)]
    L.pt_scene_set_projection.argtypes = [vp, C.POINTER(Projection)]
    L.pt_scene_get_projection.argtypes = [vp, C.POINTER(Projection), ip]
    L.pt_frame_set_projection.argtypes = [vp, C.POINTER(Projection)]
    ep = C.POINTER(EnvironmentParams)
    L.pt_scene_set_environment_file.argtypes = [vp, C.c_char_p, ep]
    L.pt_scene_set_environment_equirect.argtypes = [vp, C.c_int32, C.c_int32, fp, ep]
    L.pt_scene_set_environment_map.argtypes = [vp, C.c_int32, fp]
    L.pt_scene_get_environment.argtypes = [vp, ip, fp]
    L.pt_frame_set_environment_file.argtypes = [vp, C.c_char_p, ep]
    L.pt_frame_set_environment_equirect.argtypes = [vp, C.c_int32, C.c_int32, fp, ep]
    L.pt_frame_set_environment_map.argtypes = [vp, C.c_int32, fp]
    L.pt_frame_get_environment.argtypes = [vp, ip, fp]
    dp = C.POINTER(Dielectric)
    L.pt_scene_set_dielectrics.argtypes = [vp, dp, C.c_int32]
    L.pt_scene_get_dielectrics.argtypes = [vp, dp, ip]
    L.pt_frame_set_dielectrics.argtypes = [vp, dp, C.c_int32]
    L.pt_frame_get_dielectrics.argtypes = [vp, dp, ip]
    tp = C.POINTER(TextureEntry)
    for who in ("scene", "frame"):
        getattr(L, f"pt_{who}_set_texcoords").argtypes = [vp, fp]
        getattr(L, f"pt_{who}_get_texcoords").argtypes = [vp, fp, ip]
        getattr(L, f"pt_{who}_set_textures").argtypes = [vp, tp, C.c_int32]
        getattr(L, f"pt_{who}_get_textures").argtypes = [vp, tp, ip]
    L.pt_scene_get_texture_records.argtypes = [vp, fp]
    for who in ("scene", "frame"):
        getattr(L, f"pt_{who}_set_shading_normals").argtypes = [vp, fp]
        getattr(L, f"pt_{who}_get_shading_normals").argtypes = [vp, fp, ip]
    L.pt_scene_get_vertex_normals.argtypes = [vp, fp, ip]
    L.pt_smooth_normals.argtypes = [C.c_int32, fp, C.c_float, fp]
    L.pt_scene_load_obj_ex.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.POINTER(vp)]
    L.pt_shading_normal_at.argtypes = [fp, fp, fp, C.c_int32, fp, fp, ip]
    rp = C.POINTER(Rough)
    for who in ("scene", "frame"):
        getattr(L, f"pt_{who}_set_roughness").argtypes = [vp, rp, C.c_int32]
        getattr(L, f"pt_{who}_get_roughness").argtypes = [vp, rp, ip]
    L.pt_scene_get_mtl_roughness.argtypes = [vp, fp]
    for who in ("scene", "frame"):
        getattr(L, f"pt_{who}_set_direct_lighting").argtypes = [vp, C.c_int32]
        getattr(L, f"pt_{who}_get_direct_lighting").argtypes = [vp, ip]
        getattr(L, f"pt_{who}_get_lights").argtypes = [vp, vp, ip, fp]
    for who in ("scene", "frame"):
        getattr(L, f"pt_{who}_set_environment_sampling").argtypes = [vp, C.POINTER(C.c_float)]
        getattr(L, f"pt_{who}_get_environment_sampling").argtypes = [vp, ip, C.POINTER(C.c_float)]
        getattr(L, f"pt_{who}_get_environment_sampling_table").argtypes = [vp, vp, ip, C.POINTER(C.c_float)]
        getattr(L, f"pt_{who}_set_roulette").argtypes = [vp, C.c_int32, C.c_float]
        getattr(L, f"pt_{who}_get_roulette").argtypes = [vp, ip, C.POINTER(C.c_float)]
    L.pt_roulette_step.argtypes = [C.c_int32, C.c_float, fp, C.POINTER(C.c_uint32), fp, ip]
    L.pt_envdirect_term.argtypes = [C.c_int32, vp, C.c_int32, C.c_float, C.c_int32, fp, fp, fp, fp, fp] + [C.POINTER(C.c_uint32)] * 4 + [ip, fp, fp, fp, ip]
    L.pt_direct_term.argtypes = [C.c_int32, vp, C.c_int32, C.c_float, fp, fp, fp, fp, fp] + [C.POINTER(C.c_uint32)] * 3 + [ip, fp, fp, fp, ip]
    L.pt_rough_step.argtypes = [C.c_int32, fp, fp, fp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), fp, fp, fp]
    L.pt_scene_get_map_kd.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p)]
    L.pt_texture_load_bmp.argtypes = [C.c_char_p, C.c_float, ip, ip, fp]
    L.pt_texture_lookup.argtypes = [C.c_int32, C.c_int32, fp, C.c_int32, C.c_int32, fp, fp, ip]
    L.pt_environment_from_equirect.argtypes = [C.c_int32, C.c_int32, fp, ep, C.c_int32, fp]
    L.pt_environment_lookup.argtypes = [C.c_int32, fp, C.c_int32, fp, fp]
    L.pt_render_features_host.argtypes = [vp, C.POINTER(RenderParams), ip, fp, fp, fp, fp]
    L.pt_denoise_host.argtypes = [C.c_int, C.c_int32, C.c_int32, fp, fp, ip, fp, fp, fp, ip, C.POINTER(DenoiseParams), fp, ip, fp]
    L.pt_tonemap.argtypes = [C.c_int32, C.c_int32, fp, ip, C.c_float, fp]
    L.pt_temporal_create.argtypes = [vp, C.c_int32, C.c_int32, C.c_float, C.POINTER(vp)]
    L.pt_temporal_push_host.argtypes = [vp, fp, fp, ip, C.POINTER(TemporalParams), C.POINTER(DenoiseParams), fp, fp, ip, fp, fp, ip, fp]
    L.pt_temporal_reset.argtypes = [vp]
    L.pt_temporal_destroy.argtypes = [vp]
    L.pt_temporal_destroy.restype = None
    bp = C.POINTER(C.c_uint8)
    L.pt_display_create.argtypes = [vp, C.c_float, C.POINTER(vp)]
    L.pt_display_create_frame.argtypes = [vp, C.c_float, C.POINTER(vp)]
    L.pt_display_present.argtypes = [vp, C.POINTER(DisplayParams), bp, C.POINTER(DisplayInfo)]
    L.pt_display_present_scaled.argtypes = [vp, C.POINTER(DisplayParams), C.POINTER(UpsampleParams), bp, C.POINTER(DisplayInfo)]
    L.pt_upsample_host.argtypes = [C.c_int, C.c_int32, C.c_int32, fp, ip, fp, fp, fp, ip, C.POINTER(UpsampleParams), fp, ip, fp]
    L.pt_display_reset.argtypes = [vp]
    L.pt_display_destroy.argtypes = [vp]
    L.pt_display_destroy.restype = None
    L.pt_display_bytes_host.argtypes = [C.c_int, C.c_int32, C.c_int32, fp, ip, C.c_float, bp, C.POINTER(DisplayInfo)]
    L.pt_display_table.argtypes = [C.c_float, ip, fp, fp, fp]
    up = C.POINTER(C.c_uint32)
    L.pt_grade_host.argtypes = [C.c_int32, C.c_int32, fp, ip, C.c_float, C.c_int32, fp]
    L.pt_meter_host.argtypes = [C.c_int, C.c_int32, C.c_int32, fp, ip, up, fp]
    L.pt_exposure_from_histogram.argtypes = [up, C.POINTER(GradeParams), C.c_int32, C.c_float, fp, fp]
    L.pt_display_present_graded.argtypes = [vp, C.POINTER(DisplayParams), C.POINTER(UpsampleParams), C.POINTER(GradeParams), bp,
                                            C.POINTER(DisplayInfo), C.POINTER(GradeInfo)]
    L.pt_display_bytes_graded_host.argtypes = [C.c_int, C.c_int32, C.c_int32, fp, ip, C.c_float, C.POINTER(GradeParams), C.c_int32, C.c_float, bp,
                                               C.POINTER(DisplayInfo), C.POINTER(GradeInfo)]
    L.pt_bloom_host.argtypes = [C.c_int, C.c_int32, C.c_int32, fp, ip, C.c_float, C.POINTER(BloomParams), fp, fp]
    L.pt_display_present_bloom.argtypes = [vp, C.POINTER(DisplayParams), C.POINTER(UpsampleParams), C.POINTER(GradeParams), C.POINTER(BloomParams),
                                           bp, C.POINTER(DisplayInfo), C.POINTER(GradeInfo)]
    L.pt_local_host.argtypes = [C.c_int, C.c_int32, C.c_int32, fp, ip, C.c_float, C.POINTER(LocalParams), fp, fp]
    L.pt_display_present_local.argtypes = [vp, C.POINTER(DisplayParams), C.POINTER(UpsampleParams), C.POINTER(GradeParams), C.POINTER(BloomParams),
                                           C.POINTER(LocalParams), bp, C.POINTER(DisplayInfo), C.POINTER(GradeInfo)]
    cp = C.POINTER(ColourParams)
    L.pt_lut_create.argtypes = [C.c_int32, fp, C.POINTER(vp)]
    L.pt_lut_load_cube.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.pt_lut_size.argtypes = [vp, ip]
    L.pt_lut_destroy.argtypes = [vp]
    L.pt_lut_destroy.restype = None
    L.pt_colour_matrix.argtypes = [cp, fp]
    L.pt_colour_host.argtypes = [C.c_int32, C.c_int32, fp, ip, C.c_float, C.c_int32, cp, fp]
    L.pt_display_bytes_colour_host.argtypes = [C.c_int, C.c_int32, C.c_int32, fp, ip, C.c_float, C.POINTER(GradeParams), cp, C.c_int32, C.c_float, bp,
                                               C.POINTER(DisplayInfo), C.POINTER(GradeInfo)]
    L.pt_display_present_colour.argtypes = [vp, C.POINTER(DisplayParams), C.POINTER(UpsampleParams), C.POINTER(GradeParams), C.POINTER(BloomParams),
                                            C.POINTER(LocalParams), cp, bp, C.POINTER(DisplayInfo), C.POINTER(GradeInfo)]
    L.pt_optics_host.argtypes = [C.c_int, C.c_int32, C.c_int32, fp, ip, C.POINTER(OpticsParams), fp, ip, fp]
    L.pt_display_present_optics.argtypes = [vp, C.POINTER(DisplayParams), C.POINTER(UpsampleParams), C.POINTER(GradeParams), C.POINTER(BloomParams),
                                            C.POINTER(LocalParams), cp, C.POINTER(OpticsParams), bp, C.POINTER(DisplayInfo), C.POINTER(GradeInfo)]
    L.pt_sharpen_host.argtypes = [C.c_int, C.c_int32, C.c_int32, fp, ip, C.c_float, C.POINTER(SharpenParams), fp, fp]
    L.pt_display_present_sharpen.argtypes = [vp, C.POINTER(DisplayParams), C.POINTER(UpsampleParams), C.POINTER(GradeParams), C.POINTER(BloomParams),
                                             C.POINTER(LocalParams), cp, C.POINTER(OpticsParams), C.POINTER(SharpenParams), bp,
                                             C.POINTER(DisplayInfo), C.POINTER(GradeInfo)]
    L.pt_grain_quantize.argtypes = [C.c_int32, C.c_int32, fp, ip, C.c_float, C.POINTER(GrainParams), bp]
    L.pt_display_bytes_grain_host.argtypes = [C.c_int, C.c_int32, C.c_int32, fp, ip, C.c_float, C.POINTER(GradeParams), cp, C.POINTER(GrainParams),
                                              C.c_int32, C.c_float, bp, C.POINTER(DisplayInfo), C.POINTER(GradeInfo)]
    L.pt_display_present_grain.argtypes = [vp, C.POINTER(DisplayParams), C.POINTER(UpsampleParams), C.POINTER(GradeParams), C.POINTER(BloomParams),
                                           C.POINTER(LocalParams), cp, C.POINTER(OpticsParams), C.POINTER(SharpenParams), C.POINTER(GrainParams), bp,
                                           C.POINTER(DisplayInfo), C.POINTER(GradeInfo)]
    lin = C.POINTER(LinearParams)
    L.pt_linear_bytes.restype = C.c_size_t
    L.pt_linear_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.pt_linear_encode.argtypes = [C.c_int32, C.c_int32, fp, ip, C.c_float, lin, bp]
    L.pt_linear_encode_device_host.argtypes = [C.c_int, C.c_int32, C.c_int32, fp, ip, C.c_float, lin, bp, C.POINTER(DisplayInfo)]
    L.pt_display_present_linear.argtypes = [vp, C.POINTER(DisplayParams), C.POINTER(UpsampleParams), C.POINTER(GradeParams), C.POINTER(BloomParams),
                                            C.POINTER(LocalParams), cp, C.POINTER(OpticsParams), C.POINTER(SharpenParams), C.POINTER(GrainParams), lin,
                                            bp, bp, C.POINTER(DisplayInfo), C.POINTER(GradeInfo)]
    L.pt_write_pfm.argtypes = [C.c_char_p, C.c_int32, C.c_int32, bp]
    L.pt_write_hdr.argtypes = [C.c_char_p, C.c_int32, C.c_int32, bp]
    if hasattr(L, "pt_test_set_mutation"):
        L.pt_test_set_mutation.argtypes = [C.c_char_p, C.c_double]
    if hasattr(L, "pt_test_live_device_objects"):
        L.pt_test_live_device_objects.argtypes = []
        L.pt_test_live_device_objects.restype = C.c_long
    return L


def lib():
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH)
    return _lib


def _check(status, L=None):
    if status != PT_OK:
        raise PtError(status, (L or lib()).pt_last_error().decode(errors="replace"))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def device_count():
    return lib().pt_device_count()


class _EnvironmentMethods:
    """set_environment / set_environment_map / environment of a Scene (pt_scene_*) and of a Frame (pt_frame_*: every device's copy)."""
    _env_prefix = "pt_scene_"

    def _env_fn(self, name):
        return getattr(self._L, self._env_prefix + name)

    def set_environment(self, source, gain=1.0, rotate=0.0, size=0):
        """-ENV: an HDR panorama as a light source.  `source` is the path of a Radiance .hdr or a PFM, or an (h, w, 3) equirectangular
        picture; None or "" removes the environment.  gain scales it, rotate turns it about +y (degrees), size is N of the octahedral
        map it is resampled into (0 = by the picture's height).  Not together with a skybox."""
        prm = EnvironmentParams(gain, rotate, size)
        if source is None or isinstance(source, (str, bytes, os.PathLike)):
            path = os.fsencode(source) if source else b""
            _check(self._env_fn("set_environment_file")(self._h, path, C.byref(prm)), self._L)
            return
        pic = np.ascontiguousarray(source, np.float32)
        if pic.ndim != 3 or pic.shape[2] != 3:
            raise ValueError("set_environment: a picture must be (h, w, 3)")
        _check(self._env_fn("set_environment_equirect")(self._h, pic.shape[1], pic.shape[0], _fp(pic), C.byref(prm)), self._L)

    def set_environment_map(self, env_map):
        """pt_scene_set_environment_map / pt_frame_set_environment_map: an (n, n, 3) octahedral map given directly."""
        m = np.ascontiguousarray(env_map, np.float32)
        if m.ndim != 3 or m.shape[0] != m.shape[1] or m.shape[2] != 3:
            raise ValueError("set_environment_map: env_map must be (n, n, 3)")
        _check(self._env_fn("set_environment_map")(self._h, m.shape[0], _fp(m)), self._L)

    def environment(self):
        """The handle's octahedral map, (n, n, 3), or None if it has no environment."""
        n = C.c_int32()
        _check(self._env_fn("get_environment")(self._h, C.byref(n), None), self._L)
        if n.value == 0:
            return None
        m = np.zeros((n.value, n.value, 3), np.float32)
        _check(self._env_fn("get_environment")(self._h, C.byref(n), _fp(m)), self._L)
        return m


class _DielectricMethods:
    """set_dielectrics / dielectrics of a Scene (pt_scene_*) and of a Frame (pt_frame_*: every device's copy)."""
    _glass_prefix = "pt_scene_"

    def set_dielectrics(self, entries):
        """-GLASS: marks materials as smooth dielectrics.  `entries` is a list of pt.dielectric(material, ior, tint); None or an
        empty list clears it.  Refused: an index outside the scene or listed twice, an ior outside 0.125 .. 8, a tint component
        outside 0 .. 1, an emissive material."""
        entries = list(entries or [])
        arr = (Dielectric * len(entries))(*entries) if entries else None
        _check(getattr(self._L, self._glass_prefix + "set_dielectrics")(self._h, arr, len(entries)), self._L)

    def dielectrics(self):
        """The handle's dielectrics, a list of Dielectric in the order given ([] without any)."""
        get = getattr(self._L, self._glass_prefix + "get_dielectrics")
        n = C.c_int32()
        _check(get(self._h, None, C.byref(n)), self._L)
        arr = (Dielectric * max(n.value, 1))()
        _check(get(self._h, arr, C.byref(n)), self._L)
        return [dielectric(e.material, e.ior, tuple(e.tint)) for e in arr[:n.value]]


class _RoughMethods:
    """set_roughness / roughness / mtl_roughness of a Scene (pt_scene_*) and of a Frame (pt_frame_*: every device's copy)."""
    _rough_prefix = "pt_scene_"

    def set_roughness(self, entries):
        """-ROUGH: gives materials a rough glossy lobe.  `entries` is a list of pt.rough(material, alpha); None or an empty list clears
        it.  Refused: an index outside the scene or listed twice, an alpha outside 2^-10 .. 1, a material without a glossy lobe, a
        dielectric."""
        entries = list(entries or [])
        arr = (Rough * len(entries))(*entries) if entries else None
        _check(getattr(self._L, self._rough_prefix + "set_roughness")(self._h, arr, len(entries)), self._L)

    def roughness(self):
        """The handle's roughness list, a list of Rough in the order given ([] without any)."""
        get = getattr(self._L, self._rough_prefix + "get_roughness")
        n = C.c_int32()
        _check(get(self._h, None, C.byref(n)), self._L)
        arr = (Rough * max(n.value, 1))()
        _check(get(self._h, arr, C.byref(n)), self._L)
        return [rough(e.material, e.alpha) for e in arr[:n.value]]

    def mtl_roughness(self):
        """pt_scene_get_mtl_roughness: each material's Pr value from the MTL as the file gives it, -1 without one."""
        scene = getattr(self, "_scene", self)
        pr = np.zeros(max(scene.counts()[1], 1), np.float32)
        _check(scene._L.pt_scene_get_mtl_roughness(scene._h, _fp(pr)), scene._L)
        return pr[:scene.counts()[1]]


class _DirectMethods:
    """set_direct_lighting / direct_lighting / lights of a Scene (pt_scene_*) and of a Frame (pt_frame_*: every device's copy)."""
    _direct_prefix = "pt_scene_"

    def set_direct_lighting(self, on):
        """-DIRECT: switches direct lighting on or off (pt_hip.h: direct lighting).  Refused: a scene without a light, an emissive
        material in the texture list."""
        _check(getattr(self._L, self._direct_prefix + "set_direct_lighting")(self._h, 1 if on else 0), self._L)

    def direct_lighting(self):
        on = C.c_int32()
        _check(getattr(self._L, self._direct_prefix + "get_direct_lighting")(self._h, C.byref(on)), self._L)
        return bool(on.value)

    def lights(self):
        """The handle's light table: (records of LIGHT_DTYPE in the original triangle order, A)."""
        get = getattr(self._L, self._direct_prefix + "get_lights")
        n, area = C.c_int32(), C.c_float()
        _check(get(self._h, None, C.byref(n), C.byref(area)), self._L)
        arr = np.zeros(max(n.value, 1), LIGHT_DTYPE)
        _check(get(self._h, arr.ctypes.data_as(C.c_void_p), C.byref(n), C.byref(area)), self._L)
        return arr[:n.value], np.float32(area.value)


class _EnvDirectMethods:
    """set_environment_sampling / environment_sampling / environment_sampling_table of a Scene (pt_scene_*) and of a Frame (pt_frame_*:
    every device's copy)."""
    _envdirect_prefix = "pt_scene_"

    def set_environment_sampling(self, share=None):
        """-DIRECT_ENV: switches environment sampling on (pt_hip.h: environment sampling) with the default share (None) or a share
        strictly between 0 and 1, or off (False).  Refused: a handle without an environment, a black environment, a share out of
        range, an emissive material in the texture list."""
        fn = getattr(self._L, self._envdirect_prefix + "set_environment_sampling")
        if share is False:
            _check(fn(self._h, None), self._L)
        else:
            _check(fn(self._h, C.byref(C.c_float(0.0 if share is None or share is True else float(share)))), self._L)

    def environment_sampling(self):
        """None where the switch is off, else the share in use."""
        on, given = C.c_int32(), C.c_float()
        _check(getattr(self._L, self._envdirect_prefix + "get_environment_sampling")(self._h, C.byref(on), C.byref(given)), self._L)
        return self.environment_sampling_table()[1] if on.value else None

    def environment_sampling_table(self):
        """The table the switch uses (or would use with the default share): (records [S, S] of ENV_SAMPLE_DTYPE, the share)."""
        get = getattr(self._L, self._envdirect_prefix + "get_environment_sampling_table")
        cells, share = C.c_int32(), C.c_float()
        _check(get(self._h, None, C.byref(cells), C.byref(share)), self._L)
        arr = np.zeros((cells.value, cells.value), ENV_SAMPLE_DTYPE)
        if cells.value:
            _check(get(self._h, arr.ctypes.data_as(C.c_void_p), C.byref(cells), C.byref(share)), self._L)
        return arr, np.float32(share.value)


class _RouletteMethods:
    """set_roulette / roulette of a Scene (pt_scene_*) and of a Frame (pt_frame_*: every device's copy)."""
    _roulette_prefix = "pt_scene_"

    def set_roulette(self, start=3, floor=ROULETTE_DEFAULT_FLOOR):
        """-RR: sets Russian roulette (pt_hip.h: Russian roulette) from scattering step `start` (>= 1) on with the floor `floor` in
        [2^-10, 1] on the survival probability; None or 0 clears it.  Refused: a handle with neither direct lighting nor environment
        sampling on, a negative start, a floor out of range."""
        fn = getattr(self._L, self._roulette_prefix + "set_roulette")
        if start is None or start is False:
            _check(fn(self._h, 0, C.c_float(0.0)), self._L)
        else:
            _check(fn(self._h, int(start), C.c_float(float(floor))), self._L)

    def roulette(self):
        """None where roulette is not set, else (start, floor)."""
        start, floor = C.c_int32(), C.c_float()
        _check(getattr(self._L, self._roulette_prefix + "get_roulette")(self._h, C.byref(start), C.byref(floor)), self._L)
        return (start.value, np.float32(floor.value)) if start.value > 0 else None


class _TextureMethods:
    """set_texcoords / texcoords / set_textures / textures of a Scene (pt_scene_*) and of a Frame (pt_frame_*: every device's copy)."""
    _tex_prefix = "pt_scene_"

    def _tex_fn(self, name):
        return getattr(self._L, self._tex_prefix + name)

    def set_texcoords(self, uv):
        """The handle's texture coordinates: (n_tri, 3, 2) -- (u, v) per corner of every triangle -- or None to clear them."""
        if uv is None:
            _check(self._tex_fn("set_texcoords")(self._h, None), self._L)
            return
        a = np.ascontiguousarray(uv, np.float32)
        if a.size != 6 * self._n_tri():
            raise ValueError("set_texcoords: 6 floats per triangle")
        _check(self._tex_fn("set_texcoords")(self._h, _fp(a)), self._L)

    def texcoords(self):
        """(n_tri, 3, 2), or None if the handle has none (a scene loaded from an OBJ has the file's vt)."""
        has = C.c_int32()
        _check(self._tex_fn("get_texcoords")(self._h, None, C.byref(has)), self._L)
        if not has.value:
            return None
        a = np.zeros((self._n_tri(), 3, 2), np.float32)
        _check(self._tex_fn("get_texcoords")(self._h, _fp(a), C.byref(has)), self._L)
        return a

    def set_textures(self, entries):
        """-TEXTURE: `entries` is a list of pt.texture(material, texels, filter); None or an empty list clears it.  Refused: an index
        outside the scene or listed twice, a side above TEXTURE_MAX_SIDE, a negative or non-finite texel, an unknown filter, a
        dielectric material, a handle without texture coordinates."""
        entries = list(entries or [])
        arr = (TextureEntry * len(entries))(*[TextureEntry(e.material, e.texels.shape[1], e.texels.shape[0], e.filter, _fp(e.texels)) for e in entries]) if entries else None
        _check(self._tex_fn("set_textures")(self._h, arr, len(entries)), self._L)

    def textures(self):
        """The handle's textures, a list of Texture in the order given ([] without any)."""
        n = C.c_int32()
        _check(self._tex_fn("get_textures")(self._h, None, C.byref(n)), self._L)
        arr = (TextureEntry * max(n.value, 1))()
        _check(self._tex_fn("get_textures")(self._h, arr, C.byref(n)), self._L)
        return [Texture(e.material, np.ctypeslib.as_array(e.rgb, (e.height, e.width, 3)).copy(), e.filter) for e in arr[:n.value]]


class _SmoothMethods:
    """set_shading_normals / shading_normals / vertex_normals of a Scene (pt_scene_*) and of a Frame (pt_frame_*: every device's copy)."""
    _smooth_prefix = "pt_scene_"

    def set_shading_normals(self, normals):
        """-SMOOTH: the handle's shading normals, (n_tri, 3, 3) -- a normal per corner of every triangle -- or None to clear them.
        Zeros mean "use the stored normal"; a component that is not finite is refused."""
        fn = getattr(self._L, self._smooth_prefix + "set_shading_normals")
        if normals is None:
            _check(fn(self._h, None), self._L)
            return
        a = np.ascontiguousarray(normals, np.float32)
        if a.size != 9 * self._n_tri():
            raise ValueError("set_shading_normals: 9 floats per triangle")
        _check(fn(self._h, _fp(a)), self._L)

    def _normals(self, fn):
        has = C.c_int32()
        _check(fn(self._h, None, C.byref(has)), self._L)
        if not has.value:
            return None
        a = np.zeros((self._n_tri(), 3, 3), np.float32)
        _check(fn(self._h, _fp(a), C.byref(has)), self._L)
        return a

    def shading_normals(self):
        """(n_tri, 3, 3), or None if the handle has none."""
        return self._normals(getattr(self._L, self._smooth_prefix + "get_shading_normals"))

    def vertex_normals(self):
        """pt_scene_get_vertex_normals: the vn the loader kept, (n_tri, 3, 3), or None for a scene made from arrays."""
        scene = getattr(self, "_scene", self)
        return scene._normals(scene._L.pt_scene_get_vertex_normals)


class Scene(_EnvironmentMethods, _DielectricMethods, _TextureMethods, _SmoothMethods, _RoughMethods, _DirectMethods, _EnvDirectMethods, _RouletteMethods):
    """Owns a pt_scene handle (Scene + LoadModel of the reference, scene.h:17-19)."""

    def __init__(self, handle, library=None):
        self._h = handle
        self._L = library or lib()

    @classmethod
    def load_obj(cls, model_dir, model_name, device=0, library=None, geometric_planes=False):
        """pt_scene_load_obj; geometric_planes (PT_LOAD_GEOMETRIC_PLANES): every plane from the cross product, whatever vn the face names."""
        L = library or lib()
        h = C.c_void_p()
        if geometric_planes:
            _check(L.pt_scene_load_obj_ex(model_dir.encode(), model_name.encode(), device, LOAD_GEOMETRIC_PLANES, C.byref(h)), L)
        else:
            _check(L.pt_scene_load_obj(model_dir.encode(), model_name.encode(), device, C.byref(h)), L)
        return cls(h, L)

    load = load_obj

    @classmethod
    def create(cls, triangles, triangle_material, materials, device=0, library=None):
        L = library or lib()
        t = np.ascontiguousarray(triangles, np.float32).reshape(-1, 14)
        m = np.ascontiguousarray(triangle_material, np.int32)
        k = np.ascontiguousarray(materials, np.float32).reshape(-1, 10)
        h = C.c_void_p()
        _check(L.pt_scene_create(_fp(t), _ip(m), len(t), _fp(k), len(k), device, C.byref(h)), L)
        return cls(h, L)

    def _n_tri(self):
        return self.counts()[0]

    def texture_records(self):
        """pt_scene_get_texture_records: (n_tri, 8), the per-triangle records the texture kernels take a hit point's barycentrics from."""
        r = np.zeros((self._n_tri(), 8), np.float32)
        _check(self._L.pt_scene_get_texture_records(self._h, _fp(r)), self._L)
        return r

    def map_kd(self):
        """The file name of each material's map_Kd line in the model's MTL ("" where it has none)."""
        out = []
        for m in range(self.counts()[1]):
            name = C.c_char_p()
            _check(self._L.pt_scene_get_map_kd(self._h, m, C.byref(name)), self._L)
            out.append((name.value or b"").decode(errors="replace"))
        return out

    def counts(self):
        nt, nm = C.c_int32(), C.c_int32()
        _check(self._L.pt_scene_counts(self._h, C.byref(nt), C.byref(nm)), self._L)
        return nt.value, nm.value

    def triangles(self):
        nt, _ = self.counts()
        t = np.zeros((nt, 14), np.float32)
        m = np.zeros(nt, np.int32)
        _check(self._L.pt_scene_get_triangles(self._h, _fp(t), _ip(m)), self._L)
        return t, m

    def materials(self):
        _, nm = self.counts()
        k = np.zeros((nm, 10), np.float32)
        _check(self._L.pt_scene_get_materials(self._h, _fp(k)), self._L)
        return k

    def render_host(self, width, height, spp, mrr, *, eps=1e-4, error=-1.0, seed=42, rows=None, pass_begin=0,
                    accum=None, want_stats=True, rng_policy=RNG_COUNTER, row_stride=0):
        r0, r1 = rows if rows is not None else (0, height)
        p = RenderParams(width, height, r0, r1, pass_begin, spp, mrr, eps, error, seed, rng_policy, row_stride)
        n = band_rows(p, self._L) * width
        if accum is None:
            s, s2, c = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        else:
            s, s2, c = accum
        st = RenderStats()
        _check(self._L.pt_render_host(self._h, C.byref(p), _fp(s), _fp(s2), _ip(c), C.byref(st) if want_stats else None), self._L)
        return s, s2, c, st.as_dict()

    def clone_to_device(self, device):
        """The same scene on another device; host side (parsed model, hierarchies) shared."""
        h = C.c_void_p()
        _check(self._L.pt_scene_clone_to_device(self._h, device, C.byref(h)), self._L)
        return Scene(h, self._L)

    def timings(self):
        t = (C.c_double * 2)()
        _check(self._L.pt_scene_timings(self._h, t), self._L)
        return {"load_s": t[0], "hierarchy_build_s": t[1]}

    def set_skybox(self, path):
        """-SKYBOX: a 24-bit BMP sampled by rays that hit nothing (scene.cpp:126-154); None or "" removes it."""
        _check(self._L.pt_scene_set_skybox_bmp(self._h, (path or "").encode()), self._L)

    def skybox_size(self):
        w, h = C.c_int32(), C.c_int32()
        _check(self._L.pt_scene_skybox_size(self._h, C.byref(w), C.byref(h)), self._L)
        return w.value, h.value

    def set_camera(self, camera):
        """pt_scene_set_camera: a Camera (or an (origin, right, up, forward) tuple) for this handle; None = the reference's."""
        if camera is not None and not isinstance(camera, Camera):
            camera = Camera.of(*camera)
        _check(self._L.pt_scene_set_camera(self._h, C.byref(camera) if camera is not None else None), self._L)

    def camera(self):
        """The handle's Camera, or None if it has none (it then renders the reference's view, REFERENCE_CAMERA)."""
        cam, is_set = Camera(), C.c_int32()
        _check(self._L.pt_scene_get_camera(self._h, C.byref(cam), C.byref(is_set)), self._L)
        return cam if is_set.value else None

    def set_lens(self, radius, focus_distance=None):
        """pt_scene_set_lens: a thin lens of aperture `radius` focused at `focus_distance` (or a Lens); None or radius 0 = a
        pinhole.  On a handle without a camera the lens applies to the reference camera."""
        _check(self._L.pt_scene_set_lens(self._h, _lens_arg(radius, focus_distance)), self._L)

    def lens(self):
        """The handle's Lens, or None if it has none."""
        lens, is_set = Lens(), C.c_int32()
        _check(self._L.pt_scene_get_lens(self._h, C.byref(lens), C.byref(is_set)), self._L)
        return lens if is_set.value else None

    def set_camera_motion(self, end_camera):
        """pt_scene_set_camera_motion: the camera moves from the handle's camera to `end_camera` (a Camera or its four vectors)
        while the shutter is open, every path at a time of its own; None, or an end pose equal to the camera, = no motion.
        The handle's camera, lens and motion are checked against one another whenever one is set: before moving the camera of a
        handle that has a motion, clear the motion (None), then set_camera, then the new end pose."""
        if end_camera is not None and not isinstance(end_camera, Camera):
            end_camera = Camera.of(*end_camera)
        _check(self._L.pt_scene_set_camera_motion(self._h, C.byref(end_camera) if end_camera is not None else None), self._L)

    def get_camera_motion(self):
        """The handle's end pose (a Camera), or None if it has no motion."""
        end, is_set = Camera(), C.c_int32()
        _check(self._L.pt_scene_get_camera_motion(self._h, C.byref(end), C.byref(is_set)), self._L)
        return end if is_set.value else None

    def set_projection(self, projection_):
        """pt_scene_set_projection: a Projection (pt.projection), or a kind that needs no angles ("ortho", "equirect" = the full
        sphere); None or "perspective" = the pinhole.  Not together with a lens or a camera motion: clear those first."""
        _check(self._L.pt_scene_set_projection(self._h, _projection_arg(projection_, self._L)), self._L)

    def get_projection(self):
        """The handle's Projection, or None if it has none (the pinhole)."""
        p, is_set = Projection(), C.c_int32()
        _check(self._L.pt_scene_get_projection(self._h, C.byref(p), C.byref(is_set)), self._L)
        return p if is_set.value else None

    def cull_tables(self, eps=1e-4):
        """The culling hierarchy for `eps` (diagnostics): dict of clusters, spheres, bary records, constants."""
        counts = np.zeros(4, np.int32)
        _check(self._L.pt_scene_cull_tables(self._h, eps, _ip(counts), None, None, None, None), self._L)
        cl = np.zeros((counts[0], 16), np.float32)
        sp = np.zeros((counts[1], 4), np.float32)
        ba = np.zeros((counts[2], 12), np.float32)
        k = np.zeros(5, np.float32)
        _check(self._L.pt_scene_cull_tables(self._h, eps, _ip(counts), _fp(cl), _fp(sp), _fp(ba), _fp(k)), self._L)
        meta = cl[:, 4:16].view(np.uint32)
        return {"cluster_sphere": cl[:, :4], "first_tri": meta[:, 0].astype(int), "n_tri": meta[:, 1].astype(int),
                "kind": meta[:, 2].astype(int), "data_off": meta[:, 3].astype(int), "n_levels": meta[:, 4].astype(int),
                "level_off": np.concatenate([np.zeros((len(cl), 1), int), meta[:, 5:12].astype(int)], 1),
                "spheres": sp, "bary": ba,
                "constants": dict(zip(["k1", "k2", "a_max", "m0", "t_guard"], k.tolist())), "n_large": int(counts[3])}

    def cull_layout(self, eps=1e-4):
        """Slot order of the hierarchy: dict with slot_triangle (original index per slot, -1 = padding), node counts."""
        counts = np.zeros(4, np.int32)
        _check(self._L.pt_scene_cull_layout(self._h, eps, _ip(counts), None, None), self._L)
        st = np.zeros(counts[0], np.int32)
        nodes = np.zeros((counts[1], 64), np.uint8)
        _check(self._L.pt_scene_cull_layout(self._h, eps, _ip(counts), _ip(st), nodes.ctypes.data_as(C.c_void_p)), self._L)
        return {"slot_triangle": st, "bvh": nodes, "bvh_inner_nodes": int(counts[2]), "clusters": int(counts[3]),
                "bvh_depth": bvh_depth(nodes)}

    def trace_rays(self, origins, directions, eps=1e-4):
        """Closest hit per ray (scene.cpp:114-120).  directions must be unit length (normalised as ray.h:23 does)."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        idx = np.full(len(o), -2, np.int32)
        t = np.zeros(len(o), np.float32)
        _check(self._L.pt_trace_rays_host(self._h, len(o), _fp(o), _fp(d), eps, _ip(idx), _fp(t)), self._L)
        return idx, t

    def render_features(self, width, height, rows=None, eps=1e-4, row_stride=0):
        """pt_render_features_host: what the camera sees first in every pixel of rows [r0, r1) -- dict of hit_index [n] (-1 = a miss),
        hit_t [n] (+inf), position / normal / albedo [n, 3] (zeros).  The lens is ignored."""
        r0, r1 = rows if rows is not None else (0, height)
        p = RenderParams(width, height, r0, r1, 0, 0, 0, eps, -1.0, 0, 0, row_stride)
        n = max(0, r1 - r0) * max(0, width)
        out = {"hit_index": np.full(n, -2, np.int32), "hit_t": np.zeros(n, np.float32), "position": np.zeros((n, 3), np.float32),
               "normal": np.zeros((n, 3), np.float32), "albedo": np.zeros((n, 3), np.float32)}
        _check(self._L.pt_render_features_host(self._h, C.byref(p), _ip(out["hit_index"]), _fp(out["hit_t"]), _fp(out["position"]),
                                               _fp(out["normal"]), _fp(out["albedo"])), self._L)
        return out

    def render_device(self, params, d_sum, d_sum2, d_count, stream=None, want_stats=False):
        """d_* are raw device pointers (ints), e.g. torch tensors' data_ptr(); stream is a hipStream_t value."""
        st = RenderStats()
        _check(self._L.pt_render_device(self._h, C.byref(params), C.c_void_p(d_sum), C.c_void_p(d_sum2),
                                      C.c_void_p(d_count), C.c_void_p(stream or 0),
                                      C.byref(st) if want_stats else None), self._L)
        return st.as_dict() if want_stats else None

    def close(self):
        if self._h:
            self._L.pt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def band_rows(params, L=None):
    """Rows the accumulator buffers of a call with these RenderParams hold (pt_band_rows)."""
    return (L or lib()).pt_band_rows(C.byref(params))


def interleaved_rows(height, row_begin, row_stride):
    """Image rows, in buffer order, of the interleaved band (row_begin, height, row_stride): -1 for buffer rows beyond the image."""
    out = []
    for t0 in range(row_begin, height, 8 * max(1, row_stride)):
        out += [y if y < height else -1 for y in range(t0, t0 + 8)]
    return np.array(out, np.int64)


class Session:
    """pt_session: one row band's accumulators kept on the device between pass slices (progressive driver)."""

    def __init__(self, scene, width, height, rows=None, row_stride=0):
        r0, r1 = rows if rows is not None else (0, height)
        self._scene, self._L = scene, scene._L
        self.width, self.height, self.rows, self.row_stride = width, height, (r0, r1), row_stride
        self._h = C.c_void_p()
        if row_stride > 1:
            _check(self._L.pt_session_create_strided(scene._h, width, height, r0, r1, row_stride, C.byref(self._h)), self._L)
        else:
            _check(self._L.pt_session_create(scene._h, width, height, r0, r1, C.byref(self._h)), self._L)

    def render(self, pass_begin, pass_count, mrr, *, eps=1e-4, error=-1.0, seed=42, want_stats=False):
        p = RenderParams(self.width, self.height, self.rows[0], self.rows[1], pass_begin, pass_count, mrr, eps, error, seed, 0, self.row_stride)
        st = RenderStats()
        _check(self._L.pt_session_render(self._h, C.byref(p), C.byref(st) if want_stats else None), self._L)
        return st.as_dict() if want_stats else None

    def read(self):
        n = band_rows(RenderParams(self.width, self.height, self.rows[0], self.rows[1], 0, 0, 0, 0, 0, 0, 0, self.row_stride), self._L) * self.width
        s, s2, c = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        _check(self._L.pt_session_read(self._h, _fp(s), _fp(s2), _ip(c)), self._L)
        return s, s2, c

    def clear(self):
        _check(self._L.pt_session_clear(self._h), self._L)

    def close(self):
        if self._h:
            self._L.pt_session_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Temporal:
    """pt_temporal: the history of one view sequence on the scene's device.  push() merges the reprojected history into a frame's
    accumulators (the scene's camera at the time of the call says where the frame was seen from) and optionally denoises the
    merged frame in the same chain on the device."""

    def __init__(self, scene, width, height, eps=1e-4):
        self._scene, self._L = scene, scene._L      # the scene must outlive the history
        self.width, self.height = width, height
        self._h = C.c_void_p()
        _check(self._L.pt_temporal_create(scene._h, width, height, eps, C.byref(self._h)), self._L)

    def push(self, s, s2, c, *, max_frames=0.0, sigma_plane=0.0, min_normal_dot=0.0, denoise=None, want_ms=False):
        """pt_temporal_push_host.  `denoise`: None, a DenoiseParams, or a dict of pt.denoise's keyword parameters (levels, ...).
        Returns a dict: sum, sum2 [n, 3], count [n], history_frames [n]; with `denoise` also mean_rgb [n, 3], mean_count [n]; with
        want_ms also kernel_ms."""
        n = self.width * self.height
        s, s2 = np.ascontiguousarray(s, np.float32), np.ascontiguousarray(s2, np.float32)
        c = np.ascontiguousarray(c, np.int32)
        if s.size != 3 * n or s2.size != 3 * n or c.size != n:
            raise ValueError("Temporal.push: the accumulators do not hold width x height pixels")
        if isinstance(denoise, dict):
            denoise = DenoiseParams(denoise.get("levels", 5), denoise.get("sigma_luminance", 0.0), denoise.get("sigma_plane", 0.0),
                                    denoise.get("normal_power_log2", 0), denoise.get("demodulate_albedo", 0))
        prm = TemporalParams(max_frames, sigma_plane, min_normal_dot)
        out = {"sum": np.zeros((n, 3), np.float32), "sum2": np.zeros((n, 3), np.float32), "count": np.zeros(n, np.int32),
               "history_frames": np.zeros(n, np.float32)}
        if denoise is not None:
            out["mean_rgb"], out["mean_count"] = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        ms = C.c_float()
        _check(self._L.pt_temporal_push_host(self._h, _fp(s), _fp(s2), _ip(c), C.byref(prm), C.byref(denoise) if denoise is not None else None,
                                             _fp(out["sum"]), _fp(out["sum2"]), _ip(out["count"]), _fp(out["history_frames"]),
                                             _fp(out["mean_rgb"]) if denoise is not None else None,
                                             _ip(out["mean_count"]) if denoise is not None else None, C.byref(ms)), self._L)
        if want_ms:
            out["kernel_ms"] = ms.value
        return out

    def reset(self):
        """Forget the history: the next push is a first frame."""
        _check(self._L.pt_temporal_reset(self._h), self._L)

    def close(self):
        if self._h:
            self._L.pt_temporal_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _upsample_params(upsample):
    """An UpsampleParams, or a dict of pt.upsample's keyword parameters (scale, ...) -> an UpsampleParams."""
    if isinstance(upsample, dict):
        return UpsampleParams(upsample.get("scale", 2), upsample.get("sigma_plane", 0.0), upsample.get("normal_power_log2", 0),
                              upsample.get("demodulate_albedo", 0))
    return upsample


def _denoise_params(denoise):
    """None, a DenoiseParams, or a dict of pt.denoise's keyword parameters -> a DenoiseParams (None: levels = 0)."""
    if denoise is None:
        return DenoiseParams()
    if isinstance(denoise, dict):
        return DenoiseParams(denoise.get("levels", 5), denoise.get("sigma_luminance", 0.0), denoise.get("sigma_plane", 0.0),
                             denoise.get("normal_power_log2", 0), denoise.get("demodulate_albedo", 0))
    return denoise


class Display:
    """pt_display: the image bytes of a Session (covering the whole image) or a Frame, made on the device where the accumulators
    lie.  present() runs features, the temporal merge with the display's own history, the denoiser, the tone map and the
    quantization as one chain behind the slices enqueued so far; the bytes equal the host chain's."""

    def __init__(self, session_or_frame, eps=1e-4):
        self._src, self._L = session_or_frame, session_or_frame._L      # the session / frame must outlive the display
        self.width, self.height = session_or_frame.width, session_or_frame.height
        self._h = C.c_void_p()
        create = self._L.pt_display_create_frame if isinstance(session_or_frame, Frame) else self._L.pt_display_create
        _check(create(session_or_frame._h, eps, C.byref(self._h)), self._L)

    def present(self, gamma=None, temporal=None, denoise=None, upsample=None, grade=None, bloom=None, local=None, colour=None, optics=None,
                sharpen=None, grain=None, linear=None, want_bgr=True):
        """pt_display_present.  `temporal`: None (no temporal stage), True, a TemporalParams, or a dict of Temporal.push's
        parameters (max_frames, sigma_plane, min_normal_dot); `denoise`: None, a DenoiseParams, or a dict of pt.denoise's
        parameters.  Returns (bgr uint8 [H, W, 3], info dict).
        `upsample`: None, an UpsampleParams, or a dict of pt.upsample's parameters ({"scale": 2}) -- pt_display_present_scaled: the
        image is then scale times the session's size, bgr uint8 [scale * H, scale * W, 3].
        `grade`: None, a GradeParams, or a dict of its fields ({"curve": "aces", "auto_exposure": True}) -- pt_display_present_graded:
        exposure and a tone curve before the tone map; info then also holds exposure, target, metered, dark.
        `bloom`: None, a BloomParams, or a dict of its fields ({"strength": 0.5}) -- pt_display_present_bloom: the light above the
        threshold spread over its neighbourhood before the grade (`grade` None: no grading at all, as a zeroed GradeParams).
        `local`: None, a LocalParams, or a dict of its fields ({"strength": 1.0}) -- pt_display_present_local: a gain per pixel from
        an edge-aware base of the luminance, after bloom and before the grade (`grade`, `bloom` None: zeroed, as above).
        `colour`: None, a ColourParams, or a dict {"wb": .., "saturation": .., "matrix": .., "lut": Lut} -- pt_display_present_colour: a
        matrix on the mean before the exposure and a 3D LUT behind the curve (`grade`, `bloom`, `local` None: zeroed).
        `optics`: None, an OpticsParams, or a dict of its fields ({"k1": -0.1, "ca": 0.01, "vignette": 1.0}) --
        pt_display_present_optics: distortion, chromatic aberration and vignetting of the linear mean ahead of the meter (the other
        stages None: zeroed).
        `sharpen`: None, a SharpenParams, or a dict of its fields ({"strength": 0.5, "limit": 0.0}) -- pt_display_present_sharpen: a
        contrast-adaptive sharpen of the luminance after local exposure and before the grade (the other stages None: zeroed).
        `grain`: None, a GrainParams, or a dict of its fields ({"strength": 0.2, "size": 1.5, "dither": 1.0, "seed": 7, "frame": 0}) --
        pt_display_present_grain: film grain on the graded value and a triangular dither of its level, inside the display kernel (the
        other stages None: zeroed); advance `frame` once per presented frame.
        `linear`: None, a LinearParams, or a dict {"format": "pfm" | "hdr", "exposed": False} -- pt_display_present_linear: the same
        present also encodes the linear mean the display kernel reads; info["linear"] then holds the body as bytes (pt.write_pfm /
        pt.write_hdr make a file of it).  With every grading stage None the chain has no grade at all.  `want_bgr` False (with
        `linear` only) leaves the display kernel out: the image returned is None."""
        if gamma is None:
            gamma = np.float32(1) / np.float32(2.2)   # config.h:25
        if isinstance(temporal, dict):
            temporal = TemporalParams(temporal.get("max_frames", 0.0), temporal.get("sigma_plane", 0.0), temporal.get("min_normal_dot", 0.0))
        on = temporal is not None and temporal is not False
        prm = DisplayParams(gamma, 1 if on else 0, temporal if isinstance(temporal, TemporalParams) else TemporalParams(),
                            _denoise_params(denoise))
        info = DisplayInfo()
        if linear is not None:
            graded = any(x is not None for x in (grade, bloom, local, colour, optics, sharpen, grain))
            up = _upsample_params(upsample) if upsample is not None else None
            k = up.scale if up is not None and 1 <= up.scale <= UPSAMPLE_MAX_SCALE else 1
            bgr = np.zeros((k * self.height, k * self.width, 3), np.uint8) if want_bgr else None
            lin, ginfo = _linear_params(linear), GradeInfo()
            body = np.zeros(12 * k * k * self.height * self.width, np.uint8)   # (room for either format, whatever the library makes of *lin)
            stages = [None] * 7
            if graded:
                stages = [_grade_params(grade) if grade is not None else GradeParams(), _bloom_params(bloom) if bloom is not None else BloomParams(),
                          _local_params(local) if local is not None else LocalParams(), _colour_params(colour) if colour is not None else ColourParams(),
                          _optics_params(optics) if optics is not None else OpticsParams(), _sharpen_params(sharpen) if sharpen is not None else SharpenParams(),
                          _grain_params(grain) if grain is not None else GrainParams()]
            u8 = C.POINTER(C.c_uint8)
            _check(self._L.pt_display_present_linear(self._h, C.byref(prm), C.byref(up) if up is not None else None,
                                                     *[C.byref(x) if x is not None else None for x in stages], C.byref(lin),
                                                     bgr.ctypes.data_as(u8) if want_bgr else None, body.ctypes.data_as(u8), C.byref(info),
                                                     C.byref(ginfo)), self._L)
            size = self._L.pt_linear_bytes(k * self.width, k * self.height, lin.format)
            out = dict(info.as_dict(), linear=body[:size].tobytes())
            return bgr, dict(out, **ginfo.as_dict()) if graded else out
        if not want_bgr:
            raise ValueError("present: want_bgr=False needs linear=")
        if grade is not None or bloom is not None or local is not None or colour is not None or optics is not None or sharpen is not None or \
                grain is not None:
            gp, ginfo = _grade_params(grade) if grade is not None else GradeParams(), GradeInfo()
            up = _upsample_params(upsample) if upsample is not None else None
            k = up.scale if up is not None and 1 <= up.scale <= UPSAMPLE_MAX_SCALE else 1
            bgr = np.zeros((k * self.height, k * self.width, 3), np.uint8)
            up_arg, out = C.byref(up) if up is not None else None, bgr.ctypes.data_as(C.POINTER(C.c_uint8))
            if grain is not None:
                bp_, lp = _bloom_params(bloom) if bloom is not None else BloomParams(), _local_params(local) if local is not None else LocalParams()
                cp_, op = _colour_params(colour) if colour is not None else ColourParams(), _optics_params(optics) if optics is not None else OpticsParams()
                sp, np_ = _sharpen_params(sharpen) if sharpen is not None else SharpenParams(), _grain_params(grain)
                _check(self._L.pt_display_present_grain(self._h, C.byref(prm), up_arg, C.byref(gp), C.byref(bp_), C.byref(lp), C.byref(cp_),
                                                        C.byref(op), C.byref(sp), C.byref(np_), out, C.byref(info), C.byref(ginfo)), self._L)
            elif sharpen is not None:
                bp_, lp = _bloom_params(bloom) if bloom is not None else BloomParams(), _local_params(local) if local is not None else LocalParams()
                cp_, op = _colour_params(colour) if colour is not None else ColourParams(), _optics_params(optics) if optics is not None else OpticsParams()
                sp = _sharpen_params(sharpen)
                _check(self._L.pt_display_present_sharpen(self._h, C.byref(prm), up_arg, C.byref(gp), C.byref(bp_), C.byref(lp), C.byref(cp_),
                                                          C.byref(op), C.byref(sp), out, C.byref(info), C.byref(ginfo)), self._L)
            elif optics is not None:
                bp_, lp = _bloom_params(bloom) if bloom is not None else BloomParams(), _local_params(local) if local is not None else LocalParams()
                cp_, op = _colour_params(colour) if colour is not None else ColourParams(), _optics_params(optics)
                _check(self._L.pt_display_present_optics(self._h, C.byref(prm), up_arg, C.byref(gp), C.byref(bp_), C.byref(lp), C.byref(cp_),
                                                         C.byref(op), out, C.byref(info), C.byref(ginfo)), self._L)
            elif colour is not None:
                bp_, lp = _bloom_params(bloom) if bloom is not None else BloomParams(), _local_params(local) if local is not None else LocalParams()
                cp_ = _colour_params(colour)
                _check(self._L.pt_display_present_colour(self._h, C.byref(prm), up_arg, C.byref(gp), C.byref(bp_), C.byref(lp), C.byref(cp_), out,
                                                         C.byref(info), C.byref(ginfo)), self._L)
            elif local is not None:
                bp_, lp = _bloom_params(bloom) if bloom is not None else BloomParams(), _local_params(local)
                _check(self._L.pt_display_present_local(self._h, C.byref(prm), up_arg, C.byref(gp), C.byref(bp_), C.byref(lp), out, C.byref(info),
                                                        C.byref(ginfo)), self._L)
            elif bloom is not None:
                bp_ = _bloom_params(bloom)
                _check(self._L.pt_display_present_bloom(self._h, C.byref(prm), up_arg, C.byref(gp), C.byref(bp_), out, C.byref(info),
                                                        C.byref(ginfo)), self._L)
            else:
                _check(self._L.pt_display_present_graded(self._h, C.byref(prm), up_arg, C.byref(gp), out, C.byref(info), C.byref(ginfo)), self._L)
            return bgr, dict(info.as_dict(), **ginfo.as_dict())
        if upsample is not None:
            up = _upsample_params(upsample)
            k = up.scale if 1 <= up.scale <= UPSAMPLE_MAX_SCALE else 1       # (a scale the library refuses: it writes nothing)
            bgr = np.zeros((k * self.height, k * self.width, 3), np.uint8)
            _check(self._L.pt_display_present_scaled(self._h, C.byref(prm), C.byref(up), bgr.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                     C.byref(info)), self._L)
            return bgr, info.as_dict()
        bgr = np.zeros((self.height, self.width, 3), np.uint8)
        _check(self._L.pt_display_present(self._h, C.byref(prm), bgr.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(info)), self._L)
        return bgr, info.as_dict()

    def reset(self):
        """Forget the history: the next present with a temporal stage is a first frame."""
        _check(self._L.pt_display_reset(self._h), self._L)

    def close(self):
        if self._h:
            self._L.pt_display_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def display_bytes(mean_rgb, count, gamma=None, device=0, library=None):
    """pt_display_bytes_host: the display kernel alone on a host image mean_rgb [H, W, 3] with count [H, W] -- the bytes of
    quantize(tonemap(...)).  Returns (bgr uint8 [H, W, 3], info dict)."""
    L = library or lib()
    if gamma is None:
        gamma = np.float32(1) / np.float32(2.2)
    m = np.ascontiguousarray(mean_rgb, np.float32)
    if m.ndim != 3 or m.shape[2] != 3:
        raise ValueError("display_bytes: mean_rgb must be [H, W, 3]")
    h, w, _ = m.shape
    c = np.ascontiguousarray(count, np.int32)
    if c.size != w * h:
        raise ValueError("display_bytes: count does not hold width x height pixels")
    bgr = np.zeros((h, w, 3), np.uint8)
    info = DisplayInfo()
    _check(L.pt_display_bytes_host(device, w, h, _fp(m), _ip(c), C.c_float(gamma), bgr.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(info)), L)
    return bgr, info.as_dict()


def _image_args(name, mean_rgb, count):
    m = np.ascontiguousarray(mean_rgb, np.float32)
    if m.ndim != 3 or m.shape[2] != 3:
        raise ValueError(f"{name}: mean_rgb must be [H, W, 3]")
    c = np.ascontiguousarray(count, np.int32)
    if c.size != m.shape[0] * m.shape[1]:
        raise ValueError(f"{name}: count does not hold width x height pixels")
    return m, c


def grade(mean_rgb, count, exposure=1.0, curve=CURVE_REFERENCE, library=None):
    """pt_grade_host (host only): curve(mean * exposure) per channel of the pixels with samples of mean_rgb [H, W, 3]; the others
    keep their value.  `curve`: a CURVE_* or its name."""
    L = library or lib()
    m, c = _image_args("grade", mean_rgb, count)
    out = np.zeros_like(m)
    _check(L.pt_grade_host(m.shape[1], m.shape[0], _fp(m), _ip(c), C.c_float(exposure), CURVES[curve] if isinstance(curve, str) else curve,
                           _fp(out)), L)
    return out


def bloom(device, mean_rgb, count, exposure=1.0, threshold=1.0, strength=0.5, levels=5, want_ms=False, library=None):
    """pt_bloom_host: the bloom kernels alone on a host image mean_rgb [H, W, 3] with count [H, W] -- mean + glare * strength / levels,
    the glare being the light above threshold / exposure spread by a pyramid of `levels` levels; and the kernels' milliseconds as a
    second value if want_ms."""
    L = library or lib()
    m, c = _image_args("bloom", mean_rgb, count)
    out, ms = np.zeros_like(m), C.c_float()
    prm = BloomParams(threshold, strength, levels)
    _check(L.pt_bloom_host(device, m.shape[1], m.shape[0], _fp(m), _ip(c), C.c_float(exposure), C.byref(prm), _fp(out), C.byref(ms)), L)
    return (out, ms.value) if want_ms else out


def local_exposure(device, mean_rgb, count, exposure=1.0, strength=1.0, pivot=0.18, levels=5, sigma=0.5, want_ms=False, library=None):
    """pt_local_host: the local exposure kernels alone on a host image mean_rgb [H, W, 3] with count [H, W] -- mean * g, the gain g
    = (1 + strength) / (1 + strength * base * exposure / pivot) from an edge-aware base of the luminance (`levels` levels of a 5 x 5
    spline, range weight `sigma`); and the kernels' milliseconds as a second value if want_ms."""
    L = library or lib()
    m, c = _image_args("local_exposure", mean_rgb, count)
    out, ms = np.zeros_like(m), C.c_float()
    prm = LocalParams(strength, pivot, levels, sigma)
    _check(L.pt_local_host(device, m.shape[1], m.shape[0], _fp(m), _ip(c), C.c_float(exposure), C.byref(prm), _fp(out), C.byref(ms)), L)
    return (out, ms.value) if want_ms else out


def sharpen(device, mean_rgb, count, exposure=1.0, strength=1.0, limit=0.0, want_ms=False, library=None):
    """pt_sharpen_host: the sharpening kernels alone on a host image mean_rgb [H, W, 3] with count [H, W] -- mean * g, the gain g
    from a contrast-adaptive sharpen of the compressed luminance (include/pt_hip.h states the arithmetic).  Returns the float32
    image [H, W, 3], with want_ms=True also the HIP-event time of the two kernels."""
    L = library or lib()
    m, c = _image_args("sharpen", mean_rgb, count)
    out, ms = np.empty_like(m), C.c_float(0)
    prm = SharpenParams(strength, limit)
    _check(L.pt_sharpen_host(device, m.shape[1], m.shape[0], _fp(m), _ip(c), C.c_float(exposure), C.byref(prm), _fp(out), C.byref(ms)), L)
    return (out, ms.value) if want_ms else out


def optics(device, mean_rgb, count, k1=0.0, k2=0.0, ca=0.0, vignette=0.0, want_ms=False, library=None):
    """pt_optics_host: the lens optics kernel alone on a host image mean_rgb [H, W, 3] with count [H, W] -- radial distortion
    f = 1 + r2 (k1 + k2 r2), the channels magnified by 1 - ca, 1, 1 + ca, resampled bilinearly, times the vignette 1 / (1 + vignette r2)^2.
    Returns (out [H, W, 3], count_out [H, W]: 1, or 0 where a channel found no sampled tap), and the kernel's milliseconds as a third
    value if want_ms."""
    L = library or lib()
    m, c = _image_args("optics", mean_rgb, count)
    out, out_count, ms = np.zeros_like(m), np.zeros(m.shape[:2], np.int32), C.c_float()
    prm = OpticsParams(k1, k2, ca, vignette)
    _check(L.pt_optics_host(device, m.shape[1], m.shape[0], _fp(m), _ip(c), C.byref(prm), _fp(out), _ip(out_count), C.byref(ms)), L)
    return (out, out_count, ms.value) if want_ms else (out, out_count)


def meter(mean_rgb, count, device=0, want_ms=False, library=None):
    """pt_meter_host: the meter kernel alone on a host image -- the 129 counts of the luminance histogram (uint32; [128] = dark),
    and the kernel's milliseconds as a second value if want_ms."""
    L = library or lib()
    m, c = _image_args("meter", mean_rgb, count)
    hist, ms = np.zeros(METER_ENTRIES, np.uint32), C.c_float()
    _check(L.pt_meter_host(device, m.shape[1], m.shape[0], _fp(m), _ip(c), hist.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(ms)), L)
    return (hist, ms.value) if want_ms else hist


def exposure_from_histogram(hist, grade=None, e_prev=None, library=None):
    """pt_exposure_from_histogram (host only): (e, e*) of a histogram under the metering rule of `grade` (None: the defaults);
    e_prev = the previous metered exposure, None on a first frame."""
    L = library or lib()
    h = np.ascontiguousarray(hist, np.uint32)
    if h.size != METER_ENTRIES:
        raise ValueError("exposure_from_histogram: the histogram has 129 counts")
    gp = _grade_params(grade) if grade is not None else GradeParams()
    e, t = C.c_float(), C.c_float()
    _check(L.pt_exposure_from_histogram(h.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(gp), 0 if e_prev is None else 1,
                                        C.c_float(0.0 if e_prev is None else e_prev), C.byref(e), C.byref(t)), L)
    return np.float32(e.value), np.float32(t.value)


def display_bytes_graded(mean_rgb, count, grade, gamma=None, e_prev=None, device=0, library=None):
    """pt_display_bytes_graded_host: meter (if automatic), exposure and the graded display kernel on a host image.  Returns
    (bgr uint8 [H, W, 3], info dict with the display's and the grade's fields)."""
    L = library or lib()
    if gamma is None:
        gamma = np.float32(1) / np.float32(2.2)
    m, c = _image_args("display_bytes_graded", mean_rgb, count)
    gp = _grade_params(grade)
    bgr = np.zeros(m.shape, np.uint8)
    info, ginfo = DisplayInfo(), GradeInfo()
    _check(L.pt_display_bytes_graded_host(device, m.shape[1], m.shape[0], _fp(m), _ip(c), C.c_float(gamma), C.byref(gp),
                                          0 if e_prev is None else 1, C.c_float(0.0 if e_prev is None else e_prev),
                                          bgr.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(info), C.byref(ginfo)), L)
    return bgr, dict(info.as_dict(), **ginfo.as_dict())


def colour_matrix(wb=None, saturation=None, matrix=None, library=None):
    """pt_colour_matrix (host only): M = U S W as float32 [3, 3] -- W = diag(wb), S the saturation about the meter's luminance,
    U the user matrix; None: the identity of that factor."""
    L = library or lib()
    prm = _colour_params({"wb": wb, "saturation": saturation, "matrix": matrix})
    out = np.zeros((3, 3), np.float32)
    _check(L.pt_colour_matrix(C.byref(prm), _fp(out)), L)
    return out


def colour(mean_rgb, count, exposure=1.0, curve=CURVE_REFERENCE, colour=None, library=None):
    """pt_colour_host (host only): LUT(curve((M mean) * exposure)) of the pixels with samples of mean_rgb [H, W, 3]; the others keep
    their value.  `colour`: None (pt_grade_host), a ColourParams, or a dict of its fields."""
    L = library or lib()
    m, c = _image_args("colour", mean_rgb, count)
    prm = _colour_params(colour) if colour is not None else ColourParams()
    out = np.zeros_like(m)
    _check(L.pt_colour_host(m.shape[1], m.shape[0], _fp(m), _ip(c), C.c_float(exposure), CURVES[curve] if isinstance(curve, str) else curve,
                            C.byref(prm), _fp(out)), L)
    return out


def display_bytes_colour(mean_rgb, count, grade, colour, gamma=None, e_prev=None, device=0, library=None):
    """pt_display_bytes_colour_host: meter (if automatic), exposure and the colour display kernel on a host image.  Returns
    (bgr uint8 [H, W, 3], info dict with the display's and the grade's fields)."""
    L = library or lib()
    if gamma is None:
        gamma = np.float32(1) / np.float32(2.2)
    m, c = _image_args("display_bytes_colour", mean_rgb, count)
    gp = _grade_params(grade) if grade is not None else GradeParams()
    prm = _colour_params(colour) if colour is not None else ColourParams()
    bgr = np.zeros(m.shape, np.uint8)
    info, ginfo = DisplayInfo(), GradeInfo()
    _check(L.pt_display_bytes_colour_host(device, m.shape[1], m.shape[0], _fp(m), _ip(c), C.c_float(gamma), C.byref(gp), C.byref(prm),
                                          0 if e_prev is None else 1, C.c_float(0.0 if e_prev is None else e_prev),
                                          bgr.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(info), C.byref(ginfo)), L)
    return bgr, dict(info.as_dict(), **ginfo.as_dict())


def grain_quantize(graded_rgb, count, gamma=None, grain=None, library=None):
    """pt_grain_quantize (host only): the bytes of a graded image graded_rgb [H, W, 3] (pt.colour's or pt.grade's output) with count
    [H, W] under film grain and dithered quantization -- the host chain's last step, in the place of tonemap -> quantize.  `grain`: None
    (their bytes), a GrainParams, or a dict of its fields.  Returns bgr uint8 [H, W, 3]."""
    L = library or lib()
    if gamma is None:
        gamma = np.float32(1) / np.float32(2.2)
    m, c = _image_args("grain_quantize", graded_rgb, count)
    prm = _grain_params(grain) if grain is not None else GrainParams()
    bgr = np.zeros(m.shape, np.uint8)
    _check(L.pt_grain_quantize(m.shape[1], m.shape[0], _fp(m), _ip(c), C.c_float(gamma), C.byref(prm), bgr.ctypes.data_as(C.POINTER(C.c_uint8))), L)
    return bgr


def display_bytes_grain(mean_rgb, count, grade, colour, grain, gamma=None, e_prev=None, device=0, library=None):
    """pt_display_bytes_grain_host: meter (if automatic), exposure and the grain display kernel on a host image.  Returns
    (bgr uint8 [H, W, 3], info dict with the display's and the grade's fields)."""
    L = library or lib()
    if gamma is None:
        gamma = np.float32(1) / np.float32(2.2)
    m, c = _image_args("display_bytes_grain", mean_rgb, count)
    gp = _grade_params(grade) if grade is not None else GradeParams()
    prm = _colour_params(colour) if colour is not None else ColourParams()
    np_ = _grain_params(grain) if grain is not None else GrainParams()
    bgr = np.zeros(m.shape, np.uint8)
    info, ginfo = DisplayInfo(), GradeInfo()
    _check(L.pt_display_bytes_grain_host(device, m.shape[1], m.shape[0], _fp(m), _ip(c), C.c_float(gamma), C.byref(gp), C.byref(prm), C.byref(np_),
                                         0 if e_prev is None else 1, C.c_float(0.0 if e_prev is None else e_prev),
                                         bgr.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(info), C.byref(ginfo)), L)
    return bgr, dict(info.as_dict(), **ginfo.as_dict())


def linear_encode(mean_rgb, count, exposure=1.0, format="pfm", exposed=False, library=None):
    """pt_linear_encode (host only): the body of a PFM ("pfm": 12 bytes per pixel, rows bottom-up) or of a flat Radiance picture ("hdr":
    4 bytes per pixel R, G, B, E) from the linear mean mean_rgb [H, W, 3] with count [H, W]; with `exposed` every channel is multiplied
    by `exposure` first.  Returns bytes."""
    L = library or lib()
    m, c = _image_args("linear_encode", mean_rgb, count)
    prm = _linear_params(None, format, exposed)
    out = np.zeros(12 * m.shape[0] * m.shape[1], np.uint8)
    _check(L.pt_linear_encode(m.shape[1], m.shape[0], _fp(m), _ip(c), C.c_float(exposure), C.byref(prm), out.ctypes.data_as(C.POINTER(C.c_uint8))), L)
    return out[:L.pt_linear_bytes(m.shape[1], m.shape[0], prm.format)].tobytes()


def linear_encode_device(device, mean_rgb, count, exposure=1.0, format="pfm", exposed=False, want_info=False, library=None):
    """pt_linear_encode_device_host: the encode kernel alone on a host image; the bytes are pt.linear_encode's.  Returns bytes (and the
    info dict with `want_info`)."""
    L = library or lib()
    m, c = _image_args("linear_encode_device", mean_rgb, count)
    prm = _linear_params(None, format, exposed)
    out = np.zeros(12 * m.shape[0] * m.shape[1], np.uint8)
    info = DisplayInfo()
    _check(L.pt_linear_encode_device_host(device, m.shape[1], m.shape[0], _fp(m), _ip(c), C.c_float(exposure), C.byref(prm),
                                          out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(info)), L)
    body = out[:L.pt_linear_bytes(m.shape[1], m.shape[0], prm.format)].tobytes()
    return (body, info.as_dict()) if want_info else body


def _write_linear(name, path, width, height, body, format, library):
    L = library or lib()
    b = np.frombuffer(bytes(body), np.uint8)
    if b.size != L.pt_linear_bytes(width, height, format):
        raise ValueError(f"{name}: the body does not hold width x height pixels")
    _check(getattr(L, name)(os.fsencode(path), width, height, b.ctypes.data_as(C.POINTER(C.c_uint8))), L)


def write_pfm(path, width, height, body, library=None):
    """pt_write_pfm: "PF", the size and the scale -1.0 (little-endian), then the body pt.linear_encode(format="pfm") made."""
    _write_linear("pt_write_pfm", path, width, height, body, LINEAR_PFM, library)


def write_hdr(path, width, height, body, library=None):
    """pt_write_hdr: the header of a flat Radiance picture, then the body pt.linear_encode(format="hdr") made."""
    _write_linear("pt_write_hdr", path, width, height, body, LINEAR_RGBE, library)


def display_table(gamma, library=None):
    """pt_display_table (host only): dict of thresholds [K] (T_k at [k - 1]: the smallest float the host's tone map puts at level k
    or above), doubt_lo / doubt_hi [K] (the doubt band of level k, empty where lo == hi)."""
    L = library or lib()
    k = C.c_int32()
    _check(L.pt_display_table(C.c_float(gamma), C.byref(k), None, None, None), L)
    out = {"thresholds": np.zeros(k.value, np.float32), "doubt_lo": np.zeros(k.value, np.float32), "doubt_hi": np.zeros(k.value, np.float32)}
    _check(L.pt_display_table(C.c_float(gamma), C.byref(k), _fp(out["thresholds"]), _fp(out["doubt_lo"]), _fp(out["doubt_hi"])), L)
    return out


def bvh_depth(nodes):
    """Levels of a box tree from its 64-byte nodes (BvhNode::meta: children - 1 in bits 8-10, leaf flag bit 11, base in bits
    12-31; children are consecutive nodes with larger indices): root = 1, no tree = 0."""
    n = len(nodes)
    if n == 0:
        return 0
    meta = np.ascontiguousarray(nodes).view(np.uint32).reshape(n, 16)[:, 3]
    level = np.ones(n, np.int64)
    for w in range(n):
        m = int(meta[w])
        if not (m >> 11) & 1:
            base, k = m >> 12, ((m >> 8) & 7) + 1
            level[base:base + k] = level[w] + 1
    return int(level.max())


class Frame(_EnvironmentMethods, _DielectricMethods, _TextureMethods, _SmoothMethods, _RoughMethods, _DirectMethods, _EnvDirectMethods, _RouletteMethods):
    """pt_frame: one image on several devices from one host program -- row bands, one gather to the first device."""
    _env_prefix = _glass_prefix = _tex_prefix = _smooth_prefix = _rough_prefix = _direct_prefix = _envdirect_prefix = _roulette_prefix = "pt_frame_"

    def _n_tri(self):
        return self._scene.counts()[0]

    def map_kd(self):
        return self._scene.map_kd()

    def __init__(self, scene, devices, width, height, flags=0):
        self._scene, self._L = scene, scene._L
        self.width, self.height = width, height
        devs = np.ascontiguousarray(devices, np.int32)
        self._h = C.c_void_p()
        _check(self._L.pt_frame_create(scene._h, _ip(devs), len(devs), width, height, flags, C.byref(self._h)), self._L)

    def info(self):
        n = C.c_int32()
        _check(self._L.pt_frame_info(self._h, C.byref(n), None, None, None), self._L)
        rows, dev, tr = np.zeros(2 * n.value, np.int32), np.zeros(n.value, np.int32), C.c_int32()
        _check(self._L.pt_frame_info(self._h, C.byref(n), _ip(rows), _ip(dev), C.byref(tr)), self._L)
        stride = C.c_int32()
        _check(self._L.pt_frame_row_stride(self._h, C.byref(stride)), self._L)
        return {"bands": n.value, "rows": rows.reshape(-1, 2).tolist(), "devices": dev.tolist(), "transport": TRANSPORT_NAMES[tr.value],
                "row_stride": stride.value}

    def render(self, pass_begin, pass_count, mrr, *, eps=1e-4, error=-1.0, seed=42, want_stats=False):
        p = RenderParams(self.width, self.height, 0, self.height, pass_begin, pass_count, mrr, eps, error, seed, 0)
        st = RenderStats()
        _check(self._L.pt_frame_render(self._h, C.byref(p), C.byref(st) if want_stats else None), self._L)
        return st.as_dict() if want_stats else None

    def set_camera(self, camera):
        """pt_frame_set_camera: the camera of every device's copy of the frame's scene (None = the reference's)."""
        if camera is not None and not isinstance(camera, Camera):
            camera = Camera.of(*camera)
        _check(self._L.pt_frame_set_camera(self._h, C.byref(camera) if camera is not None else None), self._L)

    def set_lens(self, radius, focus_distance=None):
        """pt_frame_set_lens: the lens of every device's copy of the frame's scene (None = a pinhole)."""
        _check(self._L.pt_frame_set_lens(self._h, _lens_arg(radius, focus_distance)), self._L)

    def set_camera_motion(self, end_camera):
        """pt_frame_set_camera_motion: the end pose of every device's copy of the frame's scene (None = no motion)."""
        if end_camera is not None and not isinstance(end_camera, Camera):
            end_camera = Camera.of(*end_camera)
        _check(self._L.pt_frame_set_camera_motion(self._h, C.byref(end_camera) if end_camera is not None else None), self._L)

    def set_projection(self, projection_):
        """pt_frame_set_projection: the projection of every device's copy of the frame's scene (None = the pinhole)."""
        _check(self._L.pt_frame_set_projection(self._h, _projection_arg(projection_, self._L)), self._L)

    def band_kernel_ms(self):
        """Kernel time of every band of the last render(want_stats=True), -1 where there is none."""
        ms = np.zeros(self.info()["bands"], np.float32)
        _check(self._L.pt_frame_band_kernel_ms(self._h, _fp(ms)), self._L)
        return ms.tolist()

    def gather(self):
        _check(self._L.pt_frame_gather(self._h), self._L)

    def wait(self):
        _check(self._L.pt_frame_wait(self._h), self._L)

    def read(self):
        n = self.width * self.height
        s, s2, c = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        _check(self._L.pt_frame_read(self._h, _fp(s), _fp(s2), _ip(c)), self._L)
        return s, s2, c

    def clear(self):
        _check(self._L.pt_frame_clear(self._h), self._L)

    def close(self):
        if self._h:
            self._L.pt_frame_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rccl_version(library=None):
    """ncclGetVersion of the RCCL the frame's gather would use; raises PtError if it cannot be loaded.  Needs no GPU."""
    L = library or lib()
    v = C.c_int32()
    _check(L.pt_rccl_available(C.byref(v)), L)
    return v.value


def resolve(width, height, s, s2, c, gamma=None):
    """main.cpp:162-201: returns (bgr uint8 [H,W,3], dispersion float32[3] = max, min, average)."""
    if gamma is None:
        gamma = np.float32(1) / np.float32(2.2)   # config.h:25
    bgr = np.zeros((height, width, 3), np.uint8)
    disp = np.zeros(3, np.float32)
    s = np.ascontiguousarray(s, np.float32)
    s2 = np.ascontiguousarray(s2, np.float32)
    c = np.ascontiguousarray(c, np.int32)
    _check(lib().pt_resolve(width, height, _fp(s), _fp(s2), _ip(c), C.c_float(gamma),
                            bgr.ctypes.data_as(C.POINTER(C.c_uint8)), _fp(disp)))
    return bgr, disp


def resolve_float(width, height, s, s2, c, gamma=None):
    """main.cpp:162-185: (rgb float32 [H,W,3] tonemapped image, dispersion float32[3])."""
    if gamma is None:
        gamma = np.float32(1) / np.float32(2.2)
    rgb = np.zeros((height, width, 3), np.float32)
    disp = np.zeros(3, np.float32)
    _check(lib().pt_resolve_float(width, height, _fp(np.ascontiguousarray(s, np.float32)), _fp(np.ascontiguousarray(s2, np.float32)),
                                  _ip(np.ascontiguousarray(c, np.int32)), C.c_float(gamma), _fp(rgb), _fp(disp)))
    return rgb, disp


def denoise(width, height, s, s2, c, features=None, *, levels=5, sigma_luminance=0.0, sigma_plane=0.0, normal_power_log2=0,
            demodulate_albedo=0, device=0, want_ms=False):
    """pt_denoise_host: the feature-guided a-trous filter on the linear mean of a whole frame's accumulators.  `features` is what
    Scene.render_features returns (not needed for levels = 0).  Returns (mean_rgb float32 [H * W, 3], count_out int32 [H * W]) -- the
    count to tone-map and quantize with --, and the kernel chain's milliseconds as a third value if want_ms."""
    n = width * height
    s, s2 = np.ascontiguousarray(s, np.float32), np.ascontiguousarray(s2, np.float32)
    c = np.ascontiguousarray(c, np.int32)
    if s.size != 3 * n or s2.size != 3 * n or c.size != n:
        raise ValueError("denoise: the accumulators do not hold width x height pixels")
    f = {}
    for k, dt, m in (("position", np.float32, 3), ("normal", np.float32, 3), ("albedo", np.float32, 3), ("hit_index", np.int32, 1)):
        f[k] = None if features is None else np.ascontiguousarray(features[k], dt)
        if f[k] is not None and f[k].size != m * n:
            raise ValueError(f"denoise: features[{k!r}] does not hold width x height pixels")
    ptr = lambda a, fn: fn(a) if a is not None else None
    prm = DenoiseParams(levels, sigma_luminance, sigma_plane, normal_power_log2, demodulate_albedo)
    mean, cout, ms = np.zeros((n, 3), np.float32), np.zeros(n, np.int32), C.c_float()
    _check(lib().pt_denoise_host(device, width, height, _fp(s), _fp(s2), _ip(c), ptr(f["position"], _fp), ptr(f["normal"], _fp),
                                 ptr(f["albedo"], _fp), ptr(f["hit_index"], _ip), C.byref(prm), _fp(mean), _ip(cout), C.byref(ms)))
    return (mean, cout, ms.value) if want_ms else (mean, cout)


def upsample(device, width, height, mean_lo, count_lo, features, scale=2, *, sigma_plane=0.0, normal_power_log2=0, demodulate_albedo=0,
             want_ms=False):
    """pt_upsample_host: a frame traced at (width / scale) x (height / scale) reconstructed at width x height, guided by the
    full-resolution `features` (what Scene.render_features returns for width x height).  mean_lo [h * w, 3], count_lo [h * w]: what
    pt.denoise returns for the low frame.  Returns (mean_rgb float32 [H * W, 3], count_out int32 [H * W]) -- the count to tone-map and
    quantize with --, and the kernel chain's milliseconds as a third value if want_ms."""
    n = width * height
    n_lo = n // (scale * scale) if scale > 0 else 0
    m = np.ascontiguousarray(mean_lo, np.float32)
    c = np.ascontiguousarray(count_lo, np.int32)
    if scale > 0 and width % scale == 0 and height % scale == 0 and (m.size != 3 * n_lo or c.size != n_lo):
        raise ValueError("upsample: mean_lo / count_lo do not hold (width / scale) x (height / scale) pixels")
    f = {}
    for k, dt, per in (("position", np.float32, 3), ("normal", np.float32, 3), ("albedo", np.float32, 3), ("hit_index", np.int32, 1)):
        f[k] = np.ascontiguousarray(features[k], dt)
        if f[k].size != per * n:
            raise ValueError(f"upsample: features[{k!r}] does not hold width x height pixels")
    prm = UpsampleParams(scale, sigma_plane, normal_power_log2, demodulate_albedo)
    mean, cout, ms = np.zeros((max(n, 0), 3), np.float32), np.zeros(max(n, 0), np.int32), C.c_float()
    _check(lib().pt_upsample_host(device, width, height, _fp(m), _ip(c), _fp(f["position"]), _fp(f["normal"]), _fp(f["albedo"]),
                                  _ip(f["hit_index"]), C.byref(prm), _fp(mean), _ip(cout), C.byref(ms)))
    return (mean, cout, ms.value) if want_ms else (mean, cout)


def tonemap(width, height, mean_rgb, c, gamma=None):
    """pt_tonemap (main.cpp:179-182): rgb float32 [H, W, 3] = pow(mean, gamma) * 255 where c != 0, the mean's own value elsewhere."""
    if gamma is None:
        gamma = np.float32(1) / np.float32(2.2)
    m, c = np.ascontiguousarray(mean_rgb, np.float32), np.ascontiguousarray(c, np.int32)
    if m.size != 3 * width * height or c.size != width * height:
        raise ValueError("tonemap: the buffers do not hold width x height pixels")
    rgb = np.zeros((height, width, 3), np.float32)
    _check(lib().pt_tonemap(width, height, _fp(m), _ip(c), C.c_float(gamma), _fp(rgb)))
    return rgb


def post_filter(rgb, gauss=0, median=0, device=0):
    """-GAUSS / -MEDIAN (main.cpp:187-192) on the GPU; returns the filtered float image."""
    out = np.ascontiguousarray(rgb, np.float32).copy()
    h, w, _ = out.shape
    _check(lib().pt_post_filter_host(device, w, h, _fp(out), gauss, median))
    return out


def quantize(rgb, c):
    h, w, _ = rgb.shape
    bgr = np.zeros((h, w, 3), np.uint8)
    _check(lib().pt_quantize(w, h, _fp(np.ascontiguousarray(rgb, np.float32)), _ip(np.ascontiguousarray(c, np.int32)),
                             bgr.ctypes.data_as(C.POINTER(C.c_uint8))))
    return bgr


def write_bmp(path, bgr):
    h, w, _ = bgr.shape
    bgr = np.ascontiguousarray(bgr, np.uint8)
    _check(lib().pt_write_bmp(path.encode(), w, h, bgr.ctypes.data_as(C.POINTER(C.c_uint8))))
