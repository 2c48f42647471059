"""CPU checks of the camera projections (pt_hip.h: pt_projection): the host composition against view_composition's, exact properties
of the restated rays, the handle's projection and every refusal, clones, the helpers pt_projection_make and pt_camera_ortho to the
last bit, and pt_render's projection flags as far as they run without a device."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import projection_composition as P
import view_composition as V

pt = importlib.import_module("path-tracing_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_RENDER = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
KU = 2.0 ** -24
F32 = np.float32
TWO_PI = 2.0 * np.pi


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _all_pixels(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs.ravel(), ys.ravel()], 1)


def _same(a, b):
    return all(np.array_equal(_bits(x) if x.dtype == np.float32 else x, _bits(y) if y.dtype == np.float32 else y) for x, y in zip(a, b))


# ---- 1. with kind perspective the composition is view_composition's ----------------------------------------------------------
@pytest.mark.parametrize("mrr", [1, 3, 8])
@pytest.mark.parametrize("err", [-1.0, 0.02])
def test_the_perspective_composition_is_the_view_composition(oracle_scene, mrr, err):
    W, H, spp = 20, 12, 14   # (passes > 10: the adaptive skip has something to do at -ERR 0.02)
    cam = pt.look_at((2, -3, -19), (0, 1, 0), fov_y=65.0, aspect=W / H).as_array()   # (the emitter is in view: -MRR 1 sees it or nothing)
    px = _all_pixels(W, H)
    want = V.compose(oracle_scene, W, H, px, spp, mrr, camera=cam, error=err, seed=7)
    got = P.compose(oracle_scene, W, H, px, spp, mrr, camera=cam, projection=(P.PERSPECTIVE, 0.0, 0.0), error=err, seed=7)
    assert want[2].sum() > 0
    assert _same(got, want)


def test_the_perspective_composition_under_a_skybox_is_the_view_composition(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_open_scene as MO
    d = str(tmp_path) + "/"
    MO.generate(os.path.join(ROOT, "models"), d, name="Open.obj")
    sc = O.Scene.load(d, "Open.obj")
    sc.set_skybox(d + "sky.bmp")
    W, H, spp = 20, 12, 6
    px = _all_pixels(W, H)
    for mrr in (1, 3, 8):
        want = V.compose(sc, W, H, px, spp, mrr)
        got = P.compose(sc, W, H, px, spp, mrr)
        assert _same(got, want), mrr


# ---- 2. exact properties of the restatement ------------------------------------------------------------------------------------
def _words(n, seed=3):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2 ** 32, size=(n, 4), dtype=np.uint64).astype(np.uint32)


def test_ortho_directions_are_all_identical():
    cam = pt.ortho_camera((6, 3, -15), (0, 0, 0), view_height=12.0, aspect=1.5).as_array()
    rng = np.random.default_rng(1)
    x, y = rng.integers(0, 300, 400), rng.integers(0, 200, 400)
    o, d = P.primary_rays(x, y, 300, 200, _words(400), cam, (P.ORTHOGRAPHIC, 0.0, 0.0))
    assert (_bits(d) == _bits(d[0])).all()
    assert _bits(d[0]).tolist() == _bits(V.normalize3(cam[3][None, :])[0]).tolist()
    assert len(np.unique(_bits(o), axis=0)) == 400        # and the origins differ


def test_the_fisheye_centre_looks_along_forward_and_its_radius_is_the_angle():
    cam = pt.look_at((6, 3, -15), (0, 0, 0), fov_y=45.0).as_array()
    fh = V.lens_axes(cam)[2]
    prj = (P.FISHEYE, F32(np.pi), F32(np.pi))
    _, d = P.rays_from_uv(np.zeros(1, F32), np.zeros(1, F32), cam, prj)         # theta == 0: k = 1, no division
    assert np.isfinite(d).all() and np.abs(d[0] - fh).max() < 2e-7
    u = np.linspace(-0.5, 0.5, 41).astype(F32)
    _, d = P.rays_from_uv(u, np.zeros_like(u), cam, prj)
    d64, f64 = d.astype(np.float64), fh.astype(np.float64)
    ang = np.arctan2(np.linalg.norm(np.cross(d64, f64), axis=1), d64 @ f64)       # (well conditioned at every angle, unlike arccos)
    # equidistant, to the rounding of a float direction: a few ulps of 2^-24 per component of d and of f^
    assert np.abs(ang - np.abs(u.astype(np.float64) * float(F32(np.pi)))).max() < 1e-6


def test_the_full_sphere_stays_within_the_sincos_domain():
    prj = pt.projection("equirect")
    assert prj.kind == pt.PROJECTION_EQUIRECTANGULAR
    for uv in (F32(0.5), F32(-0.5)):
        assert abs(uv * F32(prj.span_x)) <= F32(TWO_PI) and abs(uv * F32(prj.span_y)) <= F32(TWO_PI)
    # at u = +-0.5 the view looks backwards, at v = +-0.5 straight up and down
    cam = V.REFERENCE_CAMERA
    _, d = P.rays_from_uv(np.array([0.5, -0.5, 0, 0, 0], F32), np.array([0, 0, 0.5, -0.5, 0], F32), cam, (3, prj.span_x, prj.span_y))
    want = np.array([[0, 0, -1], [0, 0, -1], [0, 1, 0], [0, -1, 0], [0, 0, 1]], np.float64)
    assert np.abs(d - want).max() < 1e-6


# ---- 3. the interface ------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def tor(models_dir):
    s = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    yield s
    s.close()


def test_symbols_and_struct_size():
    L = pt.lib()
    for name in ("pt_projection_make", "pt_camera_ortho", "pt_scene_set_projection", "pt_scene_get_projection", "pt_frame_set_projection"):
        getattr(L, name)
    assert C.sizeof(pt.Projection) == 12
    header = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    for k, name in enumerate(("PERSPECTIVE", "ORTHOGRAPHIC", "FISHEYE", "EQUIRECTANGULAR")):
        assert f"#define PT_PROJECTION_{name}" in header and getattr(pt, "PROJECTION_" + name) == k
    assert "#define PT_ABI_VERSION 5" in header


def test_projection_round_trips_and_resets(tor):
    assert tor.get_projection() is None
    fish = pt.projection("fisheye", fov_y=180.0, aspect=1.5)
    tor.set_projection(fish)
    assert tor.get_projection() == fish
    tor.set_projection("ortho")
    assert tor.get_projection() == pt.Projection(pt.PROJECTION_ORTHOGRAPHIC, 0.0, 0.0)
    tor.set_projection(pt.Projection(pt.PROJECTION_ORTHOGRAPHIC, 7.0, float("nan")))      # kinds 0 and 1 ignore the spans
    assert tor.get_projection() == pt.Projection(pt.PROJECTION_ORTHOGRAPHIC, 0.0, 0.0)
    tor.set_projection("equirect")
    assert tor.get_projection() == pt.Projection(3, np.float32(TWO_PI), np.float32(np.pi))
    tor.set_projection(None)
    assert tor.get_projection() is None


def test_kind_perspective_leaves_the_handle_as_never_set(tor):
    tor.set_projection(pt.Projection(pt.PROJECTION_PERSPECTIVE, 1.0, 2.0))
    assert tor.get_projection() is None
    tor.set_lens(0.5, 16.0)                      # what a handle without a projection accepts
    tor.set_camera_motion(pt.look_at((1, 0, -20), (0, 0, 0)))
    tor.set_projection("perspective")            # and a lens and a motion do not object to it
    assert tor.get_projection() is None and tor.lens() == pt.Lens(0.5, 16.0) and tor.get_camera_motion() is not None


def test_clones_inherit_the_projection_of_the_handle_they_are_made_from(tor):
    fish = pt.projection("fisheye", fov_y=200.0)
    tor.set_projection(fish)
    c1 = tor.clone_to_device(-1)
    assert c1.get_projection() == fish
    c1.set_projection(None)                       # a copy's projection is its own
    assert tor.get_projection() == fish and c1.get_projection() is None
    tor.set_projection(None)
    c2 = tor.clone_to_device(-1)
    assert c2.get_projection() is None
    c1.close()
    c2.close()


# ---- 4. the refusals ---------------------------------------------------------------------------------------------------------------
def _refused(call, status):
    with pytest.raises(pt.PtError) as e:
        call()
    assert e.value.status == status, e.value


@pytest.mark.parametrize("bad", [
    pt.Projection(4, 1.0, 1.0), pt.Projection(-1, 1.0, 1.0),                                         # unknown kinds
    pt.Projection(2, float("nan"), 1.0), pt.Projection(2, 1.0, float("inf")), pt.Projection(2, 0.0, 1.0), pt.Projection(2, 1.0, -1.0),
    pt.Projection(3, float("inf"), 1.0), pt.Projection(3, 1.0, float("nan")), pt.Projection(3, -2.0, 1.0), pt.Projection(3, 1.0, 0.0),
    pt.Projection(2, 9.0, 9.0),                                                                      # corner angle 6.36 > 2 pi
    pt.Projection(3, 12.6, 1.0), pt.Projection(3, 1.0, 12.6),                                        # > 4 pi = 12.566
])
def test_bad_projections_are_refused_and_leave_the_handle_alone(tor, bad):
    keep = pt.projection("fisheye", fov_y=120.0)
    tor.set_projection(keep)
    _refused(lambda: tor.set_projection(bad), pt.PT_ERR_INVALID_ARGUMENT)
    assert tor.get_projection() == keep
    tor.set_projection(None)
    _refused(lambda: tor.set_projection(bad), pt.PT_ERR_INVALID_ARGUMENT)
    assert tor.get_projection() is None


def test_the_span_bounds_are_where_the_header_puts_them(tor):
    # fisheye: 0.5 sqrt(sx^2 + sy^2) <= 2 pi, in double, of the float spans
    s = np.float32(TWO_PI * np.sqrt(2.0))
    below = s if 0.5 * np.sqrt(2.0 * float(s) ** 2) <= TWO_PI else np.nextafter(s, np.float32(0))
    above = np.nextafter(below, np.float32(100))
    assert 0.5 * np.sqrt(2.0 * float(below) ** 2) <= TWO_PI < 0.5 * np.sqrt(2.0 * float(above) ** 2)
    tor.set_projection(pt.Projection(2, below, below))
    _refused(lambda: tor.set_projection(pt.Projection(2, above, above)), pt.PT_ERR_INVALID_ARGUMENT)
    # equirectangular: each span <= 4 pi
    s = np.float32(2 * TWO_PI)
    below = s if float(s) <= 2 * TWO_PI else np.nextafter(s, np.float32(0))
    above = np.nextafter(below, np.float32(100))
    tor.set_projection(pt.Projection(3, below, below))
    _refused(lambda: tor.set_projection(pt.Projection(3, above, 1.0)), pt.PT_ERR_INVALID_ARGUMENT)
    _refused(lambda: tor.set_projection(pt.Projection(3, 1.0, above)), pt.PT_ERR_INVALID_ARGUMENT)
    assert tor.get_projection() == pt.Projection(3, below, below)


@pytest.mark.parametrize("kind", ["ortho", "fisheye", "equirect"])
def test_a_projection_and_a_lens_or_a_motion_refuse_each_other_in_both_orders(tor, kind):
    prj = pt.projection(kind, fov_y=150.0)
    end = pt.look_at((1, 0, -20), (0, 0, 0))
    # the projection first
    tor.set_projection(prj)
    _refused(lambda: tor.set_lens(0.5, 16.0), pt.PT_ERR_UNSUPPORTED)
    _refused(lambda: tor.set_camera_motion(end), pt.PT_ERR_UNSUPPORTED)
    assert tor.lens() is None and tor.get_camera_motion() is None and tor.get_projection() == prj
    tor.set_lens(None)                            # clearing what is not there is no combination
    tor.set_lens(0.0, 5.0)
    tor.set_camera_motion(None)
    assert tor.get_projection() == prj
    # the lens first
    tor.set_projection(None)
    tor.set_lens(0.5, 16.0)
    _refused(lambda: tor.set_projection(prj), pt.PT_ERR_UNSUPPORTED)
    assert tor.get_projection() is None and tor.lens() == pt.Lens(0.5, 16.0)
    tor.set_lens(None)
    # the motion first
    tor.set_camera_motion(end)
    _refused(lambda: tor.set_projection(prj), pt.PT_ERR_UNSUPPORTED)
    assert tor.get_projection() is None and tor.get_camera_motion() == end
    tor.set_camera_motion(None)                   # "clear one first"
    tor.set_projection(prj)
    assert tor.get_projection() == prj


def _ortho_reach(cam):
    """max_i(|o_i| + 0.5 (|r_i| + |p_i|)) (1 + 2^-18), in double (pt_hip.h: pt_scene_set_projection)."""
    c = np.asarray(cam, np.float32).reshape(4, 3).astype(np.float64)
    return float((np.abs(c[0]) + 0.5 * (np.abs(c[1]) + np.abs(c[2]))).max() * (1.0 + 2.0 ** -18))


def _camera_at_the_bound():
    """An orthographic camera whose reach is the largest one <= PT_CAMERA_MAX_ORIGIN (4096), and its float neighbour beyond it."""
    right, up, fwd = (64.0, 0.0, 0.0), (0.0, 32.0, 0.0), (0.0, 0.0, 1.0)
    x = np.float32(4096.0 / (1.0 + 2.0 ** -18) - 32.0)
    while _ortho_reach(((x, 0, 0), right, up, fwd)) > 4096.0:
        x = np.nextafter(x, np.float32(0))
    while _ortho_reach(((np.nextafter(x, np.float32(1e9)), 0, 0), right, up, fwd)) <= 4096.0:
        x = np.nextafter(x, np.float32(1e9))
    inside = ((float(x), 0.0, 0.0), right, up, fwd)
    outside = ((float(np.nextafter(x, np.float32(1e9))), 0.0, 0.0), right, up, fwd)
    assert _ortho_reach(inside) <= 4096.0 < _ortho_reach(outside)
    return inside, outside


def test_the_orthographic_envelope_refusal_sits_exactly_at_the_bound_in_both_orders(tor):
    inside, outside = _camera_at_the_bound()
    assert tor.cull_tables()["constants"]["k2"] > 0       # (Tor.obj lies well within 4096: the bound is PT_CAMERA_MAX_ORIGIN)
    # the camera first, then the projection
    tor.set_camera(inside)
    tor.set_projection("ortho")
    tor.set_projection(None)
    tor.set_camera(outside)                               # a pinhole may stand there
    _refused(lambda: tor.set_projection("ortho"), pt.PT_ERR_UNSUPPORTED)
    assert tor.get_projection() is None
    tor.set_projection(pt.projection("fisheye", fov_y=90.0))   # rays that start at the eye do not mind
    # the projection first, then the camera
    tor.set_camera(inside)
    tor.set_projection("ortho")
    _refused(lambda: tor.set_camera(outside), pt.PT_ERR_UNSUPPORTED)
    assert tor.camera() == pt.Camera.of(*inside) and tor.get_projection().kind == pt.PROJECTION_ORTHOGRAPHIC
    wide = ((0, 0, -20), (9000.0, 0, 0), (0, 1, 0), (0, 0, 1))                  # the image plane itself reaches too far
    _refused(lambda: tor.set_camera(wide), pt.PT_ERR_UNSUPPORTED)
    assert tor.camera() == pt.Camera.of(*inside)


def _r_org(scene, eps=1e-4):
    """k2 = kU (24 sqrt(3) + 8) r_org (pt_cull_tables.cpp, margins of the barycentric test); r_org = the envelope radius + 1."""
    return scene.cull_tables(eps)["constants"]["k2"] / (KU * (24 * np.sqrt(3) + 8))


@pytest.mark.parametrize("eye,target,height", [((6, 3, -15), (0, 0, 0), 12.0), ((19.0, -19.0, 5.0), (0, 0, 0), 30.0),
                                               ((0, 0, -200), (3, 1, 0), 40.0), ((100, 50, -20), (0, 0, 0), 8.0)])
def test_every_ortho_origin_lies_within_the_envelope_the_library_reports(tor, eye, target, height):
    W, H = 64, 48
    cam = pt.ortho_camera(eye, target, view_height=height, aspect=W / H)
    tor.set_camera(cam)
    tor.set_projection("ortho")
    r_max = _r_org(tor) - 1.0
    extent = float(np.abs(tor.triangles()[0][:, 4:13]).max())                      # the scene's largest |vertex coordinate|
    assert r_max <= max(20.0, extent, _ortho_reach(cam.as_array())) * (1 + 1e-6)  # no looser than the stated term
    u = np.array([-0.5, 0.5, -0.5, 0.5, 0.0], F32)
    v = np.array([-0.5, -0.5, 0.5, 0.5, 0.0], F32)
    o, _ = P.rays_from_uv(u, v, cam.as_array(), (P.ORTHOGRAPHIC, 0, 0))
    assert np.abs(o).max() <= r_max, (np.abs(o).max(), r_max)
    # every pixel of a frame with its extreme jitter words: within the envelope's slack of one scene unit (r_org)
    px = _all_pixels(W, H)
    for w in (0, 0xFFFFFFFF):
        words = np.full((len(px), 4), w, np.uint32)
        o, _ = P.primary_rays(px[:, 0], px[:, 1], W, H, words, cam.as_array(), (P.ORTHOGRAPHIC, 0, 0))
        assert np.abs(o).max() <= r_max + 0.5, (np.abs(o).max(), r_max)


def _tables(scene, eps=1e-4):
    t = scene.cull_tables(eps)
    lay = scene.cull_layout(eps)
    return [t["cluster_sphere"], t["spheres"], t["bary"], np.array(list(t["constants"].values()), np.float32),
            lay["slot_triangle"], lay["bvh"]]


def test_views_inside_the_camera_free_envelope_share_the_camera_free_tables(models_dir):
    plain = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    want = _tables(plain)
    views = ((pt.ortho_camera((5, -7, 12), (0, 1, 3), view_height=6.0), "ortho"),
             (pt.look_at((5, -7, 12), (0, 1, 3), fov_y=70.0), pt.projection("fisheye", fov_y=200.0)),
             (None, "equirect"))
    for cam, prj in views:
        s = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
        if cam is not None:
            s.set_camera(cam)
        s.set_projection(prj)
        for a, b in zip(want, _tables(s)):
            assert a.shape == b.shape and a.tobytes() == b.tobytes()
        s.close()
    wide = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    wide.set_camera(pt.ortho_camera((0, 0, -20), (0, 0, 0), view_height=80.0))   # the image plane spans x and y up to 40
    wide.set_projection("ortho")
    assert 41.0 <= _r_org(wide) <= 41.0 * (1 + 1e-4)
    wide.close()
    plain.close()


# ---- 5. the helpers, to the last bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fov,aspect", [(180.0, 0.0), (180.0, 16 / 9), (53.13010235415598, 1.5), (220.0, 1.0), (1e-3, 3.0), (359.0, 0.5)])
def test_projection_make_equals_the_double_precision_restatement(fov, aspect):
    fov, aspect = np.float32(fov), np.float32(aspect)
    rad = float(fov) * (np.pi / 180.0)
    a = float(aspect) if aspect > 0 else 1.0
    for kind in (pt.PROJECTION_FISHEYE, pt.PROJECTION_EQUIRECTANGULAR):
        got = pt.projection(kind, fov_y=float(fov), aspect=float(aspect))
        assert got == pt.Projection(kind, np.float32(rad * a), np.float32(rad))
    assert pt.projection("equirect", fov_y=0.0, aspect=float(aspect)) == pt.Projection(3, np.float32(2.0 * np.pi), np.float32(np.pi))
    assert pt.projection("equirect", fov_y=-5.0) == pt.Projection(3, np.float32(2.0 * np.pi), np.float32(np.pi))
    assert pt.projection("ortho", fov_y=float(fov), aspect=2.0) == pt.Projection(1, 0.0, 0.0)
    assert pt.projection("perspective", fov_y=float(fov)) == pt.Projection(0, 0.0, 0.0)


def test_projection_make_refuses_what_it_cannot_make():
    for call in (lambda: pt.projection(7), lambda: pt.projection("fisheye", fov_y=0.0), lambda: pt.projection("fisheye", fov_y=-3.0),
                 lambda: pt.projection("fisheye", fov_y=float("nan")), lambda: pt.projection("equirect", fov_y=90.0, aspect=float("inf"))):
        _refused(call, pt.PT_ERR_INVALID_ARGUMENT)
    with pytest.raises(ValueError):
        pt.projection("panini")


@pytest.mark.parametrize("eye,target,up,height,aspect", [
    ((6, 3, -15), (0, 0, 0), (0, 1, 0), 12.0, 1.5), ((0, 0, -20), (0, 0, 0), (0, 1, 0), 1.0, 0.0),
    ((4.25, -3.5, -6.125), (-9.5, 9.5, 9.5), (0.1, 1.0, 0.0), 7.3, 16 / 9), ((1e3, 2e3, -3e3), (0.5, 0.25, 0.125), (0, 0, 1), 333.0, 0.75)])
def test_camera_ortho_equals_the_double_precision_restatement(eye, target, up, height, aspect):
    got = pt.ortho_camera(eye, target, up, view_height=height, aspect=aspect).as_array()
    e, t, u = (np.asarray(v, np.float32).astype(np.float64) for v in (eye, target, up))
    f = t - e
    f = f / np.sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2])
    r = np.array([u[1] * f[2] - u[2] * f[1], u[2] * f[0] - u[0] * f[2], u[0] * f[1] - u[1] * f[0]])
    r = r / np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    p = np.array([f[1] * r[2] - f[2] * r[1], f[2] * r[0] - f[0] * r[2], f[0] * r[1] - f[1] * r[0]])
    sy = float(np.float32(height))
    sx = sy * (float(np.float32(aspect)) if aspect > 0 else 1.0)
    want = np.stack([e, r * sx, p * sy, f]).astype(np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    assert abs(np.linalg.norm(got[1].astype(np.float64)) - sx) < 1e-6 * sx and abs(np.linalg.norm(got[2].astype(np.float64)) - sy) < 1e-6 * sy


def test_camera_ortho_refuses_bad_input():
    for call in (lambda: pt.ortho_camera((0, 0, 0), (0, 0, 0)), lambda: pt.ortho_camera((0, 0, -1), (0, 0, 0), view_height=0.0),
                 lambda: pt.ortho_camera((0, 0, -1), (0, 0, 0), view_height=-2.0), lambda: pt.ortho_camera((0, -1, 0), (0, 0, 0)),
                 lambda: pt.ortho_camera((0, 0, -1), (0, 0, float("nan")))):
        _refused(call, pt.PT_ERR_INVALID_ARGUMENT)


# ---- 6. pt_render ------------------------------------------------------------------------------------------------------------------
def _print_camera(*flags):
    env = dict(os.environ, PT_RENDER_PRINT_CAMERA="1")
    return subprocess.run([PT_RENDER, *flags], env=env, capture_output=True, text=True, timeout=60)


def test_pt_render_prints_the_projection_its_flags_resolve_to():
    assert _print_camera("-PROJECTION", "perspective").stdout == "camera none\n"
    out = _print_camera("-PROJECTION", "equirect")
    assert out.returncode == 0 and out.stdout == "camera none\nprojection 3 %.9g %.9g\n" % (np.float32(2 * np.pi), np.float32(np.pi))
    out = _print_camera("-PROJECTION", "fisheye", "-FOV", "220", "-ASPECT", "1.5").stdout.splitlines()
    want = pt.projection("fisheye", fov_y=220.0, aspect=1.5)
    assert out[-1] == "projection 2 %.9g %.9g" % (want.span_x, want.span_y)
    assert out[0] == "origin 0 0 -20" and out[3] == "forward 0 0 1"                 # the axes of the default view
    # ortho: the height the perspective view has at the look-at distance (20 for the reference's: 2 tan(fov / 2) 20 = 20)
    out = _print_camera("-PROJECTION", "ortho").stdout.splitlines()
    assert out == ["origin 0 0 -20", "right 20 0 0", "up 0 20 0", "forward 0 0 1", "projection 1 0 0"]
    out = _print_camera("-PROJECTION", "ortho", "-ORTHO_HEIGHT", "8", "-ASPECT", "1.5", "-EYE", "6,3,-15").stdout.splitlines()
    want = pt.ortho_camera((6, 3, -15), (0, 0, 0), view_height=8.0, aspect=1.5).as_array()
    got = np.array([[np.float32(t) for t in line.split()[1:]] for line in out[:4]], np.float32)
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("bad", [["-PROJECTION", "panini"], ["-PROJECTION", ""], ["-PROJECTION", "Ortho"],
                                 ["-PROJECTION", "ortho", "-ORTHO_HEIGHT", "0"], ["-PROJECTION", "ortho", "-ORTHO_HEIGHT", "abc"],
                                 ["-PROJECTION", "fisheye", "-ORTHO_HEIGHT", "5"], ["-PROJECTION", "fisheye", "-FOV", "0"]])
def test_pt_render_refuses_malformed_projection_flags(bad):
    out = _print_camera(*bad)
    assert out.returncode != 0 and out.stderr.strip() != "" and out.stdout == ""


@pytest.mark.parametrize("kind", ["ortho", "fisheye", "equirect"])
@pytest.mark.parametrize("extra,word", [(["-APERTURE", "0.5"], "lens"), (["-SHUTTER", "0.5", "-EYE_END", "1,0,-20"], "camera motion"),
                                        (["-SHUTTER", "0.5", "-EYE_END", "1,0,-20", "-FRAMES", "2"], "camera motion"),
                                        (["-TEMPORAL", "8"], "temporal")])
def test_pt_render_refuses_a_projection_with_a_lens_a_shutter_or_a_history(models_dir, tmp_path, kind, extra, word):
    """The refusal is the library's (its message names what the projection does not go with) and comes before any device is looked at."""
    out = subprocess.run([PT_RENDER, "--W", "16", "--H", "16", "-RPP", "1", "-MODEL_PATH", models_dir, "-QUIET", "1", "-PROJECTION", kind,
                          "-OUT", os.path.join(str(tmp_path), "never.bmp")] + extra, capture_output=True, text=True, timeout=60)
    assert out.returncode != 0
    assert word in out.stderr and "non-perspective projection" in out.stderr, out.stderr
    assert "no HIP device" not in out.stderr
    assert not os.path.exists(os.path.join(str(tmp_path), "never.bmp"))


def test_pt_render_projection_flags_leave_the_config_printout_alone():
    env = dict(os.environ, PT_RENDER_PRINT_CONFIG="1")
    a = subprocess.run([PT_RENDER, "-MRR", "3"], env=env, capture_output=True, text=True, timeout=60)
    b = subprocess.run([PT_RENDER, "-MRR", "3", "-PROJECTION", "fisheye", "-FOV", "180"], env=env, capture_output=True, text=True, timeout=60)
    assert a.returncode == b.returncode == 0 and a.stdout == b.stdout
