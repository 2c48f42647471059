"""Dielectric materials on the GPU (pt_hip.h: pt_dielectric; pt_kernels.hip: integrate_kernel_glass), bit for bit against
tests/glass_composition.py: environment_composition's frame with the restated dielectric step (tests/glass_restatement.py).
Tor.obj with each non-emissive material as glass and two at once; a closed room made with pt_scene_create that holds a closed glass
box (entering, leaving, chains of total internal reflection), and a single pane between eye and emitter; indices 1, 1.5, 8 and 0.5,
tints with a zero channel and all zero; every view, every miss shader, statistics (the counters too), adaptive sampling, a late pass
window, the box tree, bands, frames, a clone, both verification builds, and a list set and cleared."""
import importlib
import os
import sys

import numpy as np
import pytest

import glass_composition as GC
import oracle_lib as O
from glass_fuzz_scenes import _box, _quad, _room, _write_obj

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SHAPES = [(32, 16), (24, 20), (17, 9)]      # whole 16 x 8 tiles; partial tiles in both directions


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def gpu():
    assert pt.device_count() >= 1, "no HIP device: the integrator has no CPU fallback"


def _all_pixels(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.ravel(), ys.ravel()], 1)


def _entries(glass):
    return [pt.dielectric(m, ior, tint) for m, (ior, tint) in glass.items()]


def _check(scene, osc, glass, w, h, spp, mrr, *, env=None, px=None, error=-1.0, stats=False, pass_begin=0, seed=42, **view):
    """Renders the frame and compares the pixels `px` (default: all) with the composition; with stats the counters as well."""
    px = _all_pixels(w, h) if px is None else px
    s, s2, c, st = scene.render_host(w, h, spp, mrr, error=error, seed=seed, want_stats=stats, pass_begin=pass_begin)
    i = px[:, 1] * w + px[:, 0]
    tally = {}
    ws, ws2, wc = GC.compose(osc, glass, env, w, h, px, spp, mrr, seed=seed, error=error, pass_begin=pass_begin, stats=tally, **view)
    assert np.array_equal(c[i], wc), int((c[i] != wc).sum())
    assert np.array_equal(_bits(s.reshape(-1, 3)[i]), _bits(ws)) and np.array_equal(_bits(s2.reshape(-1, 3)[i]), _bits(ws2))
    if stats:
        assert len(px) == w * h
        assert (st["samples_traced"], st["segments"], st["misses"], st["contributing"]) == \
               (tally["samples_traced"], tally["segments"], tally["misses"], tally["contributing"]), (st, tally)
    return s, s2, c, st


# ---- scenes --------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def glass_box(tmp_path_factory):
    """The room with a closed box of material 2 in it, a smaller box of material 3 beside it; made with pt_scene_create from the
    triangles and materials the oracle parsed, so both sides hold the same records."""
    d = str(tmp_path_factory.mktemp("glassbox")) + "/"
    _write_obj(d, "box.obj", _room() + _box((-2.5, -2.0, -8.0), (1.5, 2.0, -4.0), 2) + _box((2.5, -5.0, -7.0), (4.5, -3.0, -5.0), 3))
    osc = O.Scene.load(d, "box.obj")
    tri, tri_mat = osc.triangles()
    return pt.Scene.create(tri, tri_mat, osc.materials(), device=0), osc


@pytest.fixture(scope="module")
def pane(tmp_path_factory):
    """The room with one pane of material 2 from wall to wall, between the eye and everything else, the emitter behind it."""
    d = str(tmp_path_factory.mktemp("pane")) + "/"
    _write_obj(d, "pane.obj", _room() + _quad((-6.0, -6.0, -14.0), (6.0, -6.0, -14.0), (6.0, 6.0, -14.0), (-6.0, 6.0, -14.0), 2))
    return pt.Scene.load_obj(d, "pane.obj", device=0), O.Scene.load(d, "pane.obj")


@pytest.fixture(scope="module")
def tor(models_dir):
    return pt.Scene.load_obj(models_dir, "Tor.obj", device=0), O.Scene.load(models_dir, "Tor.obj")


@pytest.fixture(scope="module")
def open_tor(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_open_scene as MO
    d = str(tmp_path_factory.mktemp("open")) + "/"
    MO.generate(os.path.join(ROOT, "models"), d, name="Open.obj")
    return d, pt.Scene.load_obj(d, "Open.obj", device=0), O.Scene.load(d, "Open.obj")


def _reset(scene):
    scene.set_projection(None); scene.set_camera_motion(None); scene.set_lens(None); scene.set_camera(None)
    scene.set_environment(None); scene.set_skybox(None); scene.set_dielectrics(None)


# ---- 1. Tor.obj: each material, two at once --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("glass", [{1: (1.5, (1, 1, 1))}, {2: (1.33, (1, 1, 1))}, {3: (1.5, (0.9, 0.5, 1.0))}, {4: (1.5, (1, 1, 1))},
                                   {4: (1.5, (0.9, 1.0, 0.9)), 2: (1.33, (1.0, 0.8, 0.6))}], ids=["m1", "m2", "m3", "m4", "m4_m2"])
def test_tor_with_each_material_as_glass(gpu, tor, glass, shape):
    scene, osc = tor
    _reset(scene)
    scene.set_dielectrics(_entries(glass))
    w, h = shape
    _check(scene, osc, glass, w, h, 4, 8)


@pytest.mark.parametrize("mrr", [1, 2, 4, 8])
def test_every_path_length(gpu, tor, mrr):
    scene, osc = tor
    _reset(scene)
    glass = {4: (1.5, (0.9, 1.0, 0.9)), 1: (1.5, (1, 1, 1))}
    scene.set_dielectrics(_entries(glass))
    s, _, c, _ = _check(scene, osc, glass, 24, 20, 6, mrr)
    assert mrr == 1 or c.sum() > 0


# ---- 2. the box and the pane: indices and tints ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ior", [1.0, 1.5, 8.0, 0.5])
@pytest.mark.parametrize("tint", [(1.0, 1.0, 1.0), (0.8, 0.0, 0.9), (0.0, 0.0, 0.0)], ids=["clear", "zero_channel", "black"])
def test_a_closed_glass_box_in_a_closed_room(gpu, glass_box, ior, tint):
    scene, osc = glass_box
    _reset(scene)
    glass = {2: (ior, tint), 3: (1.5, (1.0, 0.9, 0.8))}
    scene.set_dielectrics(_entries(glass))
    s, _, c, st = _check(scene, osc, glass, 24, 20, 5, 8, stats=True)
    assert c.sum() > 0 and st["misses"] == 0          # the room is closed
    if tint == (0.0, 0.0, 0.0) and ior != 0.5:          # a path that enters the black box dies there: fewer contributions than through clear glass
        clear = dict(glass)
        clear[2] = (ior, (1.0, 1.0, 1.0))
        scene.set_dielectrics(_entries(clear))
        assert scene.render_host(24, 20, 5, 8, want_stats=False)[2].sum() > c.sum()


@pytest.mark.parametrize("ior", [1.0, 1.5, 8.0, 0.5])
def test_a_pane_between_eye_and_emitter(gpu, pane, ior):
    scene, osc = pane
    _reset(scene)
    glass = {2: (ior, (0.7, 1.0, 0.0))}
    scene.set_dielectrics(_entries(glass))
    s, _, c, _ = _check(scene, osc, glass, 17, 9, 8, 4)
    lit = s.reshape(-1, 3)[c > 0]
    assert len(lit) and (lit[:, 2] == 0).all()          # whatever reached the emitter crossed the pane once or three times: no blue


# ---- 3. views, miss shaders, kernels ----------------------------------------------------------------------------------------------------
CAM = dict(eye=(4.0, 3.0, -19.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
END = dict(eye=(3.0, 4.0, -18.0), target=(0.5, 0.0, 0.0), up=(0.0, 1.0, 0.0))


def _set_view(scene, view, w, h):
    """Sets `view` on the handle and returns the composition's keywords."""
    if view == "free":
        return {}
    cam = pt.look_at(CAM["eye"], CAM["target"], CAM["up"], fov_y=60.0, aspect=w / h)
    scene.set_camera(cam)
    kw = dict(camera=cam.as_array())
    if view in ("lens", "lens_shutter"):
        scene.set_lens(0.3, 18.0)
        kw["lens"] = (0.3, 18.0)
    if view in ("shutter", "lens_shutter"):
        end = pt.look_at(END["eye"], END["target"], END["up"], fov_y=60.0, aspect=w / h)
        scene.set_camera_motion(end)
        kw["motion_end"] = end.as_array()
    if view in ("ortho", "fisheye", "equirect"):
        if view == "ortho":
            cam = pt.ortho_camera(CAM["eye"], CAM["target"], CAM["up"], view_height=12.0, aspect=w / h)
            scene.set_camera(cam)
            kw["camera"] = cam.as_array()
            prj = pt.projection("ortho")
        else:
            prj = pt.projection(view, fov_y=170.0, aspect=w / h) if view == "fisheye" else pt.projection("equirect")
        scene.set_projection(prj)
        kw["projection"] = (prj.kind, prj.span_x, prj.span_y)
    return kw


VIEWS = ["free", "camera", "lens", "shutter", "lens_shutter", "ortho", "fisheye", "equirect"]
TOR_GLASS = {4: (1.5, (0.9, 1.0, 0.9)), 2: (1.33, (1.0, 0.8, 0.6))}


@pytest.mark.parametrize("view", VIEWS)
def test_every_view_in_the_closed_room(gpu, tor, view):
    scene, osc = tor
    _reset(scene)
    scene.set_dielectrics(_entries(TOR_GLASS))
    _check(scene, osc, TOR_GLASS, 24, 20, 4, 4, **_set_view(scene, view, 24, 20))
    _reset(scene)


def _env_map(seed):
    return np.random.default_rng(seed).uniform(0.05, 2.0, (8, 8, 3)).astype(F32)


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("miss", ["skybox", "environment"])
def test_every_view_under_every_miss_shader(gpu, open_tor, miss, view):
    d, scene, osc = open_tor
    _reset(scene)
    osc.set_skybox(None)
    env = None
    if miss == "skybox":
        scene.set_skybox(d + "sky.bmp")
        osc.set_skybox(d + "sky.bmp")
    else:
        env = _env_map(3)
        scene.set_environment_map(env)
    scene.set_dielectrics(_entries(TOR_GLASS))
    try:
        _check(scene, osc, TOR_GLASS, 24, 20, 4, 4, env=env, **_set_view(scene, view, 24, 20))
    finally:
        osc.set_skybox(None)
        _reset(scene)


@pytest.mark.parametrize("miss", ["none", "skybox", "environment"])
@pytest.mark.parametrize("case", ["stats", "adaptive", "late_window"])
def test_statistics_adaptive_sampling_and_a_late_pass_window(gpu, open_tor, tor, case, miss):
    d, scene, osc = open_tor if miss != "none" else (None,) + tor
    _reset(scene)
    osc.set_skybox(None)
    env = None
    if miss == "skybox":
        scene.set_skybox(d + "sky.bmp")
        osc.set_skybox(d + "sky.bmp")
    elif miss == "environment":
        env = _env_map(4)
        scene.set_environment_map(env)
    scene.set_dielectrics(_entries(TOR_GLASS))
    try:
        kw = _set_view(scene, "camera", 24, 20)
        if case == "stats":
            st = _check(scene, osc, TOR_GLASS, 24, 20, 4, 4, env=env, stats=True, **kw)[3]
            assert st["samples_traced"] == 24 * 20 * 4 and st["segments"] > st["samples_traced"], st
        elif case == "adaptive":
            _check(scene, osc, TOR_GLASS, 24, 20, 16, 3, env=env, error=0.02, **kw)
        else:
            _check(scene, osc, TOR_GLASS, 24, 20, 4, 4, env=env, pass_begin=5, **kw)
    finally:
        osc.set_skybox(None)
        _reset(scene)


def test_adaptive_batches_over_wide_tiles(gpu, tor):
    """A frame large enough for the batch kernels' 16 x 8 and 32 x 8 tiles under adaptive sampling, compared at a sample of pixels."""
    scene, osc = tor
    _reset(scene)
    scene.set_dielectrics(_entries(TOR_GLASS))
    rng = np.random.default_rng(0)
    for w, h in ((200, 144), (640, 360)):
        px = np.unique(np.stack([rng.integers(0, w, 40), rng.integers(0, h, 40)], 1), axis=0)
        _check(scene, osc, TOR_GLASS, w, h, 14, 3, px=px, error=0.05)
    _reset(scene)


def test_box_tree_frames_equal_the_composition(gpu, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_replicated_scene as MR
    d = str(tmp_path) + "/"
    MR.generate(os.path.join(ROOT, "models"), d, "TorX4.obj", 4)
    scene, osc = pt.Scene.load_obj(d, "TorX4.obj", device=0), O.Scene.load(d, "TorX4.obj")
    assert scene.counts()[0] > pt.BIG_SCENE_TRIANGLES
    glass = {m: (1.5, (0.9, 1.0, 0.9)) for m in range(osc.n_mat) if m % 5 == 4}      # every copy's torus
    scene.set_dielectrics(_entries(glass))
    px = _all_pixels(24, 20)[::7]
    _check(scene, osc, glass, 24, 20, 3, 4, px=px, **_set_view(scene, "camera", 24, 20))
    _reset(scene)
    scene.set_dielectrics(_entries(glass))
    _check(scene, osc, glass, 24, 20, 3, 4, stats=True)
    _check(scene, osc, glass, 24, 20, 12, 3, px=px, error=0.05)
    env = _env_map(5)
    scene.set_environment_map(env)
    _check(scene, osc, glass, 24, 20, 3, 4, px=px, env=env)
    scene.close()


# ---- 4. whole frames -------------------------------------------------------------------------------------------------------------------
def _same(got, ref):
    return np.array_equal(_bits(got[0]), _bits(ref[0])) and np.array_equal(_bits(got[1]), _bits(ref[1])) and np.array_equal(got[2], ref[2])


def test_bands_a_clone_the_verification_builds_and_a_cleared_list(gpu, models_dir):
    W, H, SPP = 40, 24, 5
    scene = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    plain = scene.render_host(W, H, SPP, 8, want_stats=False)
    scene.set_dielectrics(_entries(TOR_GLASS))
    one = scene.render_host(W, H, SPP, 8, want_stats=False)
    assert not _same(one, plain)
    parts = [scene.render_host(W, H, SPP, 8, rows=r, want_stats=False) for r in ((0, 8), (8, 16), (16, H))]
    assert _same([np.concatenate([p[k] for p in parts]) for k in range(3)], one)
    acc = scene.render_host(W, H, 2, 8, want_stats=False)[:3]                      # two slices of passes into the same accumulators
    assert _same(scene.render_host(W, H, SPP - 2, 8, pass_begin=2, accum=acc, want_stats=False), one)
    clone = scene.clone_to_device(0)                                               # a clone inherits the list
    assert [(e.material, e.ior) for e in clone.dielectrics()] == [(4, 1.5), (2, F32(1.33))]
    assert _same(clone.render_host(W, H, SPP, 8, want_stats=False), one)
    clone.close()
    scene.set_dielectrics(None)                                                    # set and cleared: the parent's bytes
    assert scene.dielectrics() == [] and _same(scene.render_host(W, H, SPP, 8, want_stats=False), plain)
    scene.close()
    for path in (pt.VERIFY_LIB_PATH, os.path.join(os.path.dirname(pt.VERIFY_LIB_PATH), "libpt_verify_shipped.so")):
        L = pt.load_library(path)
        sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0, library=L)
        sc.set_dielectrics(_entries(TOR_GLASS))
        r = sc.render_host(W, H, SPP, 8, want_stats=True)
        assert r[3]["verify_checked"] > W * H and r[3]["verify_mismatches"] == 0, r[3]
        assert _same(r, one)
        sc.close()


def test_a_rehearsed_three_band_frame_inherits_the_list_or_is_given_it(gpu, models_dir):
    W, H, SPP = 40, 24, 5
    a = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    plain = a.render_host(W, H, SPP, 8, error=-1.0, want_stats=False)
    a.set_dielectrics(_entries(TOR_GLASS))
    want = a.render_host(W, H, SPP, 8, error=-1.0, want_stats=False)
    g = pt.Frame(a, [0, 0, 0], W, H, flags=pt.FRAME_REHEARSE)                      # made from a scene with a list: inherits it
    assert len(g.dielectrics()) == 2
    g.render(0, SPP, 8, error=-1.0)
    assert _same(g.read(), want)
    a.set_dielectrics(None)
    f = pt.Frame(a, [0, 0, 0], W, H, flags=pt.FRAME_REHEARSE)                      # made without one, given one afterwards
    assert f.dielectrics() == []
    f.render(0, SPP, 8, error=-1.0)
    assert _same(f.read(), plain)
    f.clear()
    with pytest.raises(pt.PtError):
        f.set_dielectrics([pt.dielectric(0, 1.5)])                                 # refused: no copy changes
    assert f.dielectrics() == []
    f.set_dielectrics(_entries(TOR_GLASS))
    f.render(0, SPP, 8, error=-1.0)
    assert _same(f.read(), want)
    f.clear()
    f.set_dielectrics(None)
    f.render(0, SPP, 8, error=-1.0)
    assert _same(f.read(), plain)
    f.close()
    g.close()
    a.close()


def test_the_phase_timer_build_refuses_a_handle_with_dielectrics(gpu, models_dir):
    """The diagnostic builds are linked without the dielectric kernels: PT_ERR_UNSUPPORTED, and the same handle renders once the list is gone."""
    L = pt.load_library(os.path.join(os.path.dirname(pt.VERIFY_LIB_PATH), "libpt_phase.so"))
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0, library=L)
    sc.set_dielectrics(_entries(TOR_GLASS))
    with pytest.raises(pt.PtError) as e:
        sc.render_host(24, 20, 2, 4, want_stats=False)
    assert e.value.status == 7                                                     # PT_ERR_UNSUPPORTED
    sc.set_dielectrics(None)
    assert sc.render_host(24, 20, 2, 4, want_stats=False)[2].sum() > 0
    sc.close()
