"""Environment lighting on the GPU (pt_hip.h: pt_environment_*; pt_kernels.hip: integrate_kernel_environment), bit for bit against
tests/environment_composition.py: projection_composition's frame with a restated miss (throughput x the octahedral map's lookup,
tests/environment_restatement.py).  The lookup alone on a scene no ray hits, then frames of the open room through every view, the
statistics kernels, adaptive sampling, a late pass window, the box tree and the envelope-test kernels; bands, a rehearsed frame, slices,
clones, the verification builds, the feature pass; that the
throughput is applied; and the orientation from a picture to the rendered panorama."""
import importlib
import os
import sys

import numpy as np
import pytest

import environment_composition as EC
import environment_restatement as E
import oracle_lib as O
from glass_fuzz_scenes import _sliver_scene

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
W, H, SPP = 40, 24, 6      # two and a half 16-wide tiles, three tile rows


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def gpu():
    assert pt.device_count() >= 1, "no HIP device: the integrator has no CPU fallback"


def _map(n, seed=0):
    """Random positive texels with a few at 1e4."""
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.05, 2.0, (n, n, 3)).astype(F32)
    for k in range(4):
        m[rng.integers(0, n), rng.integers(0, n)] = F32(1e4)
    return m


@pytest.fixture(scope="module")
def open_scene(tmp_path_factory):
    """Tor.obj without its back wall, and the same scene for the oracle."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_open_scene as MO
    d = str(tmp_path_factory.mktemp("open")) + "/"
    MO.generate(os.path.join(ROOT, "models"), d, name="Open.obj")
    return d, "Open.obj", O.Scene.load(d, "Open.obj")


@pytest.fixture(scope="module")
def speck(tmp_path_factory):
    """A scene no ray of these frames hits: one triangle a thousandth of a unit wide, a thousand units below the camera."""
    d = str(tmp_path_factory.mktemp("speck")) + "/"
    open(d + "Tor.mtl", "w").write(open(os.path.join(ROOT, "models", "Tor.mtl")).read())
    open(d + "Speck.obj", "w").write("mtllib Tor.mtl\no S\nv 0.0 -1000.0 0.0\nv 0.001 -1000.0 0.0\nv 0.0 -1000.0 0.001\nvn 0.0 1.0 0.0\nusemtl 1\ns off\nf 1//1 2//1 3//1\n")
    return d, "Speck.obj", O.Scene.load(d, "Speck.obj")


def _all_pixels(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.ravel(), ys.ravel()], 1)


def _sample(w, h, n=60, seed=0):
    """The corners, the first tile row's first 24 columns, the last columns and rows (the partial tiles), one pixel per 8 x 8 block, n at random."""
    rng = np.random.default_rng(seed)
    fixed = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)] + [(x, y) for y in range(0, 8, 2) for x in range(0, 24, 2)]
    fixed += [(x, y) for x in range(w - 8, w, 2) for y in range(0, h, 3)] + [(x, h - 1) for x in range(0, w, 3)]
    fixed += [(min(tx + 5, w - 1), min(ty + 3, h - 1)) for tx in range(0, w, 8) for ty in range(0, h, 8)]
    return np.unique(np.concatenate([np.array(fixed), np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], 1)]), axis=0)


def _check(scene, osc, env, px, spp, mrr, *, w=W, h=H, error=-1.0, stats=False, pass_begin=0, seed=42, **view):
    s, s2, c, st = scene.render_host(w, h, spp, mrr, error=error, seed=seed, want_stats=stats, pass_begin=pass_begin)
    i = px[:, 1] * w + px[:, 0]
    ws, ws2, wc = EC.compose(osc, env, w, h, px, spp, mrr, seed=seed, error=error, pass_begin=pass_begin, **view)
    assert wc.sum() > 0
    assert np.array_equal(c[i], wc), int((c[i] != wc).sum())
    assert np.array_equal(_bits(s.reshape(-1, 3)[i]), _bits(ws)) and np.array_equal(_bits(s2.reshape(-1, 3)[i]), _bits(ws2))
    return s, s2, c, st


# ---- 1. the lookup alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("kind", ["equirect", "fisheye220"])
def test_a_frame_of_misses_is_the_lookup_of_the_primary_directions(gpu, speck, n, kind):
    d, name, osc = speck
    scene = pt.Scene.load_obj(d, name, device=0)
    cam = pt.look_at((0.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), aspect=W / H)
    prj = pt.projection("equirect") if kind == "equirect" else pt.projection("fisheye", fov_y=220.0, aspect=W / H)
    env = _map(n, seed=n)
    scene.set_camera(cam)
    scene.set_projection(prj)
    scene.set_environment_map(env)
    s, s2, c, _ = _check(scene, osc, env, _all_pixels(W, H), 2, 3, camera=cam.as_array(), projection=(prj.kind, prj.span_x, prj.span_y))
    assert (c == 2).all() and s.max() > 100.0          # every primary ray missed; the bright texels are seen
    scene.close()


# ---- 2. frames equal the composition ----------------------------------------------------------------------------------------------
CAM = dict(eye=(6.0, 3.0, 25.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
END = dict(eye=(4.0, 4.0, 24.0), target=(0.5, 0.0, 0.0), up=(0.0, 1.0, 0.0))


def _set_view(scene, view):
    """Sets `view` on the handle and returns the composition's keywords."""
    scene.set_projection(None); scene.set_camera_motion(None); scene.set_lens(None); scene.set_camera(None)
    if view == "free":
        return {}
    cam = pt.look_at(CAM["eye"], CAM["target"], CAM["up"], fov_y=60.0, aspect=W / H)
    scene.set_camera(cam)
    kw = dict(camera=cam.as_array())
    if view in ("lens", "lens_shutter"):
        scene.set_lens(0.4, 22.0)
        kw["lens"] = (0.4, 22.0)
    if view in ("shutter", "lens_shutter"):
        end = pt.look_at(END["eye"], END["target"], END["up"], fov_y=60.0, aspect=W / H)
        scene.set_camera_motion(end)
        kw["motion_end"] = end.as_array()
    if view in ("ortho", "fisheye", "equirect"):
        if view == "ortho":
            cam = pt.ortho_camera(CAM["eye"], CAM["target"], CAM["up"], view_height=14.0, aspect=W / H)
            scene.set_camera(cam)
            kw["camera"] = cam.as_array()
            prj = pt.projection("ortho")
        else:
            prj = pt.projection(view, fov_y=170.0, aspect=W / H) if view == "fisheye" else pt.projection("equirect")
        scene.set_projection(prj)
        kw["projection"] = (prj.kind, prj.span_x, prj.span_y)
    return kw


@pytest.mark.parametrize("mrr", [1, 3, 8])
@pytest.mark.parametrize("view", ["free", "camera", "lens", "shutter", "lens_shutter", "ortho", "fisheye", "equirect"])
def test_open_room_frames_equal_the_composition(gpu, open_scene, view, mrr):
    d, name, osc = open_scene
    scene = pt.Scene.load_obj(d, name, device=0)
    env = _map(8, seed=3)
    scene.set_environment_map(env)
    _check(scene, osc, env, _sample(W, H), SPP, mrr, **_set_view(scene, view))
    scene.close()


@pytest.mark.parametrize("case", ["stats", "adaptive", "late_window"])
def test_statistics_adaptive_sampling_and_a_late_pass_window(gpu, open_scene, case):
    d, name, osc = open_scene
    scene = pt.Scene.load_obj(d, name, device=0)
    env = _map(8, seed=4)
    scene.set_environment_map(env)
    kw = _set_view(scene, "camera")
    if case == "stats":
        st = _check(scene, osc, env, _sample(W, H), SPP, 3, stats=True, **kw)[3]
        assert st["samples_traced"] == W * H * SPP and st["misses"] > 0, st
    elif case == "adaptive":
        _check(scene, osc, env, _sample(W, H), 16, 3, error=0.02, **kw)
    else:
        _check(scene, osc, env, _sample(W, H), SPP, 3, pass_begin=5, **kw)
    scene.close()


def test_box_tree_frames_equal_the_composition(gpu, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_replicated_scene as MR
    d = str(tmp_path) + "/"
    MR.generate(os.path.join(ROOT, "models"), d, "TorX4.obj", 4)
    scene, osc = pt.Scene.load_obj(d, "TorX4.obj", device=0), O.Scene.load(d, "TorX4.obj")
    assert scene.counts()[0] > pt.BIG_SCENE_TRIANGLES
    env = _map(8, seed=5)
    scene.set_environment_map(env)
    _check(scene, osc, env, _sample(W, H, n=20), 3, 3, **_set_view(scene, "camera"))
    _check(scene, osc, env, _sample(W, H, n=20), 3, 3, stats=True, **_set_view(scene, "free"))
    scene.close()


@pytest.mark.parametrize("n_small,stats", [(300, False), (300, True), (3000, False), (3000, True)], ids=["small", "small_stats", "box_tree", "box_tree_stats"])
def test_scenes_whose_paths_can_leave_the_envelope_equal_the_composition(gpu, tmp_path, n_small, stats):
    """A near-degenerate triangle sets CullTables::may_leave_envelope, so the launch runs the instantiations with the envelope test
    compiled in (integrate_kernel_environment<.., .., true, ..>), as tests/test_gpu_fuzz.py's scenes do for the skybox-free kernels:
    the camera-free kernel, a camera, a lens + shutter and a projection, on the sphere-tree path and on the box tree."""
    d = str(tmp_path) + "/"
    n = _sliver_scene(d, n_small, seed=n_small)
    scene, osc = pt.Scene.load_obj(d, "f.obj", device=0), O.Scene.load(d, "f.obj")
    assert scene.counts()[0] == n and (n > pt.BIG_SCENE_TRIANGLES) == (n_small == 3000)
    env = _map(8, seed=9)
    scene.set_environment_map(env)
    px = _sample(W, H, n=10)
    for view in ("free", "camera", "lens_shutter", "fisheye"):
        kw = _set_view(scene, view)
        if view != "free":                        # (the open room's camera stands behind these triangles: look at them from the front)
            cam = pt.look_at((3.0, 2.0, -22.0), (0.0, 0.0, -6.0), (0.0, 1.0, 0.0), fov_y=60.0, aspect=W / H)
            scene.set_projection(None); scene.set_camera_motion(None)
            scene.set_camera(cam)
            kw["camera"] = cam.as_array()
            if view == "lens_shutter":
                end = pt.look_at((2.0, 3.0, -21.0), (0.5, 0.0, -6.0), (0.0, 1.0, 0.0), fov_y=60.0, aspect=W / H)
                scene.set_camera_motion(end)
                kw["motion_end"] = end.as_array()
            if view == "fisheye":
                scene.set_projection(pt.projection("fisheye", fov_y=170.0, aspect=W / H))
        s, s2, c, st = _check(scene, osc, env, px, 3, 4, stats=stats, **kw)
        if stats:
            assert 0 < st["misses"] and st["segments"] > st["samples_traced"], st      # paths leave AND bounce
    scene.close()


# ---- 3. whole frames ---------------------------------------------------------------------------------------------------------------
def test_bands_slices_clones_and_the_verification_builds(gpu, open_scene):
    d, name, _ = open_scene
    env = _map(8, seed=6)
    scene = pt.Scene.load_obj(d, name, device=0)
    scene.set_environment_map(env)
    cam = pt.look_at(CAM["eye"], CAM["target"], CAM["up"], fov_y=60.0, aspect=W / H)
    scene.set_camera(cam)
    one = scene.render_host(W, H, SPP, 8, want_stats=False)
    # three bands of rows
    parts = [scene.render_host(W, H, SPP, 8, rows=r, want_stats=False) for r in ((0, 8), (8, 16), (16, H))]
    for k in range(3):
        assert np.array_equal(_bits(np.concatenate([p[k].reshape(-1) for p in parts])) if k < 2 else np.concatenate([p[2] for p in parts]),
                              _bits(one[k].reshape(-1)) if k < 2 else one[2])
    # two slices of passes into the same accumulators
    acc = scene.render_host(W, H, 2, 8, want_stats=False)[:3]
    two = scene.render_host(W, H, SPP - 2, 8, pass_begin=2, accum=acc, want_stats=False)
    assert all(np.array_equal(_bits(a) if a.dtype != np.int32 else a, _bits(b) if b.dtype != np.int32 else b) for a, b in zip(two[:3], one[:3]))
    # a clone inherits the environment
    clone = scene.clone_to_device(0)
    assert np.array_equal(clone.environment(), env)
    cl = clone.render_host(W, H, SPP, 8, want_stats=False)
    assert np.array_equal(_bits(cl[0]), _bits(one[0])) and np.array_equal(cl[2], one[2])
    clone.close()
    scene.close()
    # every segment against the all-triangles loop
    for path in (pt.VERIFY_LIB_PATH, os.path.join(os.path.dirname(pt.VERIFY_LIB_PATH), "libpt_verify_shipped.so")):
        L = pt.load_library(path)
        sc = pt.Scene.load_obj(d, name, device=0, library=L)
        sc.set_environment_map(env)
        sc.set_camera(cam)
        r = sc.render_host(W, H, SPP, 8, want_stats=True)
        assert r[3]["verify_checked"] > W * H and r[3]["verify_mismatches"] == 0, r[3]
        assert np.array_equal(_bits(r[0]), _bits(one[0])) and np.array_equal(r[2], one[2])
        sc.close()


def test_a_rehearsed_three_band_frame_equals_the_one_band_frame(gpu, open_scene):
    d, name, _ = open_scene
    env = _map(8, seed=7)
    a = pt.Scene.load_obj(d, name, device=0)
    cam = pt.look_at(CAM["eye"], CAM["target"], CAM["up"], fov_y=60.0, aspect=W / H)
    a.set_camera(cam)
    a.set_environment_map(env)
    want = a.render_host(W, H, SPP, 8, error=-1.0, want_stats=False)

    def same(got, ref):
        return np.array_equal(_bits(got[0]), _bits(ref[0])) and np.array_equal(_bits(got[1]), _bits(ref[1])) and np.array_equal(got[2], ref[2])

    g = pt.Frame(a, [0, 0, 0], W, H, flags=pt.FRAME_REHEARSE)     # made from a scene with an environment: inherits it
    assert np.array_equal(g.environment(), env)
    g.render(0, SPP, 8, error=-1.0)
    assert same(g.read(), want)
    a.set_environment(None)
    plain = a.render_host(W, H, SPP, 8, error=-1.0, want_stats=False)
    assert not same(plain, want)
    f = pt.Frame(a, [0, 0, 0], W, H, flags=pt.FRAME_REHEARSE)     # made without one, given one afterwards
    assert f.environment() is None
    f.render(0, SPP, 8, error=-1.0)
    assert same(f.read(), plain)
    f.clear()
    f.set_environment_map(env)
    f.render(0, SPP, 8, error=-1.0)
    assert same(f.read(), want)
    f.clear()
    f.set_environment(None)
    f.render(0, SPP, 8, error=-1.0)
    assert same(f.read(), plain)
    f.close()
    g.close()
    a.close()


def test_a_miss_pixels_features_are_what_they_are_under_a_skybox(gpu, open_scene):
    """The first-hit feature pass does not look at the environment: the same buffers without one, with one and under a skybox."""
    d, name, _ = open_scene
    sc = pt.Scene.load_obj(d, name, device=0)
    sc.set_camera(pt.look_at(CAM["eye"], CAM["target"], CAM["up"], fov_y=60.0, aspect=W / H))
    plain = sc.render_features(W, H)
    sc.set_environment_map(_map(8, seed=8))
    lit = sc.render_features(W, H)
    sc.set_environment(None)
    sc.set_skybox(d + "sky.bmp")
    sky = sc.render_features(W, H)
    miss = plain["hit_index"] < 0
    assert 0 < miss.sum() < miss.size
    for k in plain:
        for other in (lit, sky):
            assert np.array_equal(plain[k].view(np.uint32) if plain[k].dtype == np.float32 else plain[k],
                                  other[k].view(np.uint32) if other[k].dtype == np.float32 else other[k]), k
    assert np.isinf(lit["hit_t"][miss]).all() and not lit["position"][miss].any() and not lit["normal"][miss].any() and not lit["albedo"][miss].any()
    sc.close()


# ---- 4. the throughput is applied ----------------------------------------------------------------------------------------------------
def test_a_coloured_wall_under_a_white_sky_reflects_its_colour(gpu, tmp_path):
    """The only surface is red diffuse (Kd 1, 0.01, 0.01), a wall of 10 x 10 units that fills the view (the reference's area test
    loses hits on much larger triangles); the environment is constant white.  Whatever a hit pixel
    accumulates left the wall: its channels stand as the wall's, where the skybox's rule (no throughput) would give 1 : 1 : 1."""
    d = str(tmp_path) + "/"
    open(d + "Tor.mtl", "w").write("newmtl 0\nNs 0.0\nKd 1.0 0.01 0.01\nKs 0.0 0.0 0.0\nKe 0.0 0.0 0.0\n")      # one lobe: diffuse
    open(d + "Wall.obj", "w").write("mtllib Tor.mtl\no W\nv -5.0 -5.0 -12.0\nv 5.0 -5.0 -12.0\nv 5.0 5.0 -12.0\nv -5.0 5.0 -12.0\nvn 0.0 0.0 -1.0\n"
                                    "usemtl 0\ns off\nf 1//1 2//1 3//1\nf 1//1 3//1 4//1\n")
    scene = pt.Scene.load_obj(d, "Wall.obj", device=0)
    scene.set_environment_map(np.ones((8, 8, 3), F32))
    s, _, c, _ = scene.render_host(W, H, 8, 4, want_stats=False)
    s = s.reshape(-1, 3)
    assert (c > 0).all() and (s[:, 0] > 0).all()
    assert np.abs(s[:, 1] / s[:, 0] - 0.01).max() < 1e-4 and np.abs(s[:, 2] / s[:, 0] - 0.01).max() < 1e-4
    scene.close()


# ---- 5. orientation ------------------------------------------------------------------------------------------------------------------
def test_a_bright_block_of_the_picture_is_seen_where_it_lies(gpu, speck):
    d, name, _ = speck
    pic = np.full((32, 64, 3), 0.01, F32)
    pic[9:11, 44:46] = 500.0
    scene = pt.Scene.load_obj(d, name, device=0)
    scene.set_environment(pic, size=64)
    scene.set_camera(pt.look_at((0.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), aspect=2.0))     # the picture's own frame (pt_hip.h)
    scene.set_projection("equirect")
    s, _, c, _ = scene.render_host(64, 32, 4, 2, want_stats=False)
    y, x = np.unravel_index(np.argmax(s.reshape(32, 64, 3).sum(-1)), (32, 64))
    assert 43 <= x <= 46 and 8 <= y <= 11, (x, y)
    scene.close()
