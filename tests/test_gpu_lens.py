"""The thin lens on the GPU (pt_hip.h: pt_lens; pt_kernels.hip: integrate_kernel_lens), against a second oracle.

tests/view_composition.py composes, from the CPU oracle's own parts, the accumulators of any camera and lens bit for bit (it
equals orc_render for the reference view: tests/test_lens_host.py).  Device frames of lens cameras -- through every kind of
lens kernel the planner picks -- must equal it at a sample of their pixels (the composition is pixel-local, as the counter RNG
is).  One case without a lens ties the camera twins to the same oracle.  Then: multi-band frames, every segment in the
verification builds, and pt_render's lens flags."""
import hashlib
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import view_composition as V

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _digest(s, s2, c):
    return hashlib.sha256(np.ascontiguousarray(s).tobytes() + np.ascontiguousarray(s2).tobytes() + np.ascontiguousarray(c).tobytes()).hexdigest()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def gpu():
    assert pt.device_count() >= 1, "no HIP device: the integrator has no CPU fallback"


def _replica(tmp, instances):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_replicated_scene as M
    d = os.path.join(str(tmp), f"rep{instances}") + "/"
    os.makedirs(d, exist_ok=True)
    name = f"TorX{instances}.obj"
    M.generate(os.path.join(ROOT, "models"), d, name, instances)
    return d, name


def _open_scene(tmp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_open_scene as MO
    d = os.path.join(str(tmp), "open") + "/"
    MO.generate(os.path.join(ROOT, "models"), d, name="Open.obj")
    return d, "Open.obj"


def _sample(W, H, n, seed=0):
    """n pixels of a W x H frame: its corners, one whole 32 x 8 tile, and the rest drawn at random."""
    rng = np.random.default_rng(seed)
    fixed = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)] + [(x, y) for y in range(8) for x in range(32)]
    rest = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1)
    return np.unique(np.concatenate([np.array(fixed), rest]), axis=0)


def _emitter_camera(models_dir, aspect):
    """A camera inside the room below the ceiling emitter, looking at it, focused on its plane."""
    tri, mat = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1).triangles()
    centre = tri[mat == 0, 4:13].reshape(-1, 3).mean(0).astype(np.float64)
    eye = centre + np.array([-3.0, -4.5, -2.5])
    cam = pt.look_at(eye, centre, fov_y=50.0, aspect=aspect)
    return cam, float(np.linalg.norm(centre - eye))


def _cameras(models_dir, W, H):
    emit, d_emit = _emitter_camera(models_dir, W / H)
    return {
        "outside": (pt.look_at((6.0, 3.0, -15.0), (0.0, 0.0, 0.0), fov_y=45.0, aspect=W / H), (0.5, float(np.sqrt(36 + 9 + 225)))),
        "inside": (pt.look_at((4.0, -3.0, -6.0), (-9.5, 9.5, 9.5), (0.1, 1.0, 0.0), fov_y=70.0, aspect=W / H), (0.3, 8.0)),
        "emitter": (emit, (0.6, d_emit)),
        "no_lens": (pt.look_at((-5.0, 2.0, -18.0), (1.0, -1.0, 2.0), fov_y=50.0, aspect=W / H), None),
    }


def _check_against_composition(scene, osc, W, H, spp, mrr, err, stats, cam, lens, n_px=500, seed=42):
    scene.set_camera(cam)
    scene.set_lens(*(lens if lens is not None else (None,)))
    s, s2, c, st = scene.render_host(W, H, spp, mrr, error=err, seed=seed, want_stats=stats)
    px = _sample(W, H, n_px)
    i = px[:, 1] * W + px[:, 0]
    ws, ws2, wc = V.compose(osc, W, H, px, spp, mrr, camera=cam.as_array(), lens=lens, seed=seed, error=err)
    assert wc.sum() > 0
    assert np.array_equal(c[i], wc), int((c[i] != wc).sum())
    assert np.array_equal(_bits(s.reshape(-1, 3)[i]), _bits(ws)) and np.array_equal(_bits(s2.reshape(-1, 3)[i]), _bits(ws2))
    return s, s2, c, st


# ---- 1. device frames equal the composition --------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,spp,err,stats,view", [
    (1920, 1080, 4, -1.0, False, "outside"),     # two pixels per lane (16 x 8 tiles)
    (256, 256, 8, -1.0, False, "inside"),        # one pixel per lane (8 x 8 tiles)
    (1920, 1080, 24, 0.001, False, "emitter"),   # adaptive batches over 32 x 8 tiles
    (1280, 720, 24, 0.001, False, "outside"),    # ... over 16 x 8 tiles
    (640, 360, 8, 0.001, True, "inside"),        # a statistics launch
    (640, 360, 8, 0.001, True, "emitter"),
    (1920, 1080, 4, -1.0, False, "no_lens"),     # the camera twin itself against the second oracle
    (256, 256, 8, 0.001, True, "no_lens"),
], ids=["wide", "narrow", "adapt32", "adapt16", "stats_inside", "stats_emitter", "twin_wide", "twin_stats"])
def test_lens_frames_on_tor_equal_the_composition(gpu, models_dir, oracle_scene, W, H, spp, err, stats, view):
    cam, lens = _cameras(models_dir, W, H)[view]
    scene = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    _check_against_composition(scene, oracle_scene, W, H, spp, 8, err, stats, cam, lens)
    scene.close()


@pytest.mark.parametrize("err", [-1.0, 0.001])
def test_lens_frames_on_the_box_tree_equal_the_composition(gpu, tmp_path, models_dir, err):
    d, name = _replica(tmp_path, 64)
    osc = O.Scene.load(d, name)
    scene = pt.Scene.load_obj(d, name, device=0)
    for (W, H), view in (((960, 540), "outside"), ((1920, 1080), "inside")):
        cam, lens = _cameras(models_dir, W, H)[view]
        _check_against_composition(scene, osc, W, H, 12, 8, err, False, cam, lens, n_px=120)
    cam, lens = _cameras(models_dir, 64, 64)["outside"]
    _check_against_composition(scene, osc, 64, 64, 2, 8, -1.0, True, cam, lens, n_px=60)   # the statistics kernel
    scene.close()


@pytest.mark.parametrize("mrr", [1, 3, 8])
def test_lens_frames_under_a_skybox_equal_the_composition(gpu, tmp_path, mrr):
    d, name = _open_scene(tmp_path)
    osc = O.Scene.load(d, name)
    osc.set_skybox(d + "sky.bmp")
    scene = pt.Scene.load_obj(d, name, device=0)
    scene.set_skybox(d + "sky.bmp")
    cam = pt.look_at((6.0, 3.0, 25.0), (0.0, 0.0, 0.0), fov_y=65.0, aspect=480 / 270)   # from outside the open side of the room
    for stats in (False, True):
        s, s2, c, st = _check_against_composition(scene, osc, 480, 270, 16, mrr, -1.0, stats, cam, (0.8, 25.0), n_px=400)
        if stats:
            assert st["misses"] > 0
    scene.close()


# ---- 2. frames of several bands ---------------------------------------------------------------------------------------------
def test_a_rehearsed_three_band_frame_with_a_lens_equals_the_one_band_frame(gpu, models_dir):
    W, H, spp = 640, 360, 8
    cam, lens = _cameras(models_dir, W, H)["outside"]
    a = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    a.set_camera(cam)
    a.set_lens(*lens)
    want = a.render_host(W, H, spp, 8, error=-1.0, want_stats=False)
    g = pt.Frame(a, [0, 0, 0], W, H, flags=pt.FRAME_REHEARSE)   # made from a scene with a lens: inherits it
    g.render(0, spp, 8, error=-1.0)
    assert _digest(*g.read()) == _digest(*want[:3])
    a.set_lens(None)
    pinhole = a.render_host(W, H, spp, 8, error=-1.0, want_stats=False)
    assert _digest(*pinhole[:3]) != _digest(*want[:3])
    f = pt.Frame(a, [0, 0, 0], W, H, flags=pt.FRAME_REHEARSE)   # made without one, given one afterwards
    f.render(0, spp, 8, error=-1.0)
    assert _digest(*f.read()) == _digest(*pinhole[:3])
    f.clear()
    f.set_lens(*lens)
    f.render(0, spp, 8, error=-1.0)
    assert _digest(*f.read()) == _digest(*want[:3])
    f.close()
    g.close()


# ---- 3. every segment against the all-triangles loop ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vlibs(gpu):
    v = pt.load_library(pt.VERIFY_LIB_PATH)
    v.pt_test_set_mutation(b"reset", 0.0)
    shipped = pt.load_library(os.path.join(os.path.dirname(pt.VERIFY_LIB_PATH), "libpt_verify_shipped.so"))
    shipped.pt_test_set_mutation(b"reset", 0.0)
    return v, shipped


@pytest.mark.parametrize("scene", ["tor", "x64", "sky"])
def test_every_segment_of_lens_frames(tmp_path, models_dir, vlibs, scene):
    v, shipped = vlibs
    W, H = 512, 512
    sky = None
    if scene == "sky":
        d, name = _open_scene(tmp_path)
        sky = d + "sky.bmp"
        views = {"open_side": (pt.look_at((6.0, 3.0, 25.0), (0.0, 0.0, 0.0), fov_y=65.0), (2.0, 25.0))}
    else:
        d, name = (models_dir, "Tor.obj") if scene == "tor" else _replica(tmp_path, 64)
        views = {k: val for k, val in _cameras(models_dir, W, H).items() if val[1] is not None}
        views["wide_aperture"] = (pt.look_at((1.0, 0.5, -35.0), (0.0, 0.0, 0.0), fov_y=40.0), (5.0, 30.0))
    for label, (cam, lens) in views.items():
        out = []
        for lib in (v, shipped, None):
            sc = pt.Scene.load_obj(d, name, device=0, library=lib)
            if sky:
                sc.set_skybox(sky)
            sc.set_camera(cam)
            sc.set_lens(*lens)
            r = sc.render_host(W, H, 16, 8, error=-1.0, want_stats=lib is not None)
            if lib is v:
                assert r[3]["verify_checked"] == r[3]["segments"] > W * H * 16 // 2, (label, r[3])
            if lib is not None:
                assert r[3]["verify_mismatches"] == 0, (label, r[3])
            out.append(_digest(*r[:3]))
            sc.close()
        assert out[0] == out[1] == out[2], label


# ---- 4. pt_render -----------------------------------------------------------------------------------------------------------
def test_pt_render_lens_flags(gpu, tmp_path, models_dir):
    exe = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
    W, H, spp = 320, 200, 16
    base = [exe, "--W", str(W), "--H", str(H), "-RPP", str(spp), "-MRR", "8", "-MODEL_PATH", models_dir, "-QUIET", "1"]
    view = ["-EYE", "6,3,-15", "-LOOKAT", "0,0,0", "-FOV", "45", "-ASPECT", "1.6"]
    outs = {}
    for label, extra in (("plain", []), ("aperture0", ["-APERTURE", "0"]), ("view", view), ("view0", view + ["-APERTURE", "0", "-FOCUS", "3"]),
                         ("lens", view + ["-APERTURE", "0.5"]), ("lens_bands", view + ["-APERTURE", "0.5", "-GPUS", "3", "-REHEARSE", "1"])):
        path = os.path.join(str(tmp_path), label + ".bmp")
        p = subprocess.run(base + extra + ["-OUT", path], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (label, p.stderr)
        outs[label] = open(path, "rb").read()
    assert outs["plain"] == outs["aperture0"]
    assert outs["view"] == outs["view0"]
    assert outs["lens"] != outs["view"]
    assert outs["lens_bands"] == outs["lens"]
    # the same frame through the Python path: pt_render's defaults are the reference's (seed 42, -ERR 0.001, gamma 1 / 2.2)
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    sc.set_camera(pt.look_at((6, 3, -15), (0, 0, 0), fov_y=45.0, aspect=1.6))
    sc.set_lens(0.5, float(np.float32(np.sqrt(36 + 9 + 225))))
    s, s2, c, _ = sc.render_host(W, H, spp, 8, error=0.001, seed=42, want_stats=False)
    bgr, _ = pt.resolve(W, H, s, s2, c)
    mine = os.path.join(str(tmp_path), "python.bmp")
    pt.write_bmp(mine, bgr)
    assert open(mine, "rb").read() == outs["lens"]
    sc.close()
