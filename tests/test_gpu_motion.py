"""Camera motion on the GPU (pt_hip.h: pt_scene_set_camera_motion; pt_kernels.hip: integrate_kernel_motion and
integrate_kernel_motion_lens), bit for bit against tests/motion_composition.py, which composes the frame of a moving camera from the
CPU oracle's parts.  Small frames, with the launch planner's tile width forced through the test-hook build, so that every form of
the motion kernels runs: 16 x 8 tiles, 8 x 8 tiles, the adaptive batches over 16 x 8 and 32 x 8 tiles, the statistics kernels, the
box tree, path regeneration under a skybox -- each with and without a lens.  Then: frames of several bands, pass slices, an end pose
equal to the start pose, and every segment in the verification builds."""
import hashlib
import importlib
import os
import sys

import numpy as np
import pytest

import motion_composition as M
import oracle_lib as O

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


@pytest.fixture()
def hooks(gpu):
    """The test-hook build of the library, with the planner's overrides reset before and after."""
    L = pt.load_library(pt.TESTHOOKS_LIB_PATH)
    L.pt_test_set_mutation(b"reset", 0.0)
    yield L
    L.pt_test_set_mutation(b"reset", 0.0)


def _replica(tmp, instances):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_replicated_scene as MR
    d = os.path.join(str(tmp), f"rep{instances}") + "/"
    os.makedirs(d, exist_ok=True)
    name = f"TorX{instances}.obj"
    MR.generate(os.path.join(ROOT, "models"), d, name, instances)
    return d, name


def _open_scene(tmp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_open_scene as MO
    d = os.path.join(str(tmp), "open") + "/"
    MO.generate(os.path.join(ROOT, "models"), d, name="Open.obj")
    return d, "Open.obj"


def _sample(W, H, n=150, seed=0):
    """About 500 pixels of a W x H frame (all of a small frame): its corners, its first 32 x 8 tile, its last 8 columns and last 8
    rows in a stride (the partial tiles and their tail lanes), one pixel of every 16 x 8 tile, and n more drawn at random over the whole frame."""
    if W * H <= 500:
        ys, xs = np.mgrid[0:H, 0:W]
        return np.stack([xs.ravel(), ys.ravel()], 1)
    rng = np.random.default_rng(seed)
    fixed = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)] + [(x, y) for y in range(8) for x in range(32)]
    fixed += [(x, y) for x in range(W - 8, W) for y in range(0, H, 3)] + [(x, y) for y in range(H - 8, H) for x in range(0, W, 3)]
    fixed += [(min(tx + 5, W - 1), min(ty + 3, H - 1)) for tx in range(0, W, 16) for ty in range(0, H, 8)]      # one pixel of every tile
    rest = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1)
    px = np.unique(np.concatenate([np.array(fixed), rest]), axis=0)
    have = {tuple(p) for p in px.tolist()}
    assert {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)} <= have                              # the four corners
    assert sum(x >= W - 1 - (W - 1) % 8 for x, _ in have) >= 8 and sum(y >= H - 1 - (H - 1) % 8 for _, y in have) >= 8   # the last tile column and row
    assert len({(x // 16, y // 8) for x, y in have}) == -(-W // 16) * -(-H // 8)                  # every 16 x 8 tile
    return px


def _poses(W, H, which="outside"):
    """A start and an end pose: a translation and a rotation within one shutter interval."""
    if which == "outside":
        return (pt.look_at((6.0, 3.0, -15.0), (0.0, 0.0, 0.0), fov_y=45.0, aspect=W / H),
                pt.look_at((7.5, 2.5, -14.0), (1.0, -0.5, 0.5), (0.05, 1.0, 0.0), fov_y=45.0, aspect=W / H))
    if which == "inside":
        return (pt.look_at((4.0, -3.0, -6.0), (-9.5, 9.5, 9.5), (0.1, 1.0, 0.0), fov_y=70.0, aspect=W / H),
                pt.look_at((3.0, -2.0, -6.5), (-9.5, 7.5, 9.5), fov_y=70.0, aspect=W / H))
    if which == "open":     # from outside the open side of the room
        return (pt.look_at((6.0, 3.0, 25.0), (0.0, 0.0, 0.0), fov_y=65.0, aspect=W / H),
                pt.look_at((4.0, 4.0, 27.0), (1.0, 0.0, 0.0), fov_y=65.0, aspect=W / H))
    if which == "far":      # the end pose far out: at t -> 1 the origins lie at the far end of the envelope
        return (pt.look_at((6.0, 3.0, -15.0), (0.0, 0.0, 0.0), fov_y=45.0, aspect=W / H),
                pt.look_at((40.0, 20.0, -110.0), (0.0, 0.0, 0.0), (0.05, 1.0, 0.0), fov_y=45.0, aspect=W / H))
    raise KeyError(which)


def _check_against_composition(scene, osc, W, H, spp, mrr, err, stats, start, end, lens, seed=42):
    scene.set_camera_motion(None)
    scene.set_lens(*(lens if lens is not None else (None,)))
    scene.set_camera(start)
    scene.set_camera_motion(end)
    s, s2, c, st = scene.render_host(W, H, spp, mrr, error=err, seed=seed, want_stats=stats)
    px = _sample(W, H)
    assert len(px) == W * H or 400 <= len(px) <= 700
    i = px[:, 1] * W + px[:, 0]
    ws, ws2, wc = M.compose(osc, W, H, px, spp, mrr, start=start.as_array(), end=end.as_array(), lens=lens, seed=seed, error=err)
    assert wc.sum() > 0
    assert np.array_equal(c[i], wc), int((c[i] != wc).sum())
    assert np.array_equal(_bits(s.reshape(-1, 3)[i]), _bits(ws)) and np.array_equal(_bits(s2.reshape(-1, 3)[i]), _bits(ws2))
    return s, s2, c, st


# ---- 1. device frames equal the composition --------------------------------------------------------------------------------
# tile_width: the planner's override (pt_launch_plan.hpp: Overrides) -- 1 = 8 x 8 tiles, 2 = 16 x 8 (and batches over them with
# adaptive sampling on), 3 = the same and 32 x 8 for adaptive launches
@pytest.mark.parametrize("W,H,spp,err,stats,tile_width,poses,lens", [
    (48, 40, 3, -1.0, False, 2, "outside", None),       # two pixels per lane, 16 x 8 tiles
    (48, 40, 3, -1.0, True, 2, "outside", None),        # the statistics kernel
    (50, 43, 3, -1.0, False, 2, "inside", None),        # partial tiles in both directions
    (24, 16, 3, -1.0, False, 1, "outside", None),       # the 8 x 8 narrow kernel
    (48, 40, 6, 0.02, False, 2, "outside", None),       # adaptive batches over 16 x 8 tiles
    (50, 43, 6, 0.02, False, 3, "inside", None),        # ... over 32 x 8 tiles
    (48, 40, 3, -1.0, False, 2, "outside", (0.5, 16.0)),
    (48, 40, 3, -1.0, True, 2, "inside", (0.3, 8.0)),
    (24, 16, 3, -1.0, False, 1, "outside", (0.5, 16.0)),
    (50, 43, 6, 0.02, False, 2, "inside", (0.3, 8.0)),
    (50, 43, 6, 0.02, False, 3, "outside", (0.5, 16.0)),
], ids=["wide", "stats", "partial", "narrow", "adapt16", "adapt32", "lens_wide", "lens_stats", "lens_narrow", "lens_adapt16", "lens_adapt32"])
def test_motion_frames_on_tor_equal_the_composition(hooks, models_dir, oracle_scene, W, H, spp, err, stats, tile_width, poses, lens):
    hooks.pt_test_set_mutation(b"tile_width", float(tile_width))
    scene = pt.Scene.load_obj(models_dir, "Tor.obj", device=0, library=hooks)
    start, end = _poses(W, H, poses)
    moving = _check_against_composition(scene, oracle_scene, W, H, spp, 3, err, stats, start, end, lens)
    scene.set_camera_motion(None)
    still = scene.render_host(W, H, spp, 3, error=err, want_stats=False)
    assert _digest(*moving[:3]) != _digest(*still[:3])            # the motion changed the frame
    scene.close()


def test_the_product_library_picks_the_motion_kernels_too(gpu, models_dir, oracle_scene):
    """No hook: at this size the planner takes the 8 x 8 kernel."""
    scene = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    start, end = _poses(48, 40, "outside")
    _check_against_composition(scene, oracle_scene, 48, 40, 3, 3, -1.0, False, start, end, None)
    _check_against_composition(scene, oracle_scene, 48, 40, 3, 3, -1.0, False, start, end, (0.5, 16.0))
    scene.close()


@pytest.mark.parametrize("err,tile_width", [(-1.0, 0), (0.02, 2), (0.02, 3)], ids=["plain", "adapt16", "adapt32"])
def test_motion_frames_on_the_box_tree_equal_the_composition(hooks, tmp_path, err, tile_width):
    d, name = _replica(tmp_path, 9)
    osc = O.Scene.load(d, name)
    hooks.pt_test_set_mutation(b"tile_width", float(tile_width))
    scene = pt.Scene.load_obj(d, name, device=0, library=hooks)
    assert scene.cull_layout(1e-4)["bvh"].size > 0               # the box tree, not the sphere trees
    start, end = _poses(48, 40, "outside")
    spp = 6 if err > 0 else 3
    _check_against_composition(scene, osc, 48, 40, spp, 3, err, False, start, end, None)
    _check_against_composition(scene, osc, 48, 40, spp, 3, err, False, start, end, (0.5, 16.0))
    if err < 0:
        _check_against_composition(scene, osc, 48, 40, spp, 3, err, True, start, end, None)       # the statistics kernel
    scene.close()


@pytest.mark.parametrize("mrr", [1, 3])
def test_motion_frames_under_a_skybox_equal_the_composition(gpu, tmp_path, mrr):
    d, name = _open_scene(tmp_path)
    osc = O.Scene.load(d, name)
    osc.set_skybox(d + "sky.bmp")
    scene = pt.Scene.load_obj(d, name, device=0)
    scene.set_skybox(d + "sky.bmp")
    start, end = _poses(48, 40, "open")
    for stats, lens in ((False, None), (True, None), (False, (0.8, 25.0))):
        s, s2, c, st = _check_against_composition(scene, osc, 48, 40, 6, mrr, -1.0, stats, start, end, lens)
        if stats:
            assert st["misses"] > 0
    scene.close()


# ---- 2. bands, slices, no motion ----------------------------------------------------------------------------------------------
def test_a_rehearsed_three_band_frame_with_motion_equals_the_one_band_frame(gpu, models_dir):
    W, H, spp = 48, 40, 4
    start, end = _poses(W, H, "outside")
    a = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    a.set_camera(start)
    a.set_camera_motion(end)
    want = a.render_host(W, H, spp, 3, error=-1.0, want_stats=False)
    g = pt.Frame(a, [0, 0, 0], W, H, flags=pt.FRAME_REHEARSE)   # made from a scene with a motion: inherits it
    g.render(0, spp, 3, error=-1.0)
    assert _digest(*g.read()) == _digest(*want[:3])
    a.set_camera_motion(None)
    still = a.render_host(W, H, spp, 3, error=-1.0, want_stats=False)
    assert _digest(*still[:3]) != _digest(*want[:3])
    f = pt.Frame(a, [0, 0, 0], W, H, flags=pt.FRAME_REHEARSE)   # made without one, given one afterwards
    f.render(0, spp, 3, error=-1.0)
    assert _digest(*f.read()) == _digest(*still[:3])
    f.clear()
    f.set_camera_motion(end)
    f.render(0, spp, 3, error=-1.0)
    assert _digest(*f.read()) == _digest(*want[:3])
    f.close()
    g.close()


@pytest.mark.parametrize("lens", [None, (0.5, 16.0)], ids=["pinhole", "lens"])
def test_an_end_pose_equal_to_the_start_pose_gives_the_still_frame(gpu, models_dir, lens):
    W, H, spp = 48, 40, 4
    start, end = _poses(W, H, "outside")
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    sc.set_camera(start)
    if lens:
        sc.set_lens(*lens)
    still = sc.render_host(W, H, spp, 3, error=-1.0, want_stats=False)
    sc.set_camera_motion(start)
    assert sc.get_camera_motion() is None
    assert _digest(*sc.render_host(W, H, spp, 3, error=-1.0, want_stats=False)[:3]) == _digest(*still[:3])
    sc.set_camera_motion(end)
    assert _digest(*sc.render_host(W, H, spp, 3, error=-1.0, want_stats=False)[:3]) != _digest(*still[:3])
    sc.set_camera(end)                                           # the camera catches up with the end pose: no motion again
    at_end = sc.render_host(W, H, spp, 3, error=-1.0, want_stats=False)
    sc.set_camera_motion(None)
    assert _digest(*sc.render_host(W, H, spp, 3, error=-1.0, want_stats=False)[:3]) == _digest(*at_end[:3])
    sc.close()


def test_pass_slices_of_a_motion_frame_add_up(gpu, models_dir):
    W, H = 48, 40
    start, end = _poses(W, H, "inside")
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    sc.set_camera(start)
    sc.set_lens(0.3, 8.0)
    sc.set_camera_motion(end)
    whole = sc.render_host(W, H, 5, 3, error=-1.0, want_stats=False)
    s, s2, c, _ = sc.render_host(W, H, 2, 3, error=-1.0, want_stats=False)
    sc.render_host(W, H, 3, 3, error=-1.0, want_stats=False, pass_begin=2, accum=(s, s2, c))
    assert _digest(s, s2, c) == _digest(*whole[:3])
    sc.close()


# ---- 3. every segment against the all-triangles loop ------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [None, (2.0, 30.0)], ids=["pinhole", "lens"])
def test_every_segment_of_motion_frames(gpu, models_dir, lens):
    v = pt.load_library(pt.VERIFY_LIB_PATH)
    shipped = pt.load_library(os.path.join(os.path.dirname(pt.VERIFY_LIB_PATH), "libpt_verify_shipped.so"))
    W, H, spp = 96, 64, 4
    start, end = _poses(W, H, "far")
    out = []
    for lib in (v, shipped, None):
        if lib is not None:
            lib.pt_test_set_mutation(b"reset", 0.0)
        sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0, library=lib)
        sc.set_camera(start)
        if lens:
            sc.set_lens(*lens)
        sc.set_camera_motion(end)
        r = sc.render_host(W, H, spp, 8, error=-1.0, want_stats=lib is not None)
        if lib is v:
            assert r[3]["verify_checked"] == r[3]["segments"] > W * H * spp // 2, r[3]
        if lib is not None:
            assert r[3]["verify_mismatches"] == 0, r[3]
        out.append(_digest(*r[:3]))
        sc.close()
    assert out[0] == out[1] == out[2]
