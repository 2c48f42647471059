"""The camera projections on the GPU (pt_hip.h: pt_projection; pt_kernels.hip: integrate_kernel_projection), bit for bit against
tests/projection_composition.py, which composes the frame of any projection from the CPU oracle's parts.  Small frames, with the
launch planner's tile width forced through the test-hook build, so that every form of the projection kernels runs under each of
the three kinds: 16 x 8 tiles, 8 x 8 tiles, the adaptive batches over 16 x 8 and 32 x 8 tiles, the statistics kernels, the box
tree, path regeneration under a skybox.  Then: kind perspective, the orthographic first hits, the feature pass, frames of several
bands, every segment in the verification builds, and the temporal stage's refusal."""
import hashlib
import importlib
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import projection_composition as P

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
KINDS = ["ortho", "fisheye", "equirect"]


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


def _sample(W, H, n=120, seed=0):
    """About 400 pixels of a W x H frame: its four corners, the pixels around its centre, its first 32 x 8 tile, its last 8 columns
    and rows in a stride (the partial tiles), one pixel of every 16 x 8 tile, and n more drawn at random."""
    rng = np.random.default_rng(seed)
    fixed = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    fixed += [(W // 2 + dx, H // 2 + dy) for dx in (-2, -1, 0, 1) for dy in (-2, -1, 0, 1)]
    fixed += [(x, y) for y in range(8) for x in range(min(32, W))]
    fixed += [(x, y) for x in range(W - 8, W) for y in range(0, H, 3)] + [(x, y) for y in range(H - 8, H) for x in range(0, W, 3)]
    fixed += [(min(tx + 5, W - 1), min(ty + 3, H - 1)) for tx in range(0, W, 16) for ty in range(0, H, 8)]
    rest = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1)
    px = np.unique(np.concatenate([np.array(fixed), rest]), axis=0)
    have = {tuple(p) for p in px.tolist()}
    assert {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2), (W // 2 - 1, H // 2 - 1)} <= have
    return px


def _view(kind, W, H, which="outside"):
    """A camera and a projection of `kind`.  'outside' looks at the room from in front of it, 'inside' stands in it, 'open' looks
    into the open room from its open side, 'wrap' is a fisheye whose corner angle exceeds pi (and stands inside: rays go everywhere)."""
    eye, target, up = {"outside": ((6.0, 3.0, -15.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
                       "inside": ((4.0, -3.0, -6.0), (-9.5, 9.5, 9.5), (0.1, 1.0, 0.0)),
                       "wrap": ((4.0, -3.0, -6.0), (-9.5, 9.5, 9.5), (0.1, 1.0, 0.0)),
                       "open": ((6.0, 3.0, 25.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))}[which]
    if kind == "ortho":
        # (the open room's view is wider than the room: at -MRR 1 only rays that pass it by, into the sky, carry light)
        return pt.ortho_camera(eye, target, up, view_height=30.0 if which == "open" else 14.0, aspect=W / H), pt.projection("ortho")
    cam = pt.look_at(eye, target, up, fov_y=60.0, aspect=W / H)
    if kind == "equirect":
        return cam, pt.projection("equirect")                                   # the full sphere
    if which == "wrap":
        prj = pt.projection("fisheye", fov_y=300.0, aspect=W / H)
        assert 0.5 * np.hypot(prj.span_x, prj.span_y) > np.pi                   # the corners wrap beyond straight backwards
        return cam, prj
    return cam, pt.projection("fisheye", fov_y=170.0, aspect=W / H)


def _tuple(prj):
    return (prj.kind, prj.span_x, prj.span_y)


def _check_against_composition(scene, osc, W, H, spp, mrr, err, stats, cam, prj, seed=42):
    scene.set_projection(None)
    scene.set_camera(cam)
    scene.set_projection(prj)
    s, s2, c, st = scene.render_host(W, H, spp, mrr, error=err, seed=seed, want_stats=stats)
    px = _sample(W, H)
    i = px[:, 1] * W + px[:, 0]
    ws, ws2, wc = P.compose(osc, W, H, px, spp, mrr, camera=cam.as_array(), projection=_tuple(prj), seed=seed, error=err)
    assert wc.sum() > 0
    assert np.array_equal(c[i], wc), int((c[i] != wc).sum())
    assert np.array_equal(_bits(s.reshape(-1, 3)[i]), _bits(ws)) and np.array_equal(_bits(s2.reshape(-1, 3)[i]), _bits(ws2))
    return s, s2, c, st


# ---- 1. device frames equal the composition --------------------------------------------------------------------------------
# tile_width: the planner's override (pt_launch_plan.hpp: Overrides) -- 1 = 8 x 8 tiles, 2 = 16 x 8 (and batches over them with
# adaptive sampling on), 3 = the same and 32 x 8 for adaptive launches
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,H,spp,err,stats,tile_width,which", [
    (48, 40, 3, -1.0, False, 2, "outside"),      # two pixels per lane, 16 x 8 tiles
    (50, 43, 3, -1.0, True, 2, "inside"),        # the statistics kernel; partial tiles in both directions
    (24, 16, 3, -1.0, False, 1, "outside"),      # the 8 x 8 one-pixel kernel
    (48, 40, 6, 0.02, False, 2, "inside"),       # adaptive batches over 16 x 8 tiles
    (50, 43, 6, 0.02, False, 3, "outside"),      # ... over 32 x 8 tiles
], ids=["wide", "stats", "narrow", "adapt16", "adapt32"])
def test_projection_frames_on_tor_equal_the_composition(hooks, models_dir, oracle_scene, kind, W, H, spp, err, stats, tile_width, which):
    hooks.pt_test_set_mutation(b"tile_width", float(tile_width))
    scene = pt.Scene.load_obj(models_dir, "Tor.obj", device=0, library=hooks)
    cam, prj = _view(kind, W, H, which)
    got = _check_against_composition(scene, oracle_scene, W, H, spp, 3, err, stats, cam, prj)
    scene.set_projection(None)
    pinhole = scene.render_host(W, H, spp, 3, error=err, want_stats=False)
    assert _digest(*got[:3]) != _digest(*pinhole[:3])              # the projection changed the frame
    scene.close()


def test_a_fisheye_whose_corners_wrap_and_the_product_librarys_own_choice(gpu, models_dir, oracle_scene):
    """No hook: at this size the planner takes the 8 x 8 kernel.  The corner angle exceeds pi: those pixels are rays like any other."""
    scene = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    cam, prj = _view("fisheye", 48, 40, "wrap")
    _check_against_composition(scene, oracle_scene, 48, 40, 4, 8, -1.0, False, cam, prj)      # (-MRR 8: most of these rays look away from the emitter)
    cam, prj = _view("equirect", 48, 40, "inside")
    _check_against_composition(scene, oracle_scene, 48, 40, 4, 8, -1.0, True, cam, prj)
    scene.close()


@pytest.mark.parametrize("err,tile_width", [(-1.0, 0), (0.02, 2), (0.02, 3)], ids=["plain", "adapt16", "adapt32"])
def test_projection_frames_on_the_box_tree_equal_the_composition(hooks, tmp_path, err, tile_width):
    d, name = _replica(tmp_path, 9)
    osc = O.Scene.load(d, name)
    hooks.pt_test_set_mutation(b"tile_width", float(tile_width))
    scene = pt.Scene.load_obj(d, name, device=0, library=hooks)
    assert scene.cull_layout(1e-4)["bvh"].size > 0               # the box tree, not the sphere trees
    spp = 6 if err > 0 else 3
    for kind in KINDS:
        cam, prj = _view(kind, 48, 40, "outside")
        _check_against_composition(scene, osc, 48, 40, spp, 3, err, False, cam, prj)
        if err < 0:
            _check_against_composition(scene, osc, 48, 40, spp, 3, err, True, cam, prj)       # the statistics kernel
    scene.close()


@pytest.mark.parametrize("mrr", [1, 3, 8])
def test_projection_frames_under_a_skybox_equal_the_composition(gpu, tmp_path, mrr):
    d, name = _open_scene(tmp_path)
    osc = O.Scene.load(d, name)
    osc.set_skybox(d + "sky.bmp")
    scene = pt.Scene.load_obj(d, name, device=0)
    scene.set_skybox(d + "sky.bmp")
    for kind in KINDS:
        cam, prj = _view(kind, 48, 40, "open")
        for stats in (False, True):
            s, s2, c, st = _check_against_composition(scene, osc, 48, 40, 6, mrr, -1.0, stats, cam, prj)
            if stats:
                assert st["misses"] > 0
    scene.close()


# ---- 2. kind perspective --------------------------------------------------------------------------------------------------------
def test_kind_perspective_renders_the_frame_of_a_handle_without_a_projection(gpu, models_dir):
    W, H, spp = 48, 40, 4
    cam = pt.look_at((6.0, 3.0, -15.0), (0.0, 0.0, 0.0), fov_y=45.0, aspect=W / H)
    for camera in (None, cam):
        a = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
        b = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
        a.set_camera(camera)
        b.set_camera(camera)
        b.set_projection(pt.Projection(pt.PROJECTION_PERSPECTIVE, 1.0, 2.0))
        want = a.render_host(W, H, spp, 3, error=-1.0, want_stats=False)
        got = b.render_host(W, H, spp, 3, error=-1.0, want_stats=False)
        assert _digest(*got[:3]) == _digest(*want[:3])
        b.set_projection("equirect")                               # and back from another kind
        assert _digest(*b.render_host(W, H, spp, 3, error=-1.0, want_stats=False)[:3]) != _digest(*want[:3])
        b.set_projection("perspective")
        assert _digest(*b.render_host(W, H, spp, 3, error=-1.0, want_stats=False)[:3]) == _digest(*want[:3])
        a.close()
        b.close()


# ---- 3. first hits ----------------------------------------------------------------------------------------------------------------
def test_orthographic_first_hits_lie_straight_ahead_of_their_origins(gpu, models_dir):
    """forward = (0, 0, 1), right = (w, 0, 0), up = (0, h, 0): the direction is exactly (0, 0, 1), so position x and y are the origin's."""
    W, H = 40, 24
    cam = pt.Camera.of((0.5, -0.25, -20.0), (12.0, 0.0, 0.0), (0.0, 9.0, 0.0), (0.0, 0.0, 1.0))
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    sc.set_camera(cam)
    sc.set_projection("ortho")
    f = sc.render_features(W, H)
    o, d = P.feature_rays(W, H, cam.as_array(), (P.ORTHOGRAPHIC, 0.0, 0.0))
    assert (d == np.array([0, 0, 1], F32)).all()
    hit = f["hit_index"] >= 0
    assert hit.sum() > W * H // 2
    pos = f["position"][hit]
    assert np.array_equal(_bits(pos[:, 0]), _bits(o[hit, 0])) and np.array_equal(_bits(pos[:, 1]), _bits(o[hit, 1]))
    assert np.array_equal(_bits(pos[:, 2]), _bits(o[hit, 2] + f["hit_t"][hit]))
    assert len(np.unique(_bits(pos[:, 0]))) == W and len(np.unique(_bits(pos[:, 1]))) == H   # one x per column, one y per row
    sc.close()


@pytest.mark.parametrize("kind", KINDS + ["wrap"])
def test_features_equal_the_trace_of_the_rays_the_header_defines(gpu, models_dir, kind):
    W, H = 40, 24                                                  # even: column W / 2 has u == 0 exactly, row H / 2 has v == 0
    cam, prj = _view("fisheye" if kind == "wrap" else kind, W, H, "wrap" if kind == "wrap" else "inside")
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    sc.set_camera(cam)
    o, d = P.feature_rays(W, H, cam.as_array(), _tuple(prj))
    want_hit, want_t = sc.trace_rays(o, d)                         # (pt_trace_rays_host takes no camera)
    sc.set_projection(prj)
    f = sc.render_features(W, H)
    assert np.array_equal(f["hit_index"], want_hit) and np.array_equal(_bits(f["hit_t"]), _bits(want_t))
    assert (want_hit >= 0).any()
    rows = sc.render_features(W, H, rows=(5, 17))                  # a row band is the frame's rows
    assert np.array_equal(rows["hit_index"], want_hit[5 * W:17 * W]) and np.array_equal(_bits(rows["position"]), _bits(f["position"][5 * W:17 * W]))
    sc.close()


# ---- 4. bands ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_rehearsed_three_band_frame_equals_the_one_band_frame(gpu, models_dir, kind):
    W, H, spp = 48, 40, 4
    cam, prj = _view(kind, W, H, "outside")
    a = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    a.set_camera(cam)
    a.set_projection(prj)
    want = a.render_host(W, H, spp, 3, error=-1.0, want_stats=False)
    g = pt.Frame(a, [0, 0, 0], W, H, flags=pt.FRAME_REHEARSE)   # made from a scene with a projection: inherits it
    g.render(0, spp, 3, error=-1.0)
    assert _digest(*g.read()) == _digest(*want[:3])
    a.set_projection(None)
    if kind == "ortho":
        a.set_camera(pt.look_at((6.0, 3.0, -15.0), (0.0, 0.0, 0.0), fov_y=60.0, aspect=W / H))
    pinhole = a.render_host(W, H, spp, 3, error=-1.0, want_stats=False)
    assert _digest(*pinhole[:3]) != _digest(*want[:3])
    f = pt.Frame(a, [0, 0, 0], W, H, flags=pt.FRAME_REHEARSE)   # made without one, given one afterwards
    f.render(0, spp, 3, error=-1.0)
    assert _digest(*f.read()) == _digest(*pinhole[:3])
    f.clear()
    f.set_camera(cam)
    f.set_projection(prj)
    f.render(0, spp, 3, error=-1.0)
    assert _digest(*f.read()) == _digest(*want[:3])
    f.close()
    g.close()


# ---- 5. every segment against the all-triangles loop ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_every_segment_of_projection_frames(gpu, models_dir, kind):
    v = pt.load_library(pt.VERIFY_LIB_PATH)
    shipped = pt.load_library(os.path.join(os.path.dirname(pt.VERIFY_LIB_PATH), "libpt_verify_shipped.so"))
    W, H, spp = 96, 64, 4
    cam, prj = _view(kind, W, H, "inside")
    out = []
    for lib in (v, shipped, None):
        if lib is not None:
            lib.pt_test_set_mutation(b"reset", 0.0)
        sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0, library=lib)
        sc.set_camera(cam)
        sc.set_projection(prj)
        r = sc.render_host(W, H, spp, 8, error=-1.0, want_stats=lib is not None)
        if lib is v:
            assert r[3]["verify_checked"] == r[3]["segments"] > W * H * spp // 2, r[3]
        if lib is not None:
            assert r[3]["verify_mismatches"] == 0, r[3]
        out.append(_digest(*r[:3]))
        sc.close()
    assert out[0] == out[1] == out[2]


# ---- 6. the temporal stage ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_temporal_stage_refuses_a_projection(gpu, models_dir, kind):
    W, H = 24, 16
    cam, prj = _view(kind, W, H, "outside")
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    sc.set_camera(cam)
    s, s2, c, _ = sc.render_host(W, H, 2, 3, error=-1.0, want_stats=False)
    history = pt.Temporal(sc, W, H)
    ses = pt.Session(sc, W, H)
    ses.render(0, 2, 3, error=-1.0)
    disp = pt.Display(ses)
    sc.set_projection(prj)
    with pytest.raises(pt.PtError) as e:
        history.push(s, s2, c)
    assert e.value.status == pt.PT_ERR_UNSUPPORTED
    with pytest.raises(pt.PtError) as e:
        disp.present(temporal=True)
    assert e.value.status == pt.PT_ERR_UNSUPPORTED
    assert disp.present()[0].shape == (H, W, 3)                    # without the stage the display shows the frame
    sc.set_projection(None)
    assert history.push(s, s2, c)["count"].sum() > 0               # and without the projection the history takes it
    disp.close()
    history.close()
    ses.close()
    sc.close()


# ---- 7. pixels wider than the envelope's slack ----------------------------------------------------------------------------------
def test_an_orthographic_launch_with_pixels_wider_than_a_scene_unit_is_refused(gpu, models_dir):
    """u and v reach 0.5 plus half a pixel at the left and the top edge; the envelope's slack covers |r_i| / W + |p_i| / H <= 1."""
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    sc.set_camera(pt.Camera.of((0.0, 0.0, -20.0), (32.0, 0.0, 0.0), (0.0, 8.0, 0.0), (0.0, 0.0, 1.0)))
    sc.set_projection("ortho")
    with pytest.raises(pt.PtError) as e:
        sc.render_host(24, 16, 1, 3, error=-1.0, want_stats=False)            # 32 / 24 > 1
    assert e.value.status == pt.PT_ERR_UNSUPPORTED
    s, s2, c, _ = sc.render_host(32, 16, 4, 8, error=-1.0, want_stats=False)  # 32 / 32 + 0 = 1: accepted
    assert c.sum() > 0
    sc.set_projection(None)
    sc.render_host(24, 16, 1, 3, error=-1.0, want_stats=False)                # the pinhole has one origin
    sc.close()
