"""The configurable camera on the GPU (pt_hip.h: pt_camera; pt_kernels.hip: the camera twins, integrate_kernel<..., ADAPT | 1>).

The oracle knows only the reference's fixed camera, so the twins are tied to it in three ways that need no second oracle:
identity (the reference camera set explicitly runs the twins and must give the camera-free frame -- itself oracle-exact -- bit
for bit), exact mirrors (a scene mirrored as text, seen through the mirrored camera, gives the same frame pixel for pixel at
-MRR 1), and the verification builds (every segment of frames seen from arbitrary cameras against the all-triangles loop).
The geometry of the view (axes, signs, handedness, aspect) is checked independently of the kernel with probe rays through
pt_trace_rays_host."""
import hashlib
import importlib
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = pt.REFERENCE_CAMERA


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


def _pair(d, name, sky=None):
    """(camera-free scene, the same model with the reference camera set explicitly)."""
    a = pt.Scene.load_obj(d, name, device=0)
    b = pt.Scene.load_obj(d, name, device=0)
    if sky:
        a.set_skybox(sky)
        b.set_skybox(sky)
    b.set_camera(REF)
    return a, b


# ---- 1. identity: the reference camera through the twins is the camera-free frame ---------------------------------------
@pytest.mark.parametrize("W,H,spp,err,stats", [
    (1920, 1080, 4, -1.0, False),     # two pixels per lane (16 x 8 tiles)
    (256, 256, 8, -1.0, False),       # one pixel per lane (8 x 8 tiles: too few wide tiles for the chip)
    (1920, 1080, 24, 0.001, False),   # adaptive batches over 32 x 8 tiles
    (1280, 720, 24, 0.001, False),    # ... over 16 x 8 tiles
    (640, 360, 8, 0.001, True),       # a statistics launch
], ids=["wide", "narrow", "adapt32", "adapt16", "stats"])
def test_reference_camera_twin_is_bit_identical_on_tor(gpu, models_dir, W, H, spp, err, stats):
    a, b = _pair(models_dir, "Tor.obj")
    ra = a.render_host(W, H, spp, 8, error=err, want_stats=stats)
    rb = b.render_host(W, H, spp, 8, error=err, want_stats=stats)
    assert _digest(*ra[:3]) == _digest(*rb[:3])
    assert ra[2].sum() > 0
    if stats:
        for k in ("samples_traced", "segments", "contributing", "misses", "exact_tests"):
            assert ra[3][k] == rb[3][k], k


@pytest.mark.parametrize("err", [-1.0, 0.001])
def test_reference_camera_twin_is_bit_identical_on_the_box_tree(gpu, tmp_path, err):
    d, name = _replica(tmp_path, 64)
    a, b = _pair(d, name)
    for W, H in ((960, 540), (1920, 1080)):
        ra = a.render_host(W, H, 12, 8, error=err, want_stats=False)
        rb = b.render_host(W, H, 12, 8, error=err, want_stats=False)
        assert _digest(*ra[:3]) == _digest(*rb[:3]), (W, H, err)
    assert b.render_host(64, 64, 2, 8)[3]["segments"] == a.render_host(64, 64, 2, 8)[3]["segments"]   # statistics twin


def test_reference_camera_twin_is_bit_identical_under_a_skybox(gpu, tmp_path):
    d, name = _open_scene(tmp_path)
    a, b = _pair(d, name, sky=d + "sky.bmp")
    for mrr in (1, 3, 8):
        for stats in (False, True):
            ra = a.render_host(480, 270, 16, mrr, error=-1.0, want_stats=stats)
            rb = b.render_host(480, 270, 16, mrr, error=-1.0, want_stats=stats)
            assert _digest(*ra[:3]) == _digest(*rb[:3]), (mrr, stats)


def test_reference_camera_through_a_rehearsed_three_band_frame(gpu, models_dir):
    W, H, spp = 640, 360, 8
    a = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    want = a.render_host(W, H, spp, 8, error=-1.0, want_stats=False)
    f = pt.Frame(a, [0, 0, 0], W, H, flags=pt.FRAME_REHEARSE)
    f.set_camera(REF)
    f.render(0, spp, 8, error=-1.0)
    assert _digest(*f.read()) == _digest(*want[:3])
    # a camera set on the scene before the frame is made is inherited by the frame's copies
    cam = pt.look_at((3, 2, -15), (0, 0, 0), fov_y=45.0, aspect=W / H)
    a.set_camera(cam)
    one = a.render_host(W, H, spp, 8, error=-1.0, want_stats=False)
    assert _digest(*one[:3]) != _digest(*want[:3])
    g = pt.Frame(a, [0, 0, 0], W, H, flags=pt.FRAME_REHEARSE)
    g.render(0, spp, 8, error=-1.0)
    assert _digest(*g.read()) == _digest(*one[:3])
    f.clear()
    f.set_camera(cam)
    f.render(0, spp, 8, error=-1.0)
    assert _digest(*f.read()) == _digest(*one[:3])
    f.close()
    g.close()


# ---- 2. exact mirrors ------------------------------------------------------------------------------------------------------
def _negate(tok):
    if float(tok) == 0.0:
        return tok.lstrip("-")          # no signed zero appears
    return tok[1:] if tok.startswith("-") else "-" + tok


def _mirror(src_dir, name, out_dir, axis):
    """The OBJ with coordinate `axis` of every `v` and `vn` negated as text (exact); the MTL files are copied."""
    os.makedirs(out_dir, exist_ok=True)
    out = []
    for line in open(os.path.join(src_dir, name)).read().split("\n"):
        t = line.split()
        if t and t[0] in ("v", "vn") and len(t) >= 4:
            t[1 + axis] = _negate(t[1 + axis])
            line = " ".join(t)
        out.append(line)
    open(os.path.join(out_dir, name), "w").write("\n".join(out))
    for f in os.listdir(src_dir):
        if f.endswith(".mtl"):
            shutil.copy(os.path.join(src_dir, f), out_dir)


MIRROR_CAMERAS = {0: ((0, 0, -20), (-1, 0, 0), (0, 1, 0), (0, 0, 1)),     # x mirrored: right = (-1, 0, 0)
                  2: ((0, 0, 20), (1, 0, 0), (0, 1, 0), (0, 0, -1))}      # z mirrored: eye (0, 0, 20) looking down -z


@pytest.mark.parametrize("scene", ["tor", "x64"])
@pytest.mark.parametrize("axis", [0, 2], ids=["x", "z"])
def test_mirrored_scene_through_the_mirrored_camera_is_exact(gpu, tmp_path, models_dir, scene, axis):
    src_dir, name = (models_dir, "Tor.obj") if scene == "tor" else _replica(tmp_path, 64)
    mdir = os.path.join(str(tmp_path), "mirror") + "/"
    _mirror(src_dir, name, mdir, axis)
    a = pt.Scene.load_obj(src_dir, name, device=0)
    m = pt.Scene.load_obj(mdir, name, device=0)
    m.set_camera(MIRROR_CAMERAS[axis])
    W, H = 640, 360
    for err, spp in ((-1.0, 16), (0.001, 32)):
        s, s2, c, _ = a.render_host(W, H, spp, 1, error=err, want_stats=False)
        ms, ms2, mc, _ = m.render_host(W, H, spp, 1, error=err, want_stats=False)
        assert c.sum() > 0
        assert np.array_equal(c, mc), (err, int((c != mc).sum()))
        assert np.array_equal(_bits(s), _bits(ms)) and np.array_equal(_bits(s2), _bits(ms2)), err


def test_x_mirror_at_full_path_length_agrees_in_distribution(gpu, tmp_path, models_dir):
    """-MRR 8: the diffuse lobe is symmetric in x only in distribution.  Binned 16 x 16 means, z-scores from sum2."""
    mdir = os.path.join(str(tmp_path), "mirror") + "/"
    _mirror(models_dir, "Tor.obj", mdir, 0)
    a = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    m = pt.Scene.load_obj(mdir, "Tor.obj", device=0)
    m.set_camera(MIRROR_CAMERAS[0])
    W, H, spp = 240, 135, 64
    z2 = []
    outs = []
    for sc, seed in ((a, 42), (m, 4242)):
        s, s2, c, _ = sc.render_host(W, H, spp, 8, error=-1.0, seed=seed, want_stats=False)
        mean = s.reshape(H, W, 3).astype(np.float64) / spp       # every path counts: one that contributes nothing adds 0
        var = s2.reshape(H, W, 3).astype(np.float64) / spp - mean * mean
        outs.append((mean, np.maximum(var, 0.0) / spp))         # a pixel's mean and the variance of that mean
    B = 16
    (ma, va), (mb, vb) = outs
    for by in range(H // B):
        for bx in range(W // B):
            sl = (slice(by * B, (by + 1) * B), slice(bx * B, (bx + 1) * B))
            da = ma[sl].mean((0, 1)) - mb[sl].mean((0, 1))
            var = (va[sl].sum((0, 1)) + vb[sl].sum((0, 1))) / (B * B) ** 2
            ok = var > 0
            z2 += list((da * da / np.where(ok, var, 1.0))[ok])
    z2 = np.array(z2)
    assert len(z2) > 300
    assert np.sqrt(z2.max()) < 6.0, np.sqrt(z2.max())
    assert 0.7 <= z2.mean() <= 1.3, z2.mean()


# ---- 4. arbitrary cameras: every segment against the all-triangles loop ----------------------------------------------------
@pytest.fixture(scope="module")
def vlibs(gpu):
    v = pt.load_library(pt.VERIFY_LIB_PATH)
    v.pt_test_set_mutation(b"reset", 0.0)
    shipped = pt.load_library(os.path.join(os.path.dirname(pt.VERIFY_LIB_PATH), "libpt_verify_shipped.so"))
    shipped.pt_test_set_mutation(b"reset", 0.0)
    return v, shipped


def _cameras(W, H):
    return {
        "corner": (pt.look_at((4.0, -3.0, -6.0), (-9.5, 9.5, 9.5), (0.1, 1.0, 0.0), fov_y=70.0, aspect=W / H), 512, 512),
        "behind_back_wall": (pt.look_at((1.0, 0.5, -35.0), (0.0, 0.0, 0.0), fov_y=40.0), 512, 512),
        "far": (pt.look_at((0.0, 0.0, -200.0), (0.0, 0.0, 0.0), fov_y=8.0), 512, 512),
        "down_from_ceiling": (pt.look_at((0.5, 9.0, 0.3), (0.0, -10.0, 0.0), (0.0, 0.0, 1.0), fov_y=80.0), 512, 512),
        "aspect_640x360": (pt.look_at((-5.0, 2.0, -18.0), (1.0, -1.0, 2.0), fov_y=50.0, aspect=640 / 360), 640, 360),
    }


@pytest.mark.parametrize("scene", ["tor", "x64"])
def test_every_segment_of_frames_from_arbitrary_cameras(tmp_path, models_dir, vlibs, scene):
    v, shipped = vlibs
    d, name = (models_dir, "Tor.obj") if scene == "tor" else _replica(tmp_path, 64)
    for label, (cam, W, H) in _cameras(512, 512).items():
        sv = pt.Scene.load_obj(d, name, device=0, library=v)
        sv.set_camera(cam)
        s, s2, c, st = sv.render_host(W, H, 16, 8, error=-1.0)
        assert st["verify_checked"] == st["segments"] > W * H * 16, (label, st)
        assert st["verify_mismatches"] == 0, (label, st)
        ss = pt.Scene.load_obj(d, name, device=0, library=shipped)
        ss.set_camera(cam)
        q = ss.render_host(W, H, 16, 8, error=-1.0)
        assert q[3]["verify_mismatches"] == 0, (label, q[3])
        g = pt.Scene.load_obj(d, name, device=0)
        g.set_camera(cam)
        r = g.render_host(W, H, 16, 8, error=-1.0, want_stats=False)
        assert _digest(*r[:3]) == _digest(s, s2, c) == _digest(*q[:3]), label
        for x in (sv, ss, g):
            x.close()


def test_every_segment_under_a_skybox_from_an_arbitrary_camera(tmp_path, vlibs):
    v, shipped = vlibs
    d, name = _open_scene(tmp_path)
    cam = pt.look_at((6.0, 3.0, 25.0), (0.0, 0.0, 0.0), fov_y=65.0, aspect=1.0)   # from outside the open side of the room
    sv = pt.Scene.load_obj(d, name, device=0, library=v)
    sv.set_skybox(d + "sky.bmp")
    sv.set_camera(cam)
    s, s2, c, st = sv.render_host(512, 512, 16, 8, error=-1.0)
    assert st["verify_checked"] == st["segments"] > 0 and st["verify_mismatches"] == 0, st
    assert st["misses"] > 0
    g = pt.Scene.load_obj(d, name, device=0)
    g.set_skybox(d + "sky.bmp")
    g.set_camera(cam)
    assert _digest(*g.render_host(512, 512, 16, 8, error=-1.0, want_stats=False)[:3]) == _digest(s, s2, c)


# ---- 5. the geometry of the view, independently of the kernel --------------------------------------------------------------
def test_pixels_see_what_probe_rays_through_their_footprint_see(gpu, models_dir):
    W, H, spp = 128, 96, 64
    scene = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    tri, mat = scene.triangles()
    emis = mat == 0
    centre = tri[emis, 4:13].reshape(-1, 3).mean(0).astype(np.float64)
    eye = centre + np.array([-3.0, -4.5, -2.5])          # inside the room, below and to the side of the ceiling emitter
    cam = pt.look_at(eye, centre + np.array([0.3, 0.0, 0.2]), fov_y=35.0, aspect=1.6)
    scene.set_camera(cam)
    s, s2, c, _ = scene.render_host(W, H, spp, 1, error=-1.0, want_stats=False)
    o, r, u, f = cam.as_array().astype(np.float64)
    js = np.array([-0.48, 0.0, 0.48])   # the jitter lies in (-0.5, 0.5): main.cpp:92
    ys, xs, jy, jx = np.meshgrid(np.arange(H), np.arange(W), js, js, indexing="ij")
    uu = (xs + jx) / W - 0.5
    vv = -(ys + jy) / H + 0.5
    d = uu[..., None] * r + vv[..., None] * u + f
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32).reshape(-1, 3)
    origins = np.broadcast_to(o.astype(np.float32), d.shape)
    idx, t = scene.trace_rays(origins, d)
    hit_emitter = ((idx >= 0) & emis[np.maximum(idx, 0)]).reshape(H, W, 9)
    all_e, none_e = hit_emitter.all(-1), ~hit_emitter.any(-1)
    cnt = c.reshape(H, W)
    assert all_e.sum() > 0.05 * W * H, all_e.sum()          # the view really contains the emitter
    assert np.array_equal(cnt[all_e], np.full(all_e.sum(), spp)), int((cnt[all_e] != spp).sum())
    assert not cnt[none_e].any(), int((cnt[none_e] != 0).sum())
    assert (all_e | none_e).sum() >= 0.9 * W * H, (all_e | none_e).sum() / (W * H)


# ---- 6. pt_render -----------------------------------------------------------------------------------------------------------
def test_pt_render_with_the_reference_camera_spelled_out_writes_the_same_bmp(gpu, tmp_path):
    exe = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
    base = [exe, "--W", "320", "--H", "200", "-RPP", "16", "-MRR", "8", "-MODEL_PATH", os.path.join(ROOT, "models") + "/", "-QUIET", "1"]
    outs = {}
    for label, extra in (("plain", []), ("ref", ["-EYE", "0,0,-20", "-LOOKAT", "0,0,0", "-UP", "0,1,0", "-FOV", "53.13010235415598", "-ASPECT", "0"]),
                         ("other", ["-EYE", "2,1,-16", "-ASPECT", "1.6"]), ("bands", ["-EYE", "2,1,-16", "-ASPECT", "1.6", "-GPUS", "3", "-REHEARSE", "1"])):
        path = os.path.join(str(tmp_path), label + ".bmp")
        p = subprocess.run(base + extra + ["-OUT", path], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (label, p.stderr)
        outs[label] = open(path, "rb").read()
    assert outs["plain"] == outs["ref"]
    assert outs["other"] != outs["plain"]
    assert outs["bands"] == outs["other"]
