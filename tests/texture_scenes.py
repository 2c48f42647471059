"""What the texture tests share (tests/test_texture_host.py, tests/test_gpu_texture.py, tests/test_gpu_texture_cli.py): the scenes --
Tor.obj, the open Tor scene, the box-tree scene and the closed room made from arrays, each with its planar coordinates -- the
procedural textures and the texture lists of the frames, the BMP writer, the views, and the pixels compared.  The geometry of the room
is tests/glass_fuzz_scenes.py's (a shared module too).  Nothing here needs a GPU: the host test composes every scene's frame on the
CPU and asserts the share of tainted pixels, so that a breach of the cap does not look like a GPU failure."""
import os
import struct
import sys

import numpy as np

import oracle_lib as O
import texture_restatement as T
from glass_fuzz_scenes import MTL, _box, _room, _write_obj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
TAINT_CAP = 0.02
VIEWS = ["free", "camera", "lens", "shutter", "lens_shutter", "ortho", "fisheye", "equirect"]
CAM = dict(eye=(4.0, 3.0, -19.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
END = dict(eye=(3.0, 4.0, -18.0), target=(0.5, 0.0, 0.0), up=(0.0, 1.0, 0.0))


def all_pixels(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.ravel(), ys.ravel()], 1)


def env_map(seed):
    return np.random.default_rng(seed).uniform(0.05, 2.0, (8, 8, 3)).astype(F32)


def tex(w, h, seed, zero_channel=None):
    t = np.random.default_rng(seed).uniform(0.05, 1.5, (h, w, 3)).astype(F32)
    if zero_channel is not None:
        t[:, :, zero_channel] = 0
    return t


def write_bmp(path, bgr):
    h, w = bgr.shape[:2]
    pad = (4 - 3 * w % 4) % 4
    rows = b"".join(bgr[h - 1 - y].tobytes() + b"\0" * pad for y in range(h))
    hdr = struct.pack("<2sIHHI", b"BM", 54 + len(rows), 0, 0, 54) + struct.pack("<IiiHHIIiiII", 40, w, h, 1, 24, 0, len(rows), 2835, 2835, 0, 0)
    open(path, "wb").write(hdr + rows)


def planar_uv(tri14, scale=0.11, shift=(0.3, -0.2)):
    """Coordinates from the vertices' positions: u along x + z, v along y - z (runs outside [0, 1) and goes negative)."""
    v = np.asarray(tri14, F32)[:, 4:13].reshape(-1, 3, 3)
    return np.stack([(v[:, :, 0] + v[:, :, 2]) * F32(scale) + F32(shift[0]), (v[:, :, 1] - v[:, :, 2]) * F32(scale) + F32(shift[1])], -1).astype(F32)


def set_view(pt, scene, view, w, h):
    """Sets `view` on the handle `scene` of library module `pt` (None: sets nothing) and returns the composition's keywords."""
    if view == "free":
        return {}
    cam = pt.look_at(CAM["eye"], CAM["target"], CAM["up"], fov_y=60.0, aspect=w / h)
    kw = dict(camera=cam.as_array())
    end = prj = lens = None
    if view in ("lens", "lens_shutter"):
        lens = kw["lens"] = (0.3, 18.0)
    if view in ("shutter", "lens_shutter"):
        end = pt.look_at(END["eye"], END["target"], END["up"], fov_y=60.0, aspect=w / h)
        kw["motion_end"] = end.as_array()
    if view in ("ortho", "fisheye", "equirect"):
        if view == "ortho":
            cam = pt.ortho_camera(CAM["eye"], CAM["target"], CAM["up"], view_height=12.0, aspect=w / h)
            kw["camera"] = cam.as_array()
            prj = pt.projection("ortho")
        else:
            prj = pt.projection(view, fov_y=170.0, aspect=w / h) if view == "fisheye" else pt.projection("equirect")
        kw["projection"] = (prj.kind, prj.span_x, prj.span_y)
    if scene is not None:
        scene.set_camera(cam)
        if lens:
            scene.set_lens(*lens)
        if end is not None:
            scene.set_camera_motion(end)
        if prj is not None:
            scene.set_projection(prj)
    return kw


# ---- the scenes: each returns what both sides are made from ---------------------------------------------------------------------------
def tor(models_dir):
    """(oracle scene, coordinates) of Tor.obj with planar coordinates."""
    osc = O.Scene.load(models_dir, "Tor.obj")
    return osc, planar_uv(osc.triangles()[0])


def open_tor(d):
    """The open Tor scene written into directory d (Open.obj, sky.bmp): (oracle scene, coordinates)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_open_scene as MO
    MO.generate(os.path.join(ROOT, "models"), d, name="Open.obj")
    osc = O.Scene.load(d, "Open.obj")
    return osc, planar_uv(osc.triangles()[0])


def box_tree(d):
    """Tor.obj four times (TorX4.obj in d), above BIG_SCENE_TRIANGLES: (oracle scene, coordinates, texture list)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_replicated_scene as MR
    MR.generate(os.path.join(ROOT, "models"), d, "TorX4.obj", 4)
    osc = O.Scene.load(d, "TorX4.obj")
    textures = {m: (tex(3, 5, 20 + m), m % 2) for m in range(osc.n_mat) if m % 5 in (1, 4)}      # every copy's walls and torus
    return osc, planar_uv(osc.triangles()[0]), textures


def room(d):
    """The closed room of the glass tests (material 0 the emitter, 1 the walls) with a box of material 3 in it, and one more triangle
    of material 2 whose vertices are collinear (its stored plane is a valid one, as an OBJ's vn gives: the oracle sees no NaN).
    Planar coordinates that run outside [0, 1) and go negative; one wall triangle at coordinates of 2^30.
    Returns (triangle records, their materials, the materials, oracle scene, coordinates)."""
    _write_obj(d, "room.obj", _room() + _box((-2.5, -4.0, -8.0), (1.5, 0.0, -4.0), 3))
    parsed = O.Scene.load(d, "room.obj")
    tri, tri_mat = parsed.triangles()
    thin = np.zeros(14, F32)
    thin[0:4] = [0.0, 0.0, -1.0, -3.0]                   # the plane z = -3, facing the eye
    thin[4:13] = [-3.0, 1.0, -3.0, 0.0, 2.0, -3.0, 3.0, 3.0, -3.0]
    tri, tri_mat = np.vstack([tri, thin[None]]).astype(F32), np.append(tri_mat, 2).astype(np.int32)
    osc = O.Scene.from_arrays(tri, tri_mat, parsed.materials())
    uv = planar_uv(tri, scale=0.37, shift=(-1.3, 0.6))
    assert uv.min() < -1 and uv.max() > 2
    uv[3] = [[2.0 ** 30, -2.0 ** 30], [2.0 ** 30 + 128, 2.0 ** 30], [-2.0 ** 30, 2.0 ** 30 + 256]]
    return tri, tri_mat, parsed.materials(), osc, uv


def room_textures(w, h, filt):
    return {1: (tex(w, h, 11), filt), 2: (tex(w, h, 12, zero_channel=2), filt), 3: (tex(3, 5, 13), 1 - filt), 0: (tex(w, h, 14), filt)}


def sliver_scene():
    """Triangle records for the record test: slivers (aspect up to 10^6), far from the origin and near it, and one collinear triangle."""
    rng = np.random.default_rng(17)
    tri = np.zeros((41, 14), F32)
    for i in range(40):
        a = rng.uniform(-20, 20, 3)
        e1 = rng.normal(size=3) * 10.0 ** rng.uniform(-3, 1)
        e2 = e1 * rng.uniform(0.2, 2.0) + rng.normal(size=3) * np.linalg.norm(e1) * 10.0 ** rng.uniform(-6, 0)
        tri[i, 4:13] = np.concatenate([a, a + e1, a + e2])
    tri[40, 4:13] = [-3.0, 1.0, -3.0, 0.0, 2.0, -3.0, 3.0, 3.0, -3.0]
    tri[:, 0:4] = [0.0, 0.0, -1.0, 0.0]
    return tri


TOR_CASES = {"m1": {1: (tex(3, 5, 1), T.BILINEAR)}, "m2": {2: (tex(64, 64, 2), T.NEAREST)}, "m3": {3: (tex(1, 1, 3), T.BILINEAR)},
             "m4": {4: (tex(64, 64, 4), T.BILINEAR)}, "emitter": {0: (tex(3, 5, 5), T.NEAREST)},
             "m1_m4": {1: (tex(64, 64, 6, zero_channel=1), T.BILINEAR), 4: (tex(3, 5, 7), T.NEAREST)}}
TOR_TWO = TOR_CASES["m1_m4"]
