"""What the direct-lighting tests share (tests/test_direct_host.py, tests/test_gpu_direct.py, tests/test_gpu_direct_cli.py): Tor.obj
with the lists its frames combine the switch with, a closed room with several lights of different size (one of them degenerate), the
small closed room of the agreement-in-expectation test, and the list of frames the GPU test renders.  The host test composes every one
of them on the CPU first and asserts that no pixel is tainted (the oracle's nan_seen), so the GPU test leaves no pixel out."""
import numpy as np

import oracle_lib as O
import rough_scenes as RS
import texture_scenes as TS
from glass_fuzz_scenes import _box, _quad

F32 = np.float32
GLASS_TORUS = RS.GLASS_TORUS
ROUGH_FLOOR = {2: 0.3}
TEX_WALL = {1: (TS.tex(3, 5, 9), 1)}

# 0 a white lamp, 1 the walls, 2 a glossy floor, 3 a red lamp, 4 a chalk box
LIGHTS_MTL = ("newmtl 0\nKe 3 3 3\nKd 1 1 1\nnewmtl 1\nNs 0\nKd 0.8 0.8 0.8\nnewmtl 2\nNs 300\nKs 0.7 0.7 0.7\nKd 0.6 0.6 0.9\n"
              "newmtl 3\nKe 1 0 0\nKd 2.0 0.4 0.2\nnewmtl 4\nNs 0\nKd 0.9 0.9 0.3\n")


def _write(d, name, mtl_name, mtl, tris):
    open(d + mtl_name, "w").write(mtl)
    p, q, r, _ = tris[0]
    n = np.cross(np.subtract(q, p), np.subtract(r, p))
    lines = ["mtllib " + mtl_name, "vn %.6f %.6f %.6f" % tuple(n / np.linalg.norm(n))]
    for i, (p, q, r, m) in enumerate(tris):
        lines += ["v %.6f %.6f %.6f" % tuple(v) for v in (p, q, r)] + ["usemtl %d" % m]
        lines.append("f %d//1 %d//1 %d//1" % (3 * i + 1, 3 * i + 2, 3 * i + 3) if i == 0 else "f %d %d %d" % (3 * i + 1, 3 * i + 2, 3 * i + 3))
    open(d + name, "w").write("\n".join(lines) + "\n")
    return O.Scene.load(d, name)


def lights_room(d, name="lights_room.obj", degenerate=True):
    """A closed room with a 6 x 6 lamp under the ceiling, a 1 x 2 red lamp on the left wall, a small white triangle on the far wall, a
    degenerate emissive triangle (three collinear vertices: no light; the oracle marks every ray that meets its NaN plane, so the
    frames that are compared bit for bit leave it out: degenerate=False), a chalk box that shadows the floor, and a glossy floor."""
    lo, hi = (-6.0, -6.0, -22.0), (6.0, 6.0, 6.0)
    tris = _box(lo, hi, 1, split=2, inward=True, faces=(0, 1, 3, 4, 5)) + _box(lo, hi, 2, split=2, inward=True, faces=(2,))
    tris += _quad((-3.0, 5.5, -9.0), (3.0, 5.5, -9.0), (3.0, 5.5, -3.0), (-3.0, 5.5, -3.0), 0)           # shines down
    tris += _quad((-5.5, -1.0, -8.0), (-5.5, 1.0, -8.0), (-5.5, 1.0, -7.0), (-5.5, -1.0, -7.0), 3)       # shines to +x
    tris += [((1.0, 1.0, 5.5), (2.0, 3.0, 5.5), (3.0, 1.0, 5.5), 0)]                                      # faces the eye (-z)
    if degenerate:
        tris += [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0), 0)]
    tris += _box((1.0, -5.5, -7.0), (3.5, -3.0, -4.0), 4)
    return _write(d, name, name.replace(".obj", ".mtl"), LIGHTS_MTL, tris)


# The agreement-in-expectation room: a small closed box around the eye's view with a LARGE lamp -- six tenths of the ceiling -- and grey
# walls, so that at -MRR 3 a good share of the paths of the run without light sampling reach the lamp.
SMALL_MTL = "newmtl 0\nKe 2 2 2\nKd 2.0 1.6 1.2\nnewmtl 1\nNs 0\nKd 0.7 0.7 0.7\nnewmtl 2\nNs 1000\nKs 0.9 0.9 0.9\nKd 0 0 0\n"


def small_room(d, name="small_room.obj", mirror=False):
    """mirror: the floor is a mirror (material 2: the glossy lobe alone in effect), so that paths reach the lamp by it after a diffuse step."""
    lo, hi = (-4.0, -4.0, -21.0), (4.0, 4.0, -10.0)
    tris = _box(lo, hi, 1, split=1, inward=True, faces=(0, 1, 3, 4, 5)) + _box(lo, hi, 2 if mirror else 1, split=1, inward=True, faces=(2,))
    tris += _quad((-3.0, 3.9, -20.0), (3.0, 3.9, -20.0), (3.0, 3.9, -11.0), (-3.0, 3.9, -11.0), 0)
    return _write(d, name, name.replace(".obj", ".mtl"), SMALL_MTL, tris)


# name -> (shape, spp, mrr, keywords): the frames of Tor.obj tests/test_gpu_direct.py renders, each composed on the CPU first
TOR_FRAMES = {
    "one_pixel_17x9": ((17, 9), 4, 4, dict()),
    "two_pixel_40x28": ((40, 28), 4, 4, dict()),
    "odd_41x29": ((41, 29), 3, 4, dict()),
    "tiles_72x20": ((72, 20), 3, 3, dict()),
    "stats": ((40, 28), 4, 4, dict(stats=True)),
    "smooth_normals": ((40, 28), 4, 4, dict(smooth=True)),
    "textured_wall": ((40, 28), 3, 4, dict(textures=TEX_WALL)),
    "glass_torus_rough_floor_stats": ((40, 28), 4, 4, dict(rough=ROUGH_FLOOR, glass=GLASS_TORUS, stats=True)),
    "adaptive": ((40, 28), 16, 3, dict(error=0.02)),
}
VIEWS = ["camera", "lens", "shutter", "fisheye"]
# name -> (shape, spp, mrr, tile_width, keywords): frames of Tor.obj rendered through the test-hook library with the planner's tile_width
# override (pt_launch_plan.hpp: Overrides), which a frame of this size needs to reach the kernels of a 1080p frame: 1 = the 8 x 8 kernel,
# 2 = two pixels per lane over 16 x 8 tiles, and with error >= 0 the batch kernel over them, 3 = the batch kernel over 32 x 8 tiles.
# 48 x 40 is whole tiles of every width but 32; 50 x 43 has partial tiles in both directions.
FORM_FRAMES = {
    "narrow_8x8": ((24, 16), 3, 4, 1, dict()),
    "wide_16x8": ((48, 40), 3, 4, 2, dict()),
    "wide_16x8_partial": ((50, 43), 3, 4, 2, dict()),
    "wide_16x8_smooth_glass_rough": ((48, 40), 3, 4, 2, dict(smooth=True, rough=ROUGH_FLOOR, glass=GLASS_TORUS)),
    "batch_16x8": ((48, 40), 16, 3, 2, dict(error=0.02)),
    "batch_16x8_partial_textured": ((50, 43), 16, 3, 2, dict(error=0.02, textures=TEX_WALL)),
    "batch_32x8": ((50, 43), 16, 3, 3, dict(error=0.02)),
    "batch_32x8_smooth_glass_rough": ((64, 16), 16, 4, 3, dict(error=0.05, smooth=True, rough=ROUGH_FLOOR, glass=GLASS_TORUS)),
}
# (view, tile_width, error): the camera twins of the same three forms
FORM_VIEWS = [("camera", 2, -1.0), ("lens", 2, 0.02), ("shutter", 3, 0.02), ("fisheye", 2, -1.0)]
FORM_VIEW_FRAME = ((48, 24), 14, 3)
# (tile_width, error) of the box tree's batch forms, on every fifth pixel of this frame
BOX_FORMS = [(2, 0.02), (3, 0.02)]
BOX_FRAME = ((48, 24), 14, 3)
ROOM_FRAME = ((40, 28), 4, 4)
