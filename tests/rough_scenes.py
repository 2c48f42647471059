"""What the rough-specular tests share (tests/test_rough_host.py, tests/test_gpu_rough.py, tests/test_gpu_rough_cli.py): Tor.obj with
its roughness lists, a closed room whose floor is nearly all glossy lobe (Ns 900) written with an MTL that carries Pr lines, and the
list of frames the GPU test renders.  The host test composes every one of them on the CPU first and asserts that no pixel is tainted
(the oracle's nan_seen), so the GPU test leaves no pixel out."""
import numpy as np

import oracle_lib as O
import smooth_scenes as SS
import texture_scenes as TS
from glass_fuzz_scenes import EMITTER, _box

F32 = np.float32
ROUGH_TORUS = {4: 0.3}
ROUGH_ALL = {1: 0.08, 2: 1.0, 3: 2.0 ** -10, 4: 0.3}
GLASS_TORUS = SS.GLASS_TORUS
TEX_TORUS = {4: (TS.tex(3, 5, 9), 1)}

# 0 the emitter, 1 the walls, 2 the floor (the glossy lobe 9 times in 10), 3 a glossy box whose Pr lies above the range, 4 a chalk box
# whose Pr -ROUGH mtl passes over (no glossy lobe), 5 a glossy box without a Pr line
ROOM_MTL = ("newmtl 0\nKe 3 3 3\nKd 1 1 1\nnewmtl 1\nNs 0\nKd 0.8 0.8 0.8\nnewmtl 2\nNs 900\nKs 0.8 0.8 0.8\nKd 0.5 0.5 0.5\nPr 0.25\n"
            "newmtl 3\nNs 300\nKs 0.7 0.7 0.7\nKd 0.6 0.6 0.9\nPr 1.5\nnewmtl 4\nNs 0\nKd 0.9 0.3 0.3\nPr 0.4\n"
            "newmtl 5\nNs 500\nKs 0.9 0.6 0.3\nKd 0.2 0.2 0.2\n")
ROOM_PR = [-1.0, -1.0, 0.25, 1.5, 0.4, -1.0]
ROOM_MTL_LIST = {2: 0.25, 3: 1.0}                     # what -ROUGH mtl makes of it
ROOM_ROUGH = {2: 0.25, 5: 0.05}


def room(d, name="rough_room.obj"):
    """The room written into directory d: the oracle's scene."""
    lo, hi = (-6.0, -6.0, -22.0), (6.0, 6.0, 6.0)
    tris = _box(lo, hi, 1, split=2, inward=True, faces=(0, 1, 3, 4, 5)) + _box(lo, hi, 2, split=2, inward=True, faces=(2,)) + EMITTER
    tris += _box((-4.0, -5.5, -9.0), (-1.0, -3.5, -6.0), 3) + _box((1.0, -5.5, -7.0), (3.5, -4.0, -4.0), 4) + _box((-0.5, -5.5, -3.0), (2.0, -2.0, -1.0), 5)
    open(d + "rough_room.mtl", "w").write(ROOM_MTL)
    p, q, r, _ = tris[0]
    n = np.cross(np.subtract(q, p), np.subtract(r, p))
    lines = ["mtllib rough_room.mtl", "vn %.6f %.6f %.6f" % tuple(n / np.linalg.norm(n))]
    for i, (p, q, r, m) in enumerate(tris):
        lines += ["v %.6f %.6f %.6f" % tuple(v) for v in (p, q, r)] + ["usemtl %d" % m]
        lines.append("f %d//1 %d//1 %d//1" % (3 * i + 1, 3 * i + 2, 3 * i + 3) if i == 0 else "f %d %d %d" % (3 * i + 1, 3 * i + 2, 3 * i + 3))
    open(d + name, "w").write("\n".join(lines) + "\n")
    return O.Scene.load(d, name)


# name -> (shape, spp, mrr, keywords): the frames of Tor.obj tests/test_gpu_rough.py renders, each composed on the CPU first
TOR_FRAMES = {
    "one_pixel_17x9": ((17, 9), 4, 8, dict(rough=ROUGH_TORUS)),
    "two_pixel_40x28": ((40, 28), 4, 8, dict(rough=ROUGH_ALL)),
    "odd_41x29": ((41, 29), 4, 8, dict(rough=ROUGH_ALL)),
    "tiles_72x20": ((72, 20), 4, 3, dict(rough=ROUGH_ALL)),
    "stats": ((40, 28), 4, 8, dict(rough=ROUGH_ALL, stats=True)),
    "smooth_normals": ((40, 28), 8, 8, dict(rough=ROUGH_ALL, smooth=True)),
    "textured_rough_torus": ((40, 28), 4, 8, dict(rough=ROUGH_TORUS, textures=TEX_TORUS)),
    "glass_torus_rough_walls_stats": ((40, 28), 4, 8, dict(rough={1: 0.2, 2: 0.5, 3: 0.05}, glass=GLASS_TORUS, stats=True)),
    "adaptive": ((40, 28), 16, 3, dict(rough=ROUGH_ALL, error=0.02)),
}
VIEWS = ["camera", "lens", "shutter", "fisheye"]
ROOM_FRAME = ((40, 28), 4, 8)
