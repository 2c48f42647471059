"""What the environment-sampling tests share (tests/test_envdirect_host.py, tests/test_gpu_envdirect.py, tests/test_gpu_envdirect_cli.py):
the scenes -- Tor.obj without its back wall, a small room without ceiling and floor with one lamp on its left wall, and the same room with no
emitter -- and the environment maps: the smallest, one whose size is no power of two, a one-texel sun on a dim and on a black sky, and
one larger than the table's 256 cells a side."""
import numpy as np

import direct_scenes as DS
import texture_scenes as TS
from glass_fuzz_scenes import _box, _quad

F32 = np.float32


def open_tor(d):
    """(oracle scene, coordinates) of Open.obj in d."""
    return TS.open_tor(d)


# 0 the lamp -- bright enough to matter beside the sky --, 1 the walls
ROOM_MTL = "newmtl 0\nKe 2 2 2\nKd 14.0 12.0 10.0\nnewmtl 1\nNs 0\nKd 0.7 0.7 0.7\n"


def open_room(d, lamp=True, name=None):
    """Four walls of 8 x 8 x 11 units around the reference eye's view, open at the top and at the bottom, so that both hemispheres of the
    environment reach them; lamp: a 2 x 3 emitter on the left wall."""
    name = name or ("lamp_room.obj" if lamp else "dark_room.obj")
    lo, hi = (-4.0, -4.0, -21.0), (4.0, 4.0, -10.0)
    tris = _box(lo, hi, 1, split=1, inward=True, faces=(0, 1, 4, 5))
    if lamp:
        tris += _quad((-3.9, -1.0, -17.0), (-3.9, 1.0, -17.0), (-3.9, 1.0, -14.0), (-3.9, -1.0, -14.0), 0)       # shines to +x
    return DS._write(d, name, name.replace(".obj", ".mtl"), ROOM_MTL, tris)


def random_map(n, seed):
    return np.random.default_rng(seed).uniform(0.05, 2.0, (n, n, 3)).astype(F32)


def sun_map(n=32, sky=0.2, sun=5000.0, at=(18, 24)):
    """A sky of `sky` with one texel of `sun` in the upper hemisphere (texel (i, j) = m[j, i])."""
    m = np.full((n, n, 3), sky, F32)
    m[at[1], at[0]] = sun
    return m


def soft_map(seed=5):
    """The agreement test's map: 8 x 8, a bright patch in the upper hemisphere towards +x (it lights the left wall, which does not face
    along z, at an angle where n . w and |w.z| differ) and one round the lower pole (the square's corner, where
    the fold matters) on a dim random sky -- the escape-only estimator still converges on it."""
    m = np.random.default_rng(seed).uniform(0.05, 0.4, (8, 8, 3)).astype(F32)
    m[4:6, 5] = (9.0, 7.5, 6.0)
    m[0:2, 0:2] = (4.0, 6.0, 5.0)
    return m


MAPS = {
    "n8": lambda: random_map(8, 1),
    "n12": lambda: random_map(12, 2),
    "sun32": lambda: sun_map(),
    "sun32_black": lambda: sun_map(sky=0.0),
    "n512": lambda: np.maximum(random_map(512, 3), sun_map(512, 0.0, 800.0, (300, 380))),
}
# name -> (shape, spp, mrr, keywords): the frames of the open Tor scene under the sun map
TOR_FRAMES = {
    "one_pixel_17x9": ((17, 9), 4, 4, dict()),
    "two_pixel_40x28": ((40, 28), 4, 4, dict()),
    "odd_41x29": ((41, 29), 3, 4, dict()),
    "stats": ((40, 28), 4, 4, dict(stats=True)),
    "adaptive": ((40, 28), 16, 3, dict(error=0.02)),
    "glass_rough_smooth_textured": ((40, 28), 3, 4, dict(rough=DS.ROUGH_FLOOR, glass=DS.GLASS_TORUS, smooth=True, textures=DS.TEX_WALL)),
}
VIEWS = DS.VIEWS
ROOM_FRAME = ((40, 28), 4, 4)
