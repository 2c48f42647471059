"""What the smooth-shading tests share (tests/test_smooth_host.py, tests/test_gpu_smooth.py): the scenes of tests/texture_scenes.py with
generated shading normals, and the list of frames the GPU test renders.  The host test composes every one of them on the CPU first
and asserts that no pixel is tainted (the oracle's nan_seen), so the GPU test leaves no pixel out."""
import os
import sys

import numpy as np

import texture_restatement as T
import texture_scenes as TS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from make_smooth_scene import numpy_normals  # noqa: E402  (the generator restated in numpy: the tool's, so that the tool needs nothing of tests/)

F32 = np.float32
GLASS_TORUS = {4: (1.5, (0.9, 1.0, 0.8))}
TEX_WALLS = {1: (TS.tex(3, 5, 6), T.BILINEAR)}


def tor_normals(osc, crease=60.0):
    return numpy_normals(osc.triangles()[0][:, 4:13], crease)


# name -> (shape, spp, mrr, keywords): the frames of Tor.obj tests/test_gpu_smooth.py renders, each composed on the CPU first
TOR_FRAMES = {
    "one_pixel_17x9": ((17, 9), 4, 8, {}),
    "two_pixel_40x28": ((40, 28), 4, 8, {}),
    "tiles_72x20": ((72, 20), 4, 3, {}),
    "stats": ((40, 28), 4, 8, dict(stats=True)),
    "glass": ((40, 28), 8, 8, dict(glass=GLASS_TORUS)),
    "textures": ((40, 28), 4, 8, dict(textures=TEX_WALLS)),
    "glass_textures_stats": ((40, 28), 4, 8, dict(glass=GLASS_TORUS, textures=TEX_WALLS, stats=True)),
    "adaptive": ((40, 28), 16, 3, dict(error=0.02)),
}
VIEWS = TS.VIEWS[1:]
