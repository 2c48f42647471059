"""pt_render -SMOOTH on the GPU: the BMP of -SMOOTH auto (with and without -CREASE) and of -SMOOTH vn on the TorSmooth.obj that
tools/make_smooth_scene.py writes is the Python path's resolve of the same frame of a handle with the same normals, on the host path
and under -DEVICE_RESOLVE 1, and the frame is lit (the lamp of Tor.obj winds against its vn: a loader that turned it round would
leave the closed room black); a run without the flag writes the bytes of the golden frame tests/golden/tor_frame_64x64x16.npz, the
accumulators from before the feature."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
W, H, SPP, MRR = 48, 32, 32, 6


def _run(args, cwd, model_dir, shape=(W, H, SPP, MRR)):
    w, h, spp, mrr = shape
    base = ["--W", w, "--H", h, "-RPP", spp, "-MRR", mrr, "-UPDATE", 0, "-QUIET", 1, "-ERR", -1, "-SEED", 42, "-MODEL_PATH", model_dir, "-OUT", "out.bmp"]
    cwd.mkdir(exist_ok=True)
    r = subprocess.run([EXE] + [str(a) for a in base + list(args)], cwd=cwd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return open(cwd / "out.bmp", "rb").read()


def _python_bmp(sc, path):
    s, s2, c, _ = sc.render_host(W, H, SPP, MRR, error=-1.0, seed=42, want_stats=False)
    bgr = pt.resolve(W, H, s, s2, c)[0]
    pt.write_bmp(path, bgr)
    return open(path, "rb").read(), bgr


def _lit(bgr, plain):
    """A closed room whose lamp gives nothing is black in every pixel.  The room is dim -- at this sample count most pixels of the frame
    without the flag are still black -- so the frame is measured against that one: shading normals on the torus leave the walls' light
    as it was, so at least half as many pixels are lit and the mean is at least half the mean without the flag."""
    lit, lit_plain = (bgr.max(axis=2) > 0).sum(), (plain.max(axis=2) > 0).sum()
    return lit_plain > 0 and lit >= 0.5 * lit_plain and bgr.mean() >= 0.5 * plain.mean()


def test_smooth_auto_writes_the_librarys_bytes_and_is_lit(tmp_path, models_dir):
    host = _run(["-SMOOTH", "auto"], tmp_path / "host", models_dir)
    device = _run(["-SMOOTH", "auto", "-DEVICE_RESOLVE", 1], tmp_path / "device", models_dir)
    narrow = _run(["-SMOOTH", "auto", "-CREASE", 30], tmp_path / "narrow", models_dir)
    plain = _run([], tmp_path / "plain", models_dir)
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    mine = str(tmp_path / "python.bmp")
    plain_bytes, plain_bgr = _python_bmp(sc, mine)
    assert plain_bytes == plain                                             # without the flag: the frame of a handle without normals
    sc.set_shading_normals(pt.smooth_normals(sc.triangles()[0]))
    got, bgr = _python_bmp(sc, mine)
    assert got == host == device and host != plain and _lit(bgr, plain_bgr)
    sc.set_shading_normals(pt.smooth_normals(sc.triangles()[0], 30.0))
    got, bgr = _python_bmp(sc, mine)
    assert got == narrow and narrow != host and narrow != plain and _lit(bgr, plain_bgr)
    sc.close()


def test_smooth_vn_on_the_tools_scene_writes_the_librarys_bytes_and_is_lit(tmp_path, models_dir):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_smooth_scene as MS
    d = str(tmp_path / "scene") + "/"
    MS.generate(models_dir, d)
    name = ["-MODEL_NAME", "TorSmooth.obj"]
    host = _run(name + ["-SMOOTH", "vn"], tmp_path / "host", d)
    device = _run(name + ["-SMOOTH", "vn", "-DEVICE_RESOLVE", 1], tmp_path / "device", d)
    plain = _run(name, tmp_path / "plain", d)
    mine = str(tmp_path / "python.bmp")
    ref = pt.Scene.load_obj(d, "TorSmooth.obj", device=0)                   # without the flag: the reference's planes, nothing applied
    plain_bytes, plain_bgr = _python_bmp(ref, mine)
    assert plain_bytes == plain and ref.shading_normals() is None
    sc = pt.Scene.load_obj(d, "TorSmooth.obj", device=0, geometric_planes=True)
    N, N_ref, tri_mat = sc.triangles()[0][:, 0:3], ref.triangles()[0][:, 0:3], sc.triangles()[1]
    assert ((N * N_ref).sum(1) > 0).all() and (tri_mat == 0).any()          # every face, the lamp (material 0) included, keeps its side
    sc.set_shading_normals(sc.vertex_normals())
    got, bgr = _python_bmp(sc, mine)
    assert got == host == device and host != plain and _lit(bgr, plain_bgr)
    sc.close()
    ref.close()


def test_without_the_flag_the_golden_frame(tmp_path, models_dir):
    z = np.load(os.path.join(ROOT, "tests", "golden", "tor_frame_64x64x16.npz"))
    w, h, spp, mrr = int(z["width"]), int(z["height"]), int(z["spp"]), int(z["mrr"])
    assert float(z["error"]) == -1.0 and int(z["seed"]) == 42
    got = _run([], tmp_path / "plain", models_dir, (w, h, spp, mrr))
    want = str(tmp_path / "golden.bmp")
    pt.write_bmp(want, pt.resolve(w, h, z["sum_bits"].view(np.float32), z["sum2_bits"].view(np.float32), z["count"])[0])
    assert got == open(want, "rb").read()
