"""pt_render -DIRECT on the GPU: the BMP of -DIRECT 1 on Tor.obj is the Python path's resolve of the same frame of a handle with the
switch on, byte for byte, on the host path and under -DEVICE_RESOLVE 1, and combined with -GLASS, -ROUGH and -SMOOTH; -DIRECT 0 writes
the bytes of a run without the flag; a model without a light and a textured emitter end with status 2."""
import importlib
import os
import subprocess

import numpy as np
import pytest

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
W, H, SPP, MRR = 48, 32, 8, 4


def _run(args, cwd, model_dir, status=0):
    base = ["--W", W, "--H", H, "-RPP", SPP, "-MRR", MRR, "-UPDATE", 0, "-QUIET", 1, "-ERR", -1, "-SEED", 42, "-MODEL_PATH", model_dir, "-OUT", "out.bmp"]
    cwd.mkdir(exist_ok=True)
    r = subprocess.run([EXE] + [str(a) for a in base + list(args)], cwd=cwd, capture_output=True, text=True, timeout=120)
    assert r.returncode == status, (r.returncode, r.stderr)
    return open(cwd / "out.bmp", "rb").read() if status == 0 else r.stderr


def _python_bmp(sc, path):
    s, s2, c, _ = sc.render_host(W, H, SPP, MRR, error=-1.0, seed=42, want_stats=False)
    pt.write_bmp(path, pt.resolve(W, H, s, s2, c)[0])
    return open(path, "rb").read()


def test_direct_writes_the_librarys_bytes_and_direct_0_is_a_run_without_the_flag(tmp_path, models_dir):
    host = _run(["-DIRECT", 1], tmp_path / "host", models_dir)
    device = _run(["-DIRECT", 1, "-DEVICE_RESOLVE", 1], tmp_path / "device", models_dir)
    both = _run(["-DIRECT", 1, "-ROUGH", "2:0.3", "-GLASS", "4:1.5", "-SMOOTH", "auto"], tmp_path / "both", models_dir)
    plain = _run([], tmp_path / "plain", models_dir)
    off = _run(["-DIRECT", 0], tmp_path / "off", models_dir)
    assert off == plain
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    mine = str(tmp_path / "python.bmp")
    assert _python_bmp(sc, mine) == plain                                    # without the flag: the frame of a handle without the switch
    sc.set_direct_lighting(True)
    assert _python_bmp(sc, mine) == host == device and host != plain
    sc.set_roughness([pt.rough(2, 0.3)])
    sc.set_dielectrics([pt.dielectric(4, 1.5)])
    sc.set_shading_normals(pt.smooth_normals(sc.triangles()[0]))
    assert _python_bmp(sc, mine) == both and both != host
    sc.close()


def test_a_model_without_a_light_and_a_textured_emitter_end_with_status_2(tmp_path):
    d = str(tmp_path / "scene") + "/"
    os.makedirs(d)
    open(d + "dark.mtl", "w").write("newmtl 0\nNs 0\nKd 0.8 0.8 0.8\n")
    open(d + "dark.obj", "w").write("mtllib dark.mtl\nvn 0 0 -1\nv -1 -1 0\nv 1 -1 0\nv 0 1 0\nusemtl 0\nf 1//1 2//1 3//1\n")
    err = _run(["-MODEL_NAME", "dark.obj", "-DIRECT", 1], tmp_path / "dark", d, status=2)
    assert "no light" in err
    _run(["-MODEL_NAME", "dark.obj", "-DIRECT", 0], tmp_path / "dark_off", d)
    open(d + "lamp.mtl", "w").write("newmtl 0\nKe 1 1 1\nKd 1 1 1\n")
    open(d + "lamp.obj", "w").write("mtllib lamp.mtl\nvn 0 0 -1\nv -1 -1 0\nv 1 -1 0\nv 0 1 0\nusemtl 0\nf 1//1 2//1 3//1\n")
    pt.write_bmp(d + "t.bmp", np.full((2, 2, 3), 128, np.uint8))
    err = _run(["-MODEL_NAME", "lamp.obj", "-DIRECT", 1, "-TEXTURE", "0:" + d + "t.bmp"], tmp_path / "lamp", d, status=2)
    assert "texture list" in err
