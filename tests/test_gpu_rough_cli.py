"""pt_render -ROUGH on the GPU: the BMP of -ROUGH 4:0.3 on Tor.obj is the Python path's resolve of the same frame of a handle with the
same list, byte for byte, on the host path and under -DEVICE_RESOLVE 1, and combined with -GLASS and -SMOOTH; -ROUGH mtl on the room
that tests/rough_scenes.py writes (an MTL with Pr lines: one inside the range, one above it, one on a material without a glossy lobe)
is the frame of the list the flag is stated to make; a run without the flag writes the bytes of a handle without a list."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import rough_scenes as RS

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
W, H, SPP, MRR = 48, 32, 8, 6


def _run(args, cwd, model_dir):
    base = ["--W", W, "--H", H, "-RPP", SPP, "-MRR", MRR, "-UPDATE", 0, "-QUIET", 1, "-ERR", -1, "-SEED", 42, "-MODEL_PATH", model_dir, "-OUT", "out.bmp"]
    cwd.mkdir(exist_ok=True)
    r = subprocess.run([EXE] + [str(a) for a in base + list(args)], cwd=cwd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return open(cwd / "out.bmp", "rb").read()


def _python_bmp(sc, path):
    s, s2, c, _ = sc.render_host(W, H, SPP, MRR, error=-1.0, seed=42, want_stats=False)
    pt.write_bmp(path, pt.resolve(W, H, s, s2, c)[0])
    return open(path, "rb").read()


def test_rough_entries_write_the_librarys_bytes(tmp_path, models_dir):
    host = _run(["-ROUGH", "4:0.3"], tmp_path / "host", models_dir)
    device = _run(["-ROUGH", "4:0.3", "-DEVICE_RESOLVE", 1], tmp_path / "device", models_dir)
    both = _run(["-ROUGH", "1:0.1,2:1", "-GLASS", "4:1.5", "-SMOOTH", "auto"], tmp_path / "both", models_dir)
    plain = _run([], tmp_path / "plain", models_dir)
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    mine = str(tmp_path / "python.bmp")
    assert _python_bmp(sc, mine) == plain                                    # without the flag: the frame of a handle without a list
    sc.set_roughness([pt.rough(4, 0.3)])
    assert _python_bmp(sc, mine) == host == device and host != plain
    sc.set_roughness([pt.rough(1, 0.1), pt.rough(2, 1.0)])
    sc.set_dielectrics([pt.dielectric(4, 1.5)])
    sc.set_shading_normals(pt.smooth_normals(sc.triangles()[0]))
    assert _python_bmp(sc, mine) == both and both != host
    sc.close()


def test_rough_mtl_takes_the_pr_lines_of_the_materials_with_a_glossy_lobe(tmp_path):
    d = str(tmp_path / "scene") + "/"
    os.makedirs(d)
    RS.room(d)
    name = ["-MODEL_NAME", "rough_room.obj"]
    host = _run(name + ["-ROUGH", "mtl"], tmp_path / "host", d)
    listed = _run(name + ["-ROUGH", ",".join(f"{m}:{a}" for m, a in RS.ROOM_MTL_LIST.items())], tmp_path / "listed", d)
    plain = _run(name, tmp_path / "plain", d)
    sc = pt.Scene.load_obj(d, "rough_room.obj", device=0)
    mine = str(tmp_path / "python.bmp")
    assert _python_bmp(sc, mine) == plain and sc.roughness() == []           # the loader applies nothing
    assert np.array_equal(sc.mtl_roughness(), np.array(RS.ROOM_PR, np.float32))
    sc.set_roughness([pt.rough(m, a) for m, a in RS.ROOM_MTL_LIST.items()])
    assert _python_bmp(sc, mine) == host == listed and host != plain
    sc.close()
