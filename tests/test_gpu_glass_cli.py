"""pt_render -GLASS on the GPU: the BMP is the Python path's resolve of the same frame of a handle with the same dielectrics, on the
host path and under -DEVICE_RESOLVE 1, with -ENV, with -LINEAR_OUT and with -FRAMES 2; a run without -GLASS writes what the library
renders without a list."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import environment_restatement as E

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
W, H, SPP, MRR = 48, 32, 4, 6
VIEW = ["-EYE", "4,-3,-26", "-LOOKAT", "0,0,0", "-ASPECT", "1.5"]          # from outside the room: through its glass wall, past it the background
GLASS = ["-GLASS", "4:1.5:0.9:1:0.9,2:1.33,1:1.5,3:1.5"]
ENTRIES = [(4, 1.5, (0.9, 1.0, 0.9)), (2, 1.33, (1, 1, 1)), (1, 1.5, (1, 1, 1)), (3, 1.5, (1, 1, 1))]


def _run(args, cwd, models_dir, outputs=("out.bmp",)):
    base = ["--W", W, "--H", H, "-RPP", SPP, "-MRR", MRR, "-UPDATE", 0, "-QUIET", 1, "-ERR", -1, "-SEED", 42, "-MODEL_PATH", models_dir,
            "-OUT", "out.bmp"]
    cwd.mkdir(exist_ok=True)
    r = subprocess.run([EXE] + [str(a) for a in base + list(args)], cwd=cwd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return [open(cwd / o, "rb").read() for o in outputs]


def _python_bmp(sc, path):
    s, s2, c, _ = sc.render_host(W, H, SPP, MRR, error=-1.0, seed=42, want_stats=False)
    pt.write_bmp(path, pt.resolve(W, H, s, s2, c)[0])
    return open(path, "rb").read()


def test_glass_writes_the_librarys_bytes_with_and_without_an_environment(tmp_path, models_dir):
    pic = np.random.default_rng(7).uniform(0.05, 1.5, (16, 32, 3)).astype(np.float32)
    pano = str(tmp_path / "pano.pfm")
    open(pano, "wb").write(E.pfm_bytes(pic))
    host, = _run(VIEW + GLASS, tmp_path / "host", models_dir)
    device, = _run(VIEW + GLASS + ["-DEVICE_RESOLVE", 1], tmp_path / "device", models_dir)
    lit, = _run(VIEW + GLASS + ["-ENV", pano, "-ENV_SIZE", 16], tmp_path / "env", models_dir)
    plain, = _run(VIEW, tmp_path / "plain", models_dir)
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    sc.set_camera(pt.look_at((4.0, -3.0, -26.0), (0.0, 0.0, 0.0), aspect=1.5))
    mine = str(tmp_path / "python.bmp")
    assert _python_bmp(sc, mine) == plain                                   # without the flag: the frame of a handle without a list
    sc.set_dielectrics([pt.dielectric(*e) for e in ENTRIES])
    assert _python_bmp(sc, mine) == host == device and host != plain
    sc.set_environment(pic, size=16)
    assert _python_bmp(sc, mine) == lit and lit != host
    sc.close()


def test_glass_with_the_linear_output_and_two_frames(tmp_path, models_dir):
    flags = VIEW + GLASS + ["-LINEAR_OUT", "lin.hdr"]
    host = _run(flags, tmp_path / "host", models_dir, ("out.bmp", "lin.hdr"))
    assert host == _run(flags + ["-DEVICE_RESOLVE", 1], tmp_path / "device", models_dir, ("out.bmp", "lin.hdr"))
    assert host[1] != _run(VIEW + ["-LINEAR_OUT", "lin.hdr"], tmp_path / "plain", models_dir, ("lin.hdr",))[0]
    two = VIEW + GLASS + ["-FRAMES", 2, "-EYE_END", "5,-3,-26", "-LOOKAT_END", "0,0,0"]
    names = ("frame_0000.bmp", "frame_0001.bmp", "out.bmp")
    frames = _run(two, tmp_path / "two_host", models_dir, names)
    assert frames == _run(two + ["-DEVICE_RESOLVE", 1], tmp_path / "two_device", models_dir, names)
    assert frames[0] != frames[1] and frames[1] == frames[2]
    assert frames != _run(VIEW + ["-FRAMES", 2, "-EYE_END", "5,-3,-26", "-LOOKAT_END", "0,0,0"], tmp_path / "two_plain", models_dir, names)
