"""pt_render -ENV on the GPU: the BMP is the Python path's resolve of the same frame, with and without -DEVICE_RESOLVE 1 and with
-FRAMES 2; -ENV_GAIN, -ENV_ROTATE and -ENV_SIZE reach the library; the scene-linear file of both paths is the same; a run without -ENV
is unchanged by the flags' existence."""
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
W, H, SPP, MRR = 48, 32, 4, 4
VIEW = ["-EYE", "4,-3,-26", "-LOOKAT", "0,0,0", "-ASPECT", "1.5"]


def _run(args, cwd, models_dir, outputs=("out.bmp",)):
    base = ["--W", W, "--H", H, "-RPP", SPP, "-MRR", MRR, "-UPDATE", 0, "-QUIET", 1, "-ERR", -1, "-SEED", 42, "-MODEL_PATH", models_dir,
            "-OUT", "out.bmp"]
    cwd.mkdir(exist_ok=True)
    r = subprocess.run([EXE] + [str(a) for a in base + list(args)], cwd=cwd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return [open(cwd / o, "rb").read() for o in outputs]


@pytest.fixture()
def panorama(tmp_path):
    rng = np.random.default_rng(7)
    pic = rng.uniform(0.05, 1.5, (16, 32, 3)).astype(np.float32)
    pic[3, 20] = 300.0
    path = str(tmp_path / "pano.pfm")
    open(path, "wb").write(E.pfm_bytes(pic))
    return path, pic


def test_env_writes_the_python_paths_resolve_of_the_same_frame(tmp_path, models_dir, panorama):
    path, pic = panorama
    flags = VIEW + ["-ENV", path, "-ENV_GAIN", "1.5", "-ENV_ROTATE", "40", "-ENV_SIZE", "32"]
    host, = _run(flags, tmp_path / "host", models_dir)
    device, = _run(flags + ["-DEVICE_RESOLVE", 1], tmp_path / "device", models_dir)
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    sc.set_camera(pt.look_at((4.0, -3.0, -26.0), (0.0, 0.0, 0.0), aspect=1.5))
    sc.set_environment(pic, gain=1.5, rotate=40.0, size=32)
    s, s2, c, _ = sc.render_host(W, H, SPP, MRR, error=-1.0, seed=42, want_stats=False)
    bgr, _ = pt.resolve(W, H, s, s2, c)
    mine = str(tmp_path / "python.bmp")
    pt.write_bmp(mine, bgr)
    assert open(mine, "rb").read() == host == device
    # a run without -ENV writes what it wrote before the flag existed: the library's frame of a handle without an environment
    plain, = _run(VIEW, tmp_path / "plain", models_dir)
    plain_device, = _run(VIEW + ["-DEVICE_RESOLVE", 1], tmp_path / "plain_device", models_dir)
    sc.set_environment(None)
    s, s2, c, _ = sc.render_host(W, H, SPP, MRR, error=-1.0, seed=42, want_stats=False)
    pt.write_bmp(mine, pt.resolve(W, H, s, s2, c)[0])
    assert open(mine, "rb").read() == plain == plain_device
    assert host != plain                                                    # the camera stands outside the room: the background is the panorama
    sc.close()


def test_env_with_two_frames_and_the_linear_output_of_both_paths(tmp_path, models_dir, panorama):
    path, _ = panorama
    flags = VIEW + ["-ENV", path, "-LINEAR_OUT", "lin.hdr"]
    host = _run(flags, tmp_path / "host", models_dir, ("out.bmp", "lin.hdr"))
    device = _run(flags + ["-DEVICE_RESOLVE", 1], tmp_path / "device", models_dir, ("out.bmp", "lin.hdr"))
    assert host == device
    two = VIEW + ["-ENV", path, "-FRAMES", 2, "-EYE_END", "5,-3,-26", "-LOOKAT_END", "0,0,0"]
    names = ("frame_0000.bmp", "frame_0001.bmp", "out.bmp")
    frames = _run(two, tmp_path / "two_host", models_dir, names)
    assert frames == _run(two + ["-DEVICE_RESOLVE", 1], tmp_path / "two_device", models_dir, names)
    assert frames[0] != frames[1] and frames[1] == frames[2]
