"""pt_render -DIRECT_ENV on the GPU: the BMP of -ENV sun.pfm -DIRECT_ENV 1 on the open Tor scene is the Python path's resolve of the same
frame of a handle with the switch on, byte for byte, on the host path and under -DEVICE_RESOLVE 1, with a share given, and with
-FRAMES 2 (the first frame is the single frame, the second another, the same on both paths); -DIRECT_ENV 0 writes the bytes of a run without the flag; a black environment and a textured emitter
end with status 2."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import environment_restatement as E
import envdirect_scenes as ES

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
W, H, SPP, MRR = 48, 32, 8, 4


def _run(args, cwd, model_dir, status=0):
    base = ["--W", W, "--H", H, "-RPP", SPP, "-MRR", MRR, "-UPDATE", 0, "-QUIET", 1, "-ERR", -1, "-SEED", 42, "-MODEL_PATH", model_dir, "-MODEL_NAME", "Open.obj",
            "-OUT", "out.bmp"]
    cwd.mkdir(exist_ok=True)
    r = subprocess.run([EXE] + [str(a) for a in base + list(args)], cwd=cwd, capture_output=True, text=True, timeout=120)
    assert r.returncode == status, (r.returncode, r.stderr)
    return open(cwd / "out.bmp", "rb").read() if status == 0 else r.stderr


def _python_bmp(sc, path):
    s, s2, c, _ = sc.render_host(W, H, SPP, MRR, error=-1.0, seed=42, want_stats=False)
    pt.write_bmp(path, pt.resolve(W, H, s, s2, c)[0])
    return open(path, "rb").read()


def test_direct_env_writes_the_librarys_bytes_and_direct_env_0_is_a_run_without_the_flag(tmp_path):
    d = str(tmp_path / "scene") + "/"
    os.makedirs(d)
    ES.open_tor(d)
    pic = np.full((16, 32, 3), 0.2, np.float32)                                # an equirectangular picture with a sun above the horizon
    pic[5, 20] = 3000.0
    open(d + "sun.pfm", "wb").write(E.pfm_bytes(pic))
    open(d + "black.pfm", "wb").write(E.pfm_bytes(np.zeros((16, 32, 3), np.float32)))
    env = ["-ENV", d + "sun.pfm", "-ENV_SIZE", 16]
    host = _run(env + ["-DIRECT_ENV", 1], tmp_path / "host", d)
    device = _run(env + ["-DIRECT_ENV", 1, "-DEVICE_RESOLVE", 1], tmp_path / "device", d)
    frames = _run(env + ["-DIRECT_ENV", 1, "-FRAMES", 2], tmp_path / "frames", d)
    frames_device = _run(env + ["-DIRECT_ENV", 1, "-FRAMES", 2, "-DEVICE_RESOLVE", 1], tmp_path / "frames_device", d)
    given = _run(env + ["-DIRECT_ENV", 1, "-DIRECT_ENV_SHARE", 0.7, "-DIRECT", 1], tmp_path / "given", d)
    plain = _run(env, tmp_path / "plain", d)
    off = _run(env + ["-DIRECT_ENV", 0], tmp_path / "off", d)
    assert off == plain
    sc = pt.Scene.load_obj(d, "Open.obj", device=0)
    sc.set_environment(d + "sun.pfm", size=16)
    mine = str(tmp_path / "python.bmp")
    assert _python_bmp(sc, mine) == plain                                      # without the flag: the frame of a handle without the switch
    sc.set_environment_sampling()
    assert _python_bmp(sc, mine) == host == device and host != plain
    first = open(tmp_path / "frames" / "frame_0000.bmp", "rb").read()          # a sequence: frame 0 is passes [0, RPP), frame 1 the next RPP
    assert first == host and frames == frames_device and frames != host
    if len(sc.lights()[0]):
        sc.set_environment_sampling(0.7)
        sc.set_direct_lighting(True)
        assert _python_bmp(sc, mine) == given and given != host
    sc.close()
    assert "black" in _run(["-ENV", d + "black.pfm", "-DIRECT_ENV", 1], tmp_path / "black", d, status=2)
    pt.write_bmp(d + "t.bmp", np.full((2, 2, 3), 128, np.uint8))
    err = _run(env + ["-DIRECT_ENV", 1, "-TEXTURE", "0:" + d + "t.bmp"], tmp_path / "lamp", d, status=2)
    assert "texture list" in err
