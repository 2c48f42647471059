"""pt_render -RR on the GPU: the BMP of -DIRECT 1 -RR start[:floor] on Tor.obj is the Python path's resolve of the same frame of a
handle with roulette set, byte for byte, on the host path and under -DEVICE_RESOLVE 1, with the default floor and with one given, and
under -ENV ... -DIRECT_ENV 1 on the open scene; -RR 0 writes the bytes of a run without the flag; a malformed value, one out of
range, and -RR without -DIRECT 1 or -DIRECT_ENV 1 end with status 2."""
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
W, H, SPP, MRR = 48, 32, 8, 12


def _run(args, cwd, model_dir, model="Tor.obj", status=0):
    base = ["--W", W, "--H", H, "-RPP", SPP, "-MRR", MRR, "-UPDATE", 0, "-QUIET", 1, "-ERR", -1, "-SEED", 42, "-MODEL_PATH", model_dir, "-MODEL_NAME", model,
            "-OUT", "out.bmp"]
    cwd.mkdir(exist_ok=True)
    r = subprocess.run([EXE] + [str(a) for a in base + list(args)], cwd=cwd, capture_output=True, text=True, timeout=120)
    assert r.returncode == status, (r.returncode, r.stderr)
    return open(cwd / "out.bmp", "rb").read() if status == 0 else r.stderr


def _python_bmp(sc, path):
    s, s2, c, _ = sc.render_host(W, H, SPP, MRR, error=-1.0, seed=42, want_stats=False)
    pt.write_bmp(path, pt.resolve(W, H, s, s2, c)[0])
    return open(path, "rb").read()


def test_rr_writes_the_librarys_bytes_and_rr_0_is_a_run_without_the_flag(tmp_path, models_dir):
    direct = _run(["-DIRECT", 1], tmp_path / "direct", models_dir)
    off = _run(["-DIRECT", 1, "-RR", 0], tmp_path / "off", models_dir)
    host = _run(["-DIRECT", 1, "-RR", 3], tmp_path / "host", models_dir)
    device = _run(["-DIRECT", 1, "-RR", 3, "-DEVICE_RESOLVE", 1], tmp_path / "device", models_dir)
    given = _run(["-DIRECT", 1, "-RR", "1:0.5"], tmp_path / "given", models_dir)
    assert off == direct
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    sc.set_direct_lighting(True)
    mine = str(tmp_path / "python.bmp")
    assert _python_bmp(sc, mine) == direct
    sc.set_roulette(3)
    assert _python_bmp(sc, mine) == host == device and host != direct
    sc.set_roulette(1, 0.5)
    assert _python_bmp(sc, mine) == given and given != host
    sc.close()


def test_rr_under_environment_sampling(tmp_path):
    d = str(tmp_path / "scene") + "/"
    os.makedirs(d)
    ES.open_tor(d)
    pic = np.full((16, 32, 3), 0.2, np.float32)
    pic[5, 20] = 3000.0
    open(d + "sun.pfm", "wb").write(E.pfm_bytes(pic))
    env = ["-ENV", d + "sun.pfm", "-ENV_SIZE", 16, "-DIRECT_ENV", 1]
    plain = _run(env, tmp_path / "plain", d, model="Open.obj")
    host = _run(env + ["-RR", "2:0.25"], tmp_path / "host", d, model="Open.obj")
    sc = pt.Scene.load_obj(d, "Open.obj", device=0)
    sc.set_environment(d + "sun.pfm", size=16)
    sc.set_environment_sampling()
    sc.set_roulette(2, 0.25)
    assert _python_bmp(sc, str(tmp_path / "python.bmp")) == host and host != plain
    sc.close()


@pytest.mark.parametrize("flags", [["-RR", 3], ["-DIRECT", 1, "-RR", "x"], ["-DIRECT", 1, "-RR", "3:4"], ["-DIRECT", 1, "-RR", "-2"]])
def test_the_status_2_cases(tmp_path, models_dir, flags):
    err = _run(flags, tmp_path / "refused", models_dir, status=2)
    assert "-RR" in err
