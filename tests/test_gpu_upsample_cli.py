"""pt_render -RENDER_SCALE: the frame is traced at (W / s) x (H / s) and written at W x H -- the same file on the host path and
with -DEVICE_RESOLVE 1, the Python chain's image, a refusal for sizes that are no multiple of s, and nothing new at scale 1."""
import importlib
import os
import struct
import subprocess

import pytest

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
W, H, SPP, MRR = 48, 32, 4, 4


def _run(args, cwd, models_dir, expect=0):
    base = ["--W", W, "--H", H, "-RPP", SPP, "-MRR", MRR, "-UPDATE", 0, "-QUIET", 1, "-ERR", -1, "-SEED", 42, "-MODEL_PATH", models_dir,
            "-OUT", "out.bmp"]
    r = subprocess.run([EXE] + [str(a) for a in base + list(args)], cwd=cwd, capture_output=True, text=True, timeout=120)
    assert r.returncode == expect, (r.returncode, r.stderr)
    return r


def _bmp(path):
    data = open(path, "rb").read()
    return data, struct.unpack_from("<ii", data, 18)


def test_host_and_device_paths_write_the_same_file(tmp_path, models_dir):
    outs = {}
    for tag, extra in (("host", []), ("device", ["-DEVICE_RESOLVE", 1])):
        work = tmp_path / tag
        work.mkdir()
        r = _run(["-RENDER_SCALE", 2, "-DENOISE", 3] + extra, work, models_dir)
        outs[tag], size = _bmp(work / "out.bmp")
        assert size == (W, H)
        assert "max_disp" in r.stdout
    assert outs["host"] == outs["device"]
    # the same chain through the Python front end: traced at 24 x 16, denoised there, upsampled to 48 x 32
    w, h = W // 2, H // 2
    tor = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    s, s2, c, _ = tor.render_host(w, h, SPP, MRR, error=-1.0, seed=42)
    mean_lo, count_lo = pt.denoise(w, h, s, s2, c, tor.render_features(w, h), levels=3)
    mean, cnt = pt.upsample(0, W, H, mean_lo, count_lo, tor.render_features(W, H), 2)
    ref = str(tmp_path / "ref.bmp")
    pt.write_bmp(ref, pt.quantize(pt.tonemap(W, H, mean, cnt), cnt.reshape(H, W)))
    assert open(ref, "rb").read() == outs["host"]


def test_other_stages_combine_with_the_scale(tmp_path, models_dir):
    """A sequence with a temporal stage and a moving camera on both paths; a post filter at the written size on the unfiltered mean."""
    for tag, extra in (("sequence", ["-DENOISE", 2, "-FRAMES", 2, "-TEMPORAL", 8, "-EYE", "0,0,-20", "-EYE_END", "1,0,-20"]),):
        got = {}
        for path, flag in (("host", []), ("device", ["-DEVICE_RESOLVE", 1])):
            work = tmp_path / (tag + path)
            work.mkdir()
            _run(["-RENDER_SCALE", 2] + extra + flag, work, models_dir)
            got[path], size = _bmp(work / "out.bmp")
            assert size == (W, H)
        assert got["host"] == got["device"], tag
    a, b = tmp_path / "gauss", tmp_path / "nogauss"
    a.mkdir(), b.mkdir()
    _run(["-RENDER_SCALE", 4, "-GAUSS", 1], a, models_dir)
    _run(["-RENDER_SCALE", 4], b, models_dir)
    (da, sa), (db, sb) = _bmp(a / "out.bmp"), _bmp(b / "out.bmp")
    assert sa == sb == (W, H) and da != db


def test_sizes_that_are_no_multiple_of_the_scale_are_refused(tmp_path, models_dir):
    r = _run(["--W", 50, "-RENDER_SCALE", 4], tmp_path, models_dir, expect=1)
    assert "RENDER_SCALE" in r.stderr and not os.path.exists(tmp_path / "out.bmp")
    for scale in (0, 5, -2):
        r = _run(["-RENDER_SCALE", scale], tmp_path, models_dir, expect=1)
        assert "RENDER_SCALE" in r.stderr


def test_scale_1_changes_nothing(tmp_path, models_dir):
    outs = []
    for tag, extra in (("with", ["-RENDER_SCALE", 1]), ("without", [])):
        work = tmp_path / tag
        work.mkdir()
        _run(["-DENOISE", 3] + extra, work, models_dir)
        outs.append(_bmp(work / "out.bmp"))
    assert outs[0] == outs[1] and outs[0][1] == (W, H)
