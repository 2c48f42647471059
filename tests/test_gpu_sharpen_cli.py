"""pt_render's sharpening flags (-SHARPEN, -SHARPEN_LIMIT): the file of one frame is the host chain restatement -> pt_grade_host ->
pt_tonemap -> pt_quantize of the frame's accumulators; the host path and -DEVICE_RESOLVE 1 write byte-identical files, also with
-RENDER_SCALE 2 -DENOISE 3; and a run without -SHARPEN, or with -SHARPEN 0, writes what the same command writes without the flags."""
import glob
import importlib
import os
import subprocess

import numpy as np
import pytest

import sharpen_restatement as R

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
F = np.float32
W, H = 64, 48
SPP = 64                                     # at a few samples an unfiltered frame is lit pixels on black, which the stage leaves alone
LOOK = ["-EYE", "-2,-5,-8", "-LOOKAT", "0,9,0", "-OUT", "one.bmp"]


def _run(args, cwd, ok=True):
    r = subprocess.run([EXE] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def _base(models_dir):
    return ["--W", W, "--H", H, "-RPP", SPP, "-MRR", 4, "-UPDATE", 0, "-QUIET", 1, "-SEED", 42, "-MODEL_PATH", models_dir]


def _render(tmp_path, tag, args):
    work = tmp_path / tag
    work.mkdir()
    r = _run(args, work)
    assert "ignored" not in r.stderr
    return {os.path.basename(p): open(p, "rb").read() for p in glob.glob(str(work / "*.bmp"))}


def test_one_frame_is_the_library_chain_on_both_paths(tmp_path, models_dir):
    g = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    g.set_camera(pt.look_at((-2.0, -5.0, -8.0), (0.0, 9.0, 0.0)))
    s, s2, c, _ = g.render_host(W, H, SPP, 4, error=0.001, seed=42, want_stats=False)
    mean, count = pt.denoise(W, H, s, s2, c, None, levels=0)
    mean, count = np.asarray(mean, F).reshape(H, W, 3), np.asarray(count, np.int32).reshape(H, W)
    finish = lambda img, e, curve: pt.quantize(pt.tonemap(W, H, pt.grade(img, count, F(e), curve), count.reshape(-1)), count)
    seen = []
    for tag, flags, e, curve, prm in [
            ("alone", ["-SHARPEN", 0.5], 1.0, "reference", dict(strength=0.5)),
            ("graded", ["-SHARPEN", 1, "-SHARPEN_LIMIT", 0.05, "-TONE", "aces", "-EXPOSURE", 1], 2.0, "aces", dict(strength=1.0, limit=0.05))]:
        want_bgr = finish(R.sharpen(mean, count, F(e), **prm), e, curve)
        assert (want_bgr != finish(mean, e, curve)).any(), "nothing changed"
        ref = str(tmp_path / (tag + "_want.bmp"))
        pt.write_bmp(ref, want_bgr)
        want = open(ref, "rb").read()
        for path, extra in (("host", []), ("device", ["-DEVICE_RESOLVE", 1])):
            got = _render(tmp_path, tag + "_" + path, _base(models_dir) + LOOK + flags + extra)["one.bmp"]
            assert got == want, (tag, path)
        seen.append(want)
    assert seen[0] != seen[1]
    # no flag and -SHARPEN 0 write the same file, on either path
    plain = _render(tmp_path, "plain", _base(models_dir) + LOOK)["one.bmp"]
    assert _render(tmp_path, "zero", _base(models_dir) + LOOK + ["-SHARPEN", 0])["one.bmp"] == plain
    assert _render(tmp_path, "zero_device", _base(models_dir) + LOOK + ["-SHARPEN", 0, "-SHARPEN_LIMIT", 0.1, "-DEVICE_RESOLVE", 1])["one.bmp"] == plain


@pytest.mark.parametrize("extra", [["-TONE", "aces", "-AUTO_EXPOSURE", 1], ["-RENDER_SCALE", 2, "-DENOISE", 3],
                                   ["-RENDER_SCALE", 2, "-DENOISE", 3, "-BLOOM", 0.5, "-LOCAL", 1, "-SATURATION", 0.8, "-VIGNETTE", 1, "-TONE", "aces"]],
                         ids=["metered", "scale 2 with denoise 3", "scale 2 with every stage"])
def test_device_resolve_equals_the_host_path(tmp_path, models_dir, extra):
    args = _base(models_dir) + LOOK + extra
    host = _render(tmp_path, "host", args + ["-SHARPEN", 0.5])["one.bmp"]
    assert _render(tmp_path, "device", args + ["-SHARPEN", 0.5, "-DEVICE_RESOLVE", 1])["one.bmp"] == host
    assert len(host) == 54 + 3 * W * H
    plain = _render(tmp_path, "plain", args)["one.bmp"]
    assert host != plain
    assert _render(tmp_path, "zero", args + ["-SHARPEN", 0, "-DEVICE_RESOLVE", 1])["one.bmp"] == plain   # without the stage: the existing flags' file
