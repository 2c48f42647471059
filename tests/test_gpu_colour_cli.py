"""pt_render's colour flags (-WB, -SATURATION, -COLOR_MATRIX, -LUT): the file of one frame is the library's host chain of the frame's
accumulators; the host path and -DEVICE_RESOLVE 1 write byte-identical files; a run without the flags writes what it wrote
before they existed; bad values and a malformed .cube file end the run with a message."""
import glob
import importlib
import os
import subprocess

import numpy as np
import pytest

import colour_cases as K
import colour_restatement as R

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
F = np.float32
W, H = 64, 48
LOOK = ["-EYE", "-2,-5,-8", "-LOOKAT", "0,9,0", "-OUT", "one.bmp"]
MATRIX = [[0.9, 0.1, 0.0], [0.05, 0.9, 0.05], [0.0, 0.2, 0.8]]


def _run(args, cwd, ok=True):
    r = subprocess.run([EXE] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def _base(models_dir):
    return ["--W", W, "--H", H, "-RPP", 4, "-MRR", 4, "-UPDATE", 0, "-QUIET", 1, "-SEED", 42, "-MODEL_PATH", models_dir]


def _render(tmp_path, tag, args):
    work = tmp_path / tag
    work.mkdir()
    r = _run(args, work)
    assert "ignored" not in r.stderr
    return open(work / "one.bmp", "rb").read()


def test_one_frame_is_the_librarys_bytes_on_both_paths(tmp_path, models_dir):
    cube = str(tmp_path / "x.cube")
    table = K.lut("random", 17)
    R.write_cube(cube, table, title="x")
    g = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    g.set_camera(pt.look_at((-2.0, -5.0, -8.0), (0.0, 9.0, 0.0)))
    s, s2, c, _ = g.render_host(W, H, 4, 4, error=0.001, seed=42, want_stats=False)
    mean, count = pt.denoise(W, H, s, s2, c, None, levels=0)
    mean, count = np.asarray(mean, F).reshape(H, W, 3), np.asarray(count, np.int32).reshape(H, W)
    plain = _render(tmp_path, "plain", _base(models_dir) + LOOK + ["-TONE", "aces"])
    seen = [plain]
    for tag, flags, colour in [("all", ["-WB", "1.1,1,0.9", "-SATURATION", 0.8, "-LUT", cube], dict(wb=(1.1, 1, 0.9), saturation=0.8, lut=pt.Lut.load_cube(cube))),
                               ("matrix", ["-COLOR_MATRIX", ",".join(str(v) for row in MATRIX for v in row), "-SATURATION", 0], dict(matrix=MATRIX, saturation=0.0))]:
        want_bgr = pt.quantize(pt.tonemap(W, H, pt.colour(mean, count, 1.0, "aces", colour), count), count)
        ref = str(tmp_path / (tag + "_want.bmp"))
        pt.write_bmp(ref, want_bgr)
        want = open(ref, "rb").read()
        for path, extra in (("host", []), ("device", ["-DEVICE_RESOLVE", 1])):
            got = _render(tmp_path, tag + "_" + path, _base(models_dir) + LOOK + ["-TONE", "aces"] + flags + extra)
            assert got == want, (tag, path)
        seen.append(want)
    assert len(set(seen)) == 3
    # the identity in every flag is no stage: the existing chain's file, on both paths
    for path, extra in (("host", []), ("device", ["-DEVICE_RESOLVE", 1])):
        same = _render(tmp_path, "unit_" + path, _base(models_dir) + LOOK + ["-TONE", "aces", "-WB", "1,1,1", "-SATURATION", 1, "-COLOR_MATRIX", "1,0,0,0,1,0,0,0,1"] + extra)
        assert same == plain
    # alone, without -TONE: the zeroed grade; and with bloom, local exposure, a scale and a sequence's metering on both paths
    rest = ["-WB", "1.2,1,0.8", "-LUT", cube, "-BLOOM", 0.5, "-LOCAL", 1, "-RENDER_SCALE", 2, "-AUTO_EXPOSURE", 1, "-TONE", "reinhard"]
    assert _render(tmp_path, "rest_host", _base(models_dir) + LOOK + rest) == _render(tmp_path, "rest_device", _base(models_dir) + LOOK + rest + ["-DEVICE_RESOLVE", 1])
    assert _render(tmp_path, "alone_host", _base(models_dir) + LOOK + ["-LUT", cube]) == _render(tmp_path, "alone_device", _base(models_dir) + LOOK + ["-LUT", cube, "-DEVICE_RESOLVE", 1])


def test_bad_flags_and_a_malformed_cube_are_refused(tmp_path, models_dir):
    for flags, word in ((["-WB", "1,1"], "-WB"), (["-WB", "1,-1,1"], "-WB"), (["-SATURATION", -1], "-SATURATION"), (["-SATURATION", "x"], "-SATURATION"),
                        (["-COLOR_MATRIX", "1,0,0,0,1,0,0,0"], "-COLOR_MATRIX"), (["-COLOR_MATRIX", "1,0,0,0,nan,0,0,0,1"], "-COLOR_MATRIX")):
        r = _run(_base(models_dir) + ["-OUT", "x.bmp"] + flags, tmp_path, ok=False)
        assert r.returncode == 2 and word in r.stderr and not glob.glob(str(tmp_path / "*.bmp")), (flags, r.stderr)
    bad = tmp_path / "bad.cube"
    bad.write_text("LUT_3D_SIZE 2\n" + "0 0 0\n" * 7)
    r = _run(_base(models_dir) + ["-OUT", "x.bmp", "-LUT", bad], tmp_path, ok=False)
    assert r.returncode != 0 and "7 data lines" in r.stderr and "bad.cube" in r.stderr and not glob.glob(str(tmp_path / "*.bmp"))
    r = _run(_base(models_dir) + ["-OUT", "x.bmp", "-LUT", tmp_path / "missing.cube"], tmp_path, ok=False)
    assert r.returncode != 0 and "cannot open" in r.stderr
