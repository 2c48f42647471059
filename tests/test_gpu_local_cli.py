"""pt_render's local exposure flags (-LOCAL, -LOCAL_PIVOT, -LOCAL_LEVELS, -LOCAL_SIGMA): the host path and -DEVICE_RESOLVE 1 write
byte-identical files, with and without -RENDER_SCALE 2 and -BLOOM; a run without -LOCAL, or with -LOCAL 0, writes what the same
command wrote before the flags existed; and the file of one frame is the host chain restatement -> pt_grade_host -> pt_tonemap
-> pt_quantize of the frame's accumulators."""
import glob
import importlib
import os
import subprocess

import numpy as np
import pytest

import bloom_restatement as B
import local_restatement as R

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
F = np.float32
W, H = 64, 48
SEQUENCE = ["-FRAMES", 3, "-EYE", "-2,-5,-8", "-EYE_END", "3,-4,-12", "-LOOKAT", "0,9,0", "-LOOKAT_END", "4,0,0",          # up at the light
            "-TONE", "aces", "-AUTO_EXPOSURE", 1, "-KEY", 1, "-PERCENTILE", 20, "-OUT", "last.bmp"]
NAMES = ["frame_0000.bmp", "frame_0001.bmp", "frame_0002.bmp", "last.bmp"]


def _run(args, cwd, ok=True):
    r = subprocess.run([EXE] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def _files(work):
    return {os.path.basename(p): open(p, "rb").read() for p in glob.glob(str(work / "*.bmp"))}


def _base(models_dir):
    return ["--W", W, "--H", H, "-RPP", 4, "-MRR", 4, "-UPDATE", 0, "-QUIET", 1, "-SEED", 42, "-MODEL_PATH", models_dir]


def _render(tmp_path, tag, args):
    work = tmp_path / tag
    work.mkdir()
    r = _run(args, work)
    assert "ignored" not in r.stderr
    return _files(work)


@pytest.mark.parametrize("extra", [[], ["-RENDER_SCALE", 2, "-BLOOM", 0.5]], ids=["64x48", "64x48 at scale 2 with bloom"])
def test_a_locally_exposed_adapting_sequence_is_the_same_on_both_paths(tmp_path, models_dir, extra):
    args = _base(models_dir) + SEQUENCE + extra
    host = _render(tmp_path, "host", args + ["-LOCAL", 1.5])
    device = _render(tmp_path, "device", args + ["-LOCAL", 1.5, "-DEVICE_RESOLVE", 1])
    plain = _render(tmp_path, "plain", args)
    zero = _render(tmp_path, "zero", args + ["-LOCAL", 0, "-LOCAL_LEVELS", 3, "-LOCAL_PIVOT", 0.5, "-DEVICE_RESOLVE", 1])
    assert sorted(host) == NAMES == sorted(device) == sorted(plain) == sorted(zero)
    for name in NAMES:
        assert device[name] == host[name], name
        assert len(host[name]) == 54 + 3 * W * H
        assert zero[name] == plain[name], name                  # -LOCAL 0 is no stage: the existing flags' files
    assert host["frame_0000.bmp"] != plain["frame_0000.bmp"]


def test_one_frame_is_the_host_chain_and_the_flags_reach_the_library(tmp_path, models_dir):
    look = ["-EYE", "-2,-5,-8", "-LOOKAT", "0,9,0", "-OUT", "one.bmp"]
    g = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    g.set_camera(pt.look_at((-2.0, -5.0, -8.0), (0.0, 9.0, 0.0)))
    s, s2, c, _ = g.render_host(W, H, 4, 4, error=0.001, seed=42, want_stats=False)
    mean, count = pt.denoise(W, H, s, s2, c, None, levels=0)
    mean, count = np.asarray(mean, F).reshape(H, W, 3), np.asarray(count, np.int32).reshape(H, W)
    finish = lambda img, e, curve: pt.quantize(pt.tonemap(W, H, pt.grade(img, count, F(e), curve), count.reshape(-1)), count)
    seen = []
    for tag, flags, e, curve, bloom, local in [
            ("alone", ["-LOCAL", 1], 1.0, "reference", None, dict(strength=1.0)),
            ("graded", ["-LOCAL", 2, "-LOCAL_PIVOT", 0.5, "-LOCAL_LEVELS", 3, "-LOCAL_SIGMA", 2, "-TONE", "clamp", "-EXPOSURE", 1],
             2.0, "clamp", None, dict(strength=2.0, pivot=0.5, levels=3, sigma=2.0)),
            ("bloomed", ["-LOCAL", 1.5, "-BLOOM", 0.6, "-BLOOM_THRESHOLD", 0.5, "-TONE", "aces", "-EXPOSURE", 1],
             2.0, "aces", dict(strength=0.6, threshold=0.5), dict(strength=1.5))]:
        before = B.bloom(mean, count, F(e), **bloom) if bloom else mean
        want_bgr = finish(R.local_exposure(before, count, F(e), **local), e, curve)
        assert (want_bgr != finish(before, e, curve)).any(), "nothing changed"
        ref = str(tmp_path / (tag + "_want.bmp"))
        pt.write_bmp(ref, want_bgr)
        want = open(ref, "rb").read()
        for path, extra in (("host", []), ("device", ["-DEVICE_RESOLVE", 1])):
            got = _render(tmp_path, tag + "_" + path, _base(models_dir) + look + flags + extra)["one.bmp"]
            assert got == want, (tag, path)
        seen.append(want)
    assert len(set(seen)) == 3
    # no flag and -LOCAL 0 write the same file, on either path
    plain = _render(tmp_path, "plain", _base(models_dir) + look)["one.bmp"]
    assert _render(tmp_path, "zero", _base(models_dir) + look + ["-LOCAL", 0])["one.bmp"] == plain
    assert _render(tmp_path, "zero_device", _base(models_dir) + look + ["-LOCAL", 0, "-LOCAL_SIGMA", 3, "-DEVICE_RESOLVE", 1])["one.bmp"] == plain


def test_device_resolve_equals_the_host_path_on_a_96_x_54_frame(tmp_path, models_dir):
    args = ["--W", 96, "--H", 54, "-RPP", 4, "-MRR", 4, "-UPDATE", 0, "-QUIET", 1, "-SEED", 42, "-MODEL_PATH", models_dir,
            "-EYE", "-2,-5,-8", "-LOOKAT", "0,9,0", "-OUT", "one.bmp", "-DENOISE", 2, "-TONE", "reinhard", "-EXPOSURE", 2, "-LOCAL", 1, "-LOCAL_LEVELS", 8]
    host = _render(tmp_path, "host", args)["one.bmp"]
    assert _render(tmp_path, "device", args + ["-DEVICE_RESOLVE", 1])["one.bmp"] == host
    assert len(host) == 54 + 3 * 96 * 54


def test_bad_local_flags_are_refused(tmp_path, models_dir):
    for flags in (["-LOCAL", -1], ["-LOCAL", 1, "-LOCAL_LEVELS", 9], ["-LOCAL", 1, "-LOCAL_PIVOT", -2], ["-LOCAL", "nan"], ["-LOCAL", 1, "-LOCAL_SIGMA", -0.5]):
        r = _run(_base(models_dir) + ["-OUT", "x.bmp"] + flags, tmp_path, ok=False)
        assert r.returncode == 2 and "-LOCAL" in r.stderr and not glob.glob(str(tmp_path / "*.bmp"))
