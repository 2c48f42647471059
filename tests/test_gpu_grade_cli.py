"""pt_render's grading flags (-TONE, -EXPOSURE, -AUTO_EXPOSURE, -KEY, -PERCENTILE, -ADAPT): the host path and -DEVICE_RESOLVE 1
write byte-identical files, the flags change what they should, and a run without them is the pt_resolve chain as before."""
import glob
import importlib
import os
import subprocess

import pytest

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
UP_AT_THE_LIGHT = ["-EYE", "-2,-5,-8", "-LOOKAT", "0,9,0"]        # the emitter is a quad at y = 9


def _run(args, cwd, ok=True):
    r = subprocess.run([EXE] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def _files(work):
    return {os.path.basename(p): open(p, "rb").read() for p in glob.glob(str(work / "*.bmp"))}


def _both(tmp_path, args):
    out = []
    for tag, extra in (("host", []), ("device", ["-DEVICE_RESOLVE", 1])):
        work = tmp_path / tag
        work.mkdir()
        r = _run(args + extra, work)
        assert "ignored" not in r.stderr
        out.append(_files(work))
    return out


def _base(models_dir, W=32, H=24):
    return ["--W", W, "--H", H, "-RPP", 4, "-MRR", 4, "-UPDATE", 0, "-QUIET", 1, "-SEED", 42, "-MODEL_PATH", models_dir]


SEQUENCE = ["-FRAMES", 3, "-EYE", "-2,-5,-8", "-EYE_END", "3,-4,-12", "-LOOKAT", "0,9,0", "-LOOKAT_END", "4,0,0",
            "-TONE", "aces", "-AUTO_EXPOSURE", 1, "-ADAPT", 0.5, "-TEMPORAL", 8, "-DENOISE", 2, "-OUT", "last.bmp"]


@pytest.mark.parametrize("size,extra", [((32, 24), []), ((64, 48), ["-RENDER_SCALE", 2])], ids=["32x24", "64x48 at scale 2"])
def test_a_graded_adapting_sequence_is_the_same_on_both_paths(tmp_path, models_dir, size, extra):
    host, device = _both(tmp_path, _base(models_dir, *size) + SEQUENCE + extra)
    assert sorted(host) == ["frame_0000.bmp", "frame_0001.bmp", "frame_0002.bmp", "last.bmp"] == sorted(device)
    for name in host:
        assert device[name] == host[name], name
        assert len(host[name]) == 54 + 3 * size[0] * size[1]
    assert host["frame_0000.bmp"] != host["frame_0002.bmp"]


@pytest.mark.parametrize("flags", [["-TONE", "clamp", "-EXPOSURE", 1.5], ["-EXPOSURE", -1.5, "-TONE", "reinhard"], ["-EXPOSURE", 1], ["-AUTO_EXPOSURE", 1, "-KEY", 0.3, "-PERCENTILE", 80],
                                   ["-TONE", "aces", "-DENOISE", 2]], ids=["clamp", "reinhard", "exposure", "auto", "aces+denoise"])
def test_one_graded_frame_is_the_same_on_both_paths_and_differs_from_the_plain_one(tmp_path, models_dir, flags):
    args = _base(models_dir) + UP_AT_THE_LIGHT + ["-OUT", "one.bmp"]
    host, device = _both(tmp_path, args + flags)
    assert device["one.bmp"] == host["one.bmp"]
    plain = tmp_path / "plain"
    plain.mkdir()
    _run(args + [f for f in flags if f in ("-DENOISE", 2)], plain)
    assert _files(plain)["one.bmp"] != host["one.bmp"]


def test_reference_tone_at_zero_stops_and_no_flag_at_all_are_the_resolve_chain(tmp_path, models_dir):
    W, H = 32, 24
    args = _base(models_dir) + UP_AT_THE_LIGHT + ["-OUT", "one.bmp"]
    runs = {}
    for tag, extra in (("none", []), ("reference", ["-TONE", "reference", "-EXPOSURE", 0]), ("device", ["-DEVICE_RESOLVE", 1]),
                       ("reference on the device", ["-TONE", "reference", "-DEVICE_RESOLVE", 1])):
        work = tmp_path / tag.replace(" ", "_")
        work.mkdir()
        _run(args + extra, work)
        runs[tag] = _files(work)["one.bmp"]
    # the same frame through the library: the session's accumulators, pt_resolve, the BMP writer
    g = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    g.set_camera(pt.look_at((-2.0, -5.0, -8.0), (0.0, 9.0, 0.0)))
    s, s2, c, _ = g.render_host(W, H, 4, 4, error=0.001, seed=42, want_stats=False)
    bgr, _ = pt.resolve(W, H, s, s2, c)
    ref = str(tmp_path / "ref.bmp")
    pt.write_bmp(ref, bgr)
    want = open(ref, "rb").read()
    for tag, got in runs.items():
        assert got == want, tag
    assert bgr.any()


def test_bad_grading_flags_are_refused(tmp_path, models_dir):
    for flags in (["-TONE", "filmic"], ["-AUTO_EXPOSURE", 1, "-PERCENTILE", 101], ["-AUTO_EXPOSURE", 1, "-KEY", -1], ["-TONE", "aces", "-ADAPT", -0.5]):
        r = _run(_base(models_dir) + ["-OUT", "x.bmp"] + flags, tmp_path, ok=False)
        assert r.returncode == 2 and "-TONE" in r.stderr and not glob.glob(str(tmp_path / "*.bmp"))
