"""pt_render -DEVICE_RESOLVE 1: the images' bytes come from the display path on the device, and every file is byte-identical to
the one the host path writes."""
import glob
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")


def _run(args, cwd):
    r = subprocess.run([EXE] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def _files(work):
    return {os.path.basename(p): open(p, "rb").read() for p in glob.glob(str(work / "*.bmp"))}


def _both(tmp_path, args):
    """The same command without and with the flag, each in a directory of its own: name -> bytes of every BMP written, and stderr."""
    out = []
    for tag, extra in (("host", []), ("device", ["-DEVICE_RESOLVE", 1])):
        work = tmp_path / tag
        work.mkdir()
        r = _run(args + extra, work)
        out.append((_files(work), r.stderr))
    return out


def _base(models_dir):
    return ["--W", 64, "--H", 48, "-RPP", 4, "-UPDATE", 0, "-QUIET", 1, "-SEED", 42, "-MODEL_PATH", models_dir]


def test_sequence_with_temporal_and_denoise(tmp_path, models_dir):
    args = _base(models_dir) + ["-FRAMES", 3, "-EYE", "0,0,-20", "-EYE_END", "4,1,-18", "-TEMPORAL", 8, "-DENOISE", 2, "-OUT", "last.bmp"]
    (host, _), (device, err) = _both(tmp_path, args)
    assert sorted(host) == ["frame_0000.bmp", "frame_0001.bmp", "frame_0002.bmp", "last.bmp"]
    assert sorted(device) == sorted(host)
    for name in host:
        assert device[name] == host[name], name
    assert host["frame_0000.bmp"] != host["frame_0002.bmp"]
    assert "ignored" not in err


@pytest.mark.parametrize("extra", [[], ["-DENOISE", 2], ["-FRAMES", 2, "-EYE", "1,0,-20"]], ids=["plain", "denoise", "frames"])
def test_one_frame_without_stages_and_variants(tmp_path, models_dir, extra):
    (host, _), (device, _) = _both(tmp_path, _base(models_dir) + extra + ["-OUT", "one.bmp"])
    assert "one.bmp" in host and sorted(device) == sorted(host)
    for name in host:
        assert device[name] == host[name], name


def test_gauss_keeps_the_host_path(tmp_path, models_dir):
    (host, _), (device, err) = _both(tmp_path, _base(models_dir) + ["-GAUSS", 1, "-OUT", "g.bmp"])
    assert device["g.bmp"] == host["g.bmp"]
    assert "-DEVICE_RESOLVE is ignored" in err
    plain = tmp_path / "plain"
    plain.mkdir()
    _run(_base(models_dir) + ["-OUT", "g.bmp"], plain)
    assert _files(plain)["g.bmp"] != host["g.bmp"]          # the filter did act
