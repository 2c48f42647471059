"""pt_render -TEXTURE on the GPU: the BMP is the Python path's resolve of the same frame of a handle with the same textures, on the host
path and under -DEVICE_RESOLVE 1; -TEXTURE mtl on a model written into tmp_path (an OBJ with vt lines, an MTL with map_Kd, a BMP)
equals the explicit list; the flag combines with -GLASS, -ENV, -DENOISE 3 and -FRAMES 2; a refused flag ends with status 2."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import environment_restatement as E
from glass_fuzz_scenes import MTL, _box, _room
from texture_scenes import write_bmp as _write_bmp

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
W, H, SPP, MRR = 48, 32, 4, 6


def _run(args, cwd, model_dir, outputs=("out.bmp",), status=0):
    base = ["--W", W, "--H", H, "-RPP", SPP, "-MRR", MRR, "-UPDATE", 0, "-QUIET", 1, "-ERR", -1, "-SEED", 42, "-MODEL_PATH", model_dir, "-OUT", "out.bmp"]
    cwd.mkdir(exist_ok=True)
    r = subprocess.run([EXE] + [str(a) for a in base + list(args)], cwd=cwd, capture_output=True, text=True, timeout=120)
    assert r.returncode == status, (r.returncode, r.stderr)
    return [open(cwd / o, "rb").read() for o in outputs] if status == 0 else r.stderr + r.stdout


def _python_bmp(sc, path):
    s, s2, c, _ = sc.render_host(W, H, SPP, MRR, error=-1.0, seed=42, want_stats=False)
    pt.write_bmp(path, pt.resolve(W, H, s, s2, c)[0])
    return open(path, "rb").read()


@pytest.fixture()
def model(tmp_path):
    """The glass tests' room with a box in it, every corner with a vt of its own (x + z, y - z scaled: outside [0, 1) and negative),
    map_Kd on the walls (1) and on the box (3), and the two pictures."""
    d = str(tmp_path) + "/"
    tris = _room() + _box((-2.5, -4.0, -8.0), (1.5, 0.0, -4.0), 3)
    open(d + "g.mtl", "w").write(MTL.replace("Kd 0.8 0.8 0.8\n", "Kd 0.8 0.8 0.8\nmap_Kd wall.bmp\n").replace("Kd 0.9 0.3 0.3\n", "Kd 0.9 0.3 0.3\nmap_Kd box.bmp\n"))
    p, q, r, _ = tris[0]
    n = np.cross(np.subtract(q, p), np.subtract(r, p))
    lines = ["mtllib g.mtl", "vn %.6f %.6f %.6f" % tuple(n / np.linalg.norm(n))]
    for i, (p, q, r, m) in enumerate(tris):
        for v in (p, q, r):
            lines += ["v %.6f %.6f %.6f" % tuple(v), "vt %.6f %.6f" % ((v[0] + v[2]) * 0.23, (v[1] - v[2]) * 0.23)]
        lines.append("usemtl %d" % m)
        lines.append("f " + " ".join("%d/%d%s" % (3 * i + k, 3 * i + k, "/1" if i == 0 else "") for k in (1, 2, 3)))
    open(d + "room.obj", "w").write("\n".join(lines) + "\n")
    rng = np.random.default_rng(3)
    _write_bmp(d + "wall.bmp", rng.integers(0, 256, (8, 8, 3), dtype=np.uint8))
    _write_bmp(d + "box.bmp", rng.integers(0, 256, (5, 3, 3), dtype=np.uint8))
    return d


def test_texture_writes_the_librarys_bytes_and_mtl_equals_the_explicit_list(tmp_path, model):
    name = ["-MODEL_NAME", "room.obj"]
    explicit = name + ["-TEXTURE", "1:%swall.bmp,3:%sbox.bmp" % (model, model)]
    host, = _run(explicit, tmp_path / "host", model)
    device, = _run(explicit + ["-DEVICE_RESOLVE", 1], tmp_path / "device", model)
    mtl, = _run(name + ["-TEXTURE", "mtl"], tmp_path / "mtl", model)
    plain, = _run(name, tmp_path / "plain", model)
    near, = _run(name + ["-TEXTURE", "1:%swall.bmp:nearest" % model, "-TEXTURE_GAMMA", 1], tmp_path / "near", model)
    sc = pt.Scene.load_obj(model, "room.obj", device=0)
    assert sc.map_kd() == ["", "wall.bmp", "", "box.bmp"] and sc.texcoords().min() < 0 and sc.texcoords().max() > 1
    mine = str(tmp_path / "python.bmp")
    assert _python_bmp(sc, mine) == plain
    sc.set_textures([pt.texture(1, pt.load_texture_bmp(model + "wall.bmp")), pt.texture(3, pt.load_texture_bmp(model + "box.bmp"))])
    assert _python_bmp(sc, mine) == host == device == mtl and host != plain
    sc.set_textures([pt.texture(1, pt.load_texture_bmp(model + "wall.bmp", 1.0), "nearest")])
    assert _python_bmp(sc, mine) == near and near != host
    sc.close()


def test_texture_combines_with_glass_an_environment_the_denoiser_and_two_frames(tmp_path, model):
    pic = np.random.default_rng(7).uniform(0.05, 1.5, (16, 32, 3)).astype(np.float32)
    pano = str(tmp_path / "pano.pfm")
    open(pano, "wb").write(E.pfm_bytes(pic))
    tex = ["-MODEL_NAME", "room.obj", "-TEXTURE", "mtl"]
    glass, = _run(tex + ["-GLASS", "2:1.5"], tmp_path / "glass", model)
    sc = pt.Scene.load_obj(model, "room.obj", device=0)
    sc.set_textures([pt.texture(1, pt.load_texture_bmp(model + "wall.bmp")), pt.texture(3, pt.load_texture_bmp(model + "box.bmp"))])
    sc.set_dielectrics([pt.dielectric(2, 1.5)])
    assert _python_bmp(sc, str(tmp_path / "python.bmp")) == glass
    sc.set_dielectrics(None)
    sc.set_environment(pic, size=16)
    lit, = _run(tex + ["-ENV", pano, "-ENV_SIZE", 16], tmp_path / "env", model)
    assert _python_bmp(sc, str(tmp_path / "python.bmp")) == lit
    sc.close()
    for flags in (["-DENOISE", 3], ["-FRAMES", 2, "-EYE", "0,0,-20", "-LOOKAT", "0,0,0", "-EYE_END", "1,0,-20", "-LOOKAT_END", "0,0,0"]):
        with_tex = _run(tex + flags, tmp_path / ("t" + flags[0]), model)
        assert with_tex == _run(tex + flags + ["-DEVICE_RESOLVE", 1], tmp_path / ("d" + flags[0]), model)
        assert with_tex != _run(["-MODEL_NAME", "room.obj"] + flags, tmp_path / ("p" + flags[0]), model)


def test_every_refusal_ends_with_status_2(tmp_path, model):
    name = ["-MODEL_NAME", "room.obj"]
    wall = model + "wall.bmp"
    for flags, message in ((["-TEXTURE", "1"], "-TEXTURE takes"), (["-TEXTURE", "1:" + model + "none.bmp"], "cannot open"),
                           (["-TEXTURE", "9:" + wall], "outside the scene"), (["-TEXTURE", "2:" + wall, "-GLASS", "2:1.5"], "is a dielectric")):
        assert message in _run(name + flags, tmp_path / "refused", model, status=2), flags
