"""Albedo textures on the host (pt_hip.h: pt_texture; no GPU): the restated lookup (tests/texture_restatement.py) against the library's
own (pt.texture_lookup) bit for bit, its exact properties, the loader's vt and map_Kd, the BMP decode, the interface on host-only
scenes with every refusal in both orders against the dielectric list, pt_render's -TEXTURE parser, a frame composed with single errors
(the accumulators must tell each from the stated lookup), and the host code in a stand-alone program under AddressSanitizer + UBSan.

The per-triangle record of the barycentrics (pt_scene_get_texture_records) is compared with its restatement bit for bit, and every
scene the GPU tests render is composed here first: the share of pixels the oracle taints is asserted on the CPU."""
import importlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import texture_composition as TC
import texture_restatement as T
import texture_scenes as S
from texture_scenes import planar_uv

pt = importlib.import_module("path-tracing_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
PT_ERR_INVALID_ARGUMENT, PT_ERR_PARSE = 1, 3
SIZES = [(1, 1), (2, 2), (3, 5), (16, 16), (64, 64)]      # (w, h)
FILTERS = [("nearest", T.NEAREST), ("bilinear", T.BILINEAR)]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _texture(w, h, seed=0):
    return np.random.default_rng(seed).uniform(0.0, 2.0, (h, w, 3)).astype(F32)


def _coordinates(w, h):
    """Inside [0, 1); texel centres and edges; negative; 10^6, 2^30; the largest float below 1; -1e-9; NaN and the infinities."""
    rng = np.random.default_rng(7)
    one_m = np.nextafter(F32(1.0), F32(0.0))
    specials = np.array([0.0, -0.0, 0.5, one_m, 1.0, -1e-9, 1e-9, -1.0, -0.25, -7.75, 3.5, 1e6, -1e6, 1e6 + 0.25, 2.0 ** 30, -2.0 ** 30, 2.0 ** 23, 2.0 ** 23 - 0.5,
                         np.nan, np.inf, -np.inf, 1e38, -1e38, 1e-45], F32)
    centres_u, centres_v = (np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h
    edges_u, edges_v = np.arange(w + 1) / w, np.arange(h + 1) / h
    grid = [np.stack(np.meshgrid(a, b), -1).reshape(-1, 2) for a, b in ((centres_u, centres_v), (edges_u, edges_v), (specials, specials))]
    return np.concatenate([rng.uniform(0, 1, (500, 2)), rng.uniform(-40, 40, (500, 2))] + grid).astype(F32)


@pytest.mark.parametrize("name,filt", FILTERS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_restated_lookup_is_the_hosts_bit_for_bit_and_reads_inside(size, name, filt):
    w, h = size
    tex, uv = _texture(w, h), _coordinates(w, h)
    got, idx = pt.texture_lookup(tex, uv, name, want_indices=True)
    want_idx, _, _ = T.taps(w, h, uv, filt)
    assert idx.min() >= 0 and idx.max() < w * h and want_idx.min() >= 0 and want_idx.max() < w * h
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(_bits(got), _bits(T.lookup(tex, uv, filt)))
    assert np.isfinite(got).all()                       # no NaN the texels do not hold


def test_what_the_stated_special_coordinates_read():
    tex = _texture(3, 5)
    bad = np.array([[np.nan, np.nan], [np.inf, -np.inf], [-1e-9, -1e-9], [2.0 ** 30, -2.0 ** 30]], F32)
    near, idx = pt.texture_lookup(tex, bad, "nearest", want_indices=True)
    assert (idx == (5 - 1) * 3).all() and np.array_equal(_bits(near), _bits(np.tile(tex[4, 0], (4, 1))))      # the bottom-left texel
    _, idx = pt.texture_lookup(tex, bad, "bilinear", want_indices=True)
    # the four corners: the lower texel of either axis wraps to the last one (column 2; v's last texel is picture row 0), the upper one is texel 0
    assert (idx == [0 * 3 + 2, 0 * 3 + 0, 4 * 3 + 2, 4 * 3 + 0]).all()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_bilinear_at_a_texel_centre_is_the_texel_and_v_points_up(size):
    w, h = size
    tex = _texture(w, h, 1)
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    uv = np.stack([(xs.ravel() + 0.5) / w, (ys.ravel() + 0.5) / h], 1).astype(F32)
    # the centres the float coordinate hits exactly (all of them for sides that are powers of two)
    exact = ((uv[:, 0] * F32(w) - F32(0.5)) == xs.ravel()) & ((uv[:, 1] * F32(h) - F32(0.5)) == ys.ravel())
    assert exact.any() and (exact.all() or (w, h) == (3, 5))
    want = tex[h - 1 - ys.ravel(), xs.ravel()]           # row 0 is the top of the picture: v = 1
    for name in ("bilinear", "nearest"):
        got = pt.texture_lookup(tex, uv, name)
        assert np.array_equal(_bits(got[exact]), _bits(want[exact])), name
    assert np.array_equal(_bits(pt.texture_lookup(tex, uv, "nearest")), _bits(want))


@pytest.mark.parametrize("name,filt", FILTERS)
def test_a_constant_texture_gives_its_constant_and_the_lookup_has_period_1(name, filt):
    uv = _coordinates(16, 16)
    for w, h in SIZES:
        const = np.empty((h, w, 3), F32)
        const[:] = np.array([0.3, 1.7, 0.0], F32)
        assert np.array_equal(_bits(pt.texture_lookup(const, uv, name)), _bits(np.tile(const[0, 0], (len(uv), 1)))), (w, h)
        tex = _texture(w, h, 2)
        base = (np.random.default_rng(3).integers(-256, 256, (400, 2)) / 256.0).astype(F32)      # multiples of 2^-8: base + k is exact
        ref = pt.texture_lookup(tex, base, name)
        for k in (1.0, -1.0, 5.0, -1024.0):
            assert np.array_equal(_bits(pt.texture_lookup(tex, base + F32(k), name)), _bits(ref)), (w, h, k)


# ---- loader, BMP decode ---------------------------------------------------------------------------------------------------------------
_write_bmp = S.write_bmp


MTL = "newmtl 0\nKe 3 3 3\nKd 1 1 1\nmap_Kd lamp.bmp\nnewmtl 1\nNs 0\nKd 0.8 0.8 0.8\nnewmtl 2\nNs 300\nKs 0.7 0.7 0.7\nKd 0.6 0.6 0.9\nmap_Kd wall.bmp\n"
OBJ = ("mtllib t.mtl\nvn 0 0 -1\nv -1 -1 5\nv 1 -1 5\nv 1 1 5\nv -1 1 5\nvt 0 0\nvt 2 0\nvt 2 -3\nvt 0.25 0.75\n"
       "usemtl 2\nf 1/1/1 2/2/1 3/3/1\nusemtl 1\nf 1/4 3 4/2\nusemtl 0\nf 1//1 2//1 4//1\n")


@pytest.fixture()
def trio(tmp_path):
    d = str(tmp_path) + "/"
    open(d + "t.mtl", "w").write(MTL)
    open(d + "t.obj", "w").write(OBJ)
    bgr = np.random.default_rng(5).integers(0, 256, (5, 3, 3), dtype=np.uint8)
    _write_bmp(d + "wall.bmp", bgr)
    return d, bgr


def test_the_loader_keeps_each_corners_vt_and_the_map_kd_names(trio):
    d, bgr = trio
    s = pt.Scene.load_obj(d, "t.obj", device=-1)
    want = np.array([[[0, 0], [2, 0], [2, -3]], [[0.25, 0.75], [0, 0], [2, 0]], [[0, 0], [0, 0], [0, 0]]], F32)
    assert np.array_equal(s.texcoords(), want) and s.textures() == []
    assert s.map_kd() == ["lamp.bmp", "", "wall.bmp"]
    s.close()
    open(d + "bad.obj", "w").write(OBJ.replace("f 1/4 3 4/2", "f 1/5 3 4/2"))
    with pytest.raises(pt.PtError) as e:
        pt.Scene.load_obj(d, "bad.obj", device=-1)
    assert e.value.status == PT_ERR_PARSE and "texture coordinate 5 of 4" in str(e.value)
    for gamma in (2.2, 1.0, 0.45):
        got = pt.load_texture_bmp(d + "wall.bmp", gamma)
        assert got.shape == (5, 3, 3) and np.array_equal(_bits(got), _bits(T.decode_table(gamma)[bgr[:, :, ::-1]])), gamma
    assert np.array_equal(_bits(T.decode_table(1.0)), _bits((np.arange(256) / 255.0).astype(F32)))
    with pytest.raises(pt.PtError):
        pt.load_texture_bmp(d + "none.bmp")
    with pytest.raises(pt.PtError):
        pt.load_texture_bmp(d + "t.obj")
    created = pt.Scene.create(*_tiny_scene(), device=-1)      # a scene made from arrays has no coordinates until it is given some
    assert created.texcoords() is None and created.map_kd() == ["", ""]
    created.close()


def _tiny_scene():
    tri = np.zeros((2, 14), F32)
    tri[0, 4:13] = [0, 0, 5, 1, 0, 5, 0, 1, 5]
    tri[1, 4:13] = [0, 0, 6, 1, 0, 6, 2, 0, 6]          # collinear
    tri[:, 0:4] = [0, 0, -1, 5]
    mats = np.zeros((2, 10), F32)
    mats[0, 3:6] = 1
    mats[1, 0:3] = 0.5
    return tri, np.array([0, 1], np.int32), mats


# ---- the interface and its refusals ---------------------------------------------------------------------------------------------------
def _state(s):
    return ([(t.material, t.filter, t.texels.tobytes()) for t in s.textures()], None if s.texcoords() is None else s.texcoords().tobytes(),
            [(e.material, e.ior) for e in s.dielectrics()])


def test_the_interface_on_a_host_only_scene_and_every_refusal(models_dir):
    s = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    n_tri, n_mat = s.counts()
    assert s.texcoords().shape == (n_tri, 3, 2) and not s.texcoords().any()      # Tor.obj has no vt lines: (0, 0) everywhere
    uv = np.random.default_rng(0).uniform(-2, 3, (n_tri, 3, 2)).astype(F32)
    s.set_texcoords(uv)
    a, b = _texture(3, 5), _texture(1, 1, 9)
    s.set_textures([pt.texture(1, a, "nearest"), pt.texture(3, b)])
    s.set_dielectrics([pt.dielectric(4, 1.5)])
    kept = _state(s)
    assert [(m, f) for m, f, _ in kept[0]] == [(1, 0), (3, 1)] and kept[0][0][2] == a.tobytes() and kept[1] == uv.tobytes()
    bad_texel = a.copy(); bad_texel[2, 1, 0] = -0.5
    nan_texel = a.copy(); nan_texel[0, 0, 2] = np.nan
    inf_texel = a.copy(); inf_texel[4, 2, 1] = np.inf
    refused = [[pt.texture(n_mat, a)], [pt.texture(-1, a)], [pt.texture(1, a), pt.texture(1, b)], [pt.texture(1, bad_texel)], [pt.texture(1, nan_texel)],
               [pt.texture(1, inf_texel)], [pt.texture(1, a, 2)], [pt.texture(1, a, -1)], [pt.texture(2, a), pt.texture(4, b)],      # 4 is a dielectric
               [pt.texture(1, np.zeros((1, pt.TEXTURE_MAX_SIDE + 1, 3), F32))], [pt.texture(1, np.zeros((0, 4, 3), F32))]]
    for bad in refused:
        with pytest.raises(pt.PtError) as e:
            s.set_textures(bad)
        assert e.value.status == PT_ERR_INVALID_ARGUMENT and _state(s) == kept, bad
    with pytest.raises(pt.PtError) as e:                  # the other order: a textured material cannot become a dielectric
        s.set_dielectrics([pt.dielectric(4, 1.5), pt.dielectric(3, 1.5)])
    assert e.value.status == PT_ERR_INVALID_ARGUMENT and "textured" in str(e.value) and _state(s) == kept
    with pytest.raises(pt.PtError) as e:                  # the coordinates cannot go while a list is set
        s.set_texcoords(None)
    assert e.value.status == PT_ERR_INVALID_ARGUMENT and _state(s) == kept
    L = s._L
    arr = (pt.TextureEntry * 1)(pt.TextureEntry(1, 3, 5, 0, a.ctypes.data_as(pt.C.POINTER(pt.C.c_float))))
    assert L.pt_scene_set_textures(s._h, arr, -1) == PT_ERR_INVALID_ARGUMENT and L.pt_scene_set_textures(s._h, None, 1) == PT_ERR_INVALID_ARGUMENT
    assert L.pt_scene_set_textures(None, arr, 1) == PT_ERR_INVALID_ARGUMENT and L.pt_scene_set_texcoords(None, None) == PT_ERR_INVALID_ARGUMENT
    arr[0].rgb = None
    assert L.pt_scene_set_textures(s._h, arr, 1) == PT_ERR_INVALID_ARGUMENT and _state(s) == kept
    clone = s.clone_to_device(-1)                          # a clone inherits both; changing it leaves the original alone
    assert _state(clone) == kept
    clone.set_textures(None)
    clone.set_texcoords(None)
    assert clone.textures() == [] and clone.texcoords() is None and _state(s) == kept
    with pytest.raises(pt.PtError) as e:                  # a list on a handle without coordinates
        clone.set_textures([pt.texture(1, a)])
    assert e.value.status == PT_ERR_INVALID_ARGUMENT
    clone.close()
    s.set_textures([])                                     # cleared: now 3 may become a dielectric, and then cannot be textured
    s.set_dielectrics([pt.dielectric(3, 1.5)])
    with pytest.raises(pt.PtError) as e:
        s.set_textures([pt.texture(3, a)])
    assert e.value.status == PT_ERR_INVALID_ARGUMENT and "dielectric" in str(e.value) and s.textures() == []
    s.set_textures([pt.texture(0, b)])                     # the emitter may be textured
    s.close()


def test_pt_render_refuses_a_bad_texture_flag(trio, models_dir):
    d, _ = trio
    exe = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
    model = ["-MODEL_PATH", models_dir, "-MODEL_NAME", "Tor.obj"]
    wall = d + "wall.bmp"
    cases = [(["-TEXTURE", "1"], "-TEXTURE takes"), (["-TEXTURE", "1:"], "-TEXTURE takes"), (["-TEXTURE", "x:" + wall], "-TEXTURE takes"),
             (["-TEXTURE", ":" + wall], "-TEXTURE takes"), (["-TEXTURE", "-1:" + wall], "-TEXTURE takes"), (["-TEXTURE", "1.5:" + wall], "-TEXTURE takes"),
             (["-TEXTURE", "1:" + wall + ","], "-TEXTURE takes"), (["-TEXTURE", "1:" + wall + ":nearest,2"], "-TEXTURE takes"), (["-TEXTURE", "1::bilinear"], "-TEXTURE takes"),
             (["-TEXTURE", "1:" + d + "none.bmp"], "cannot open"), (["-TEXTURE", "1:" + d + "t.obj"], "invalid type value"),
             (["-TEXTURE", "1:" + wall + ":cubic"], "cannot open"),                       # (an unknown filter name is part of the file name)
             (["-TEXTURE", "7:" + wall], "outside the scene"), (["-TEXTURE", "1:" + wall + ",1:" + wall], "listed twice"),
             (["-TEXTURE", "4:" + wall, "-GLASS", "4:1.5"], "is a dielectric"), (["-TEXTURE_GAMMA", "2.2"], "needs -TEXTURE"),
             (["-TEXTURE", "1:" + wall, "-TEXTURE_GAMMA", "0"], "-TEXTURE_GAMMA takes"), (["-TEXTURE", "1:" + wall, "-TEXTURE_GAMMA", "x"], "-TEXTURE_GAMMA takes")]
    for flags, message in cases:
        run = subprocess.run([exe] + model + flags, capture_output=True, text=True, cwd=d, timeout=60)
        assert run.returncode == 2 and message in run.stderr + run.stdout, (flags, run.returncode, run.stderr)


# ---- the composition tells a wrong lookup from the right one ---------------------------------------------------------------------------
def test_a_frame_tells_each_single_error_from_the_stated_lookup_and_no_pixel_is_tainted(oracle_scene):
    W, H, SPP, MRR = 40, 28, 8, 8
    tri, _ = oracle_scene.triangles()
    uv = planar_uv(tri)
    mats = oracle_scene.materials()
    diffuse_and_glossy = [m for m in range(oracle_scene.n_mat) if mats[m, 9] != 0 and mats[m, 6:9].any() and not mats[m, 3:6].any()]
    assert diffuse_and_glossy                              # (else the glossy error cannot show)
    textures = {m: (_texture(3, 5, 10 + m), T.BILINEAR) for m in range(oracle_scene.n_mat)}
    px = np.array([(x, y) for y in range(H) for x in range(W)])
    tally = {}
    right = TC.compose(oracle_scene, textures, uv, None, None, W, H, px, SPP, MRR, stats=tally)
    assert tally["tainted"].mean() == 0.0                  # Tor.obj: measured 0, cap 2 %
    plain = TC.compose(oracle_scene, None, uv, None, None, W, H, px, SPP, MRR)
    assert not np.array_equal(_bits(right[0]), _bits(plain[0]))
    for errors in (dict(flip_v=False), dict(glossy_too=True), dict(swap_b=True), dict(clamp=True)):
        wrong = TC.compose(oracle_scene, textures, uv, None, None, W, H, px, SPP, MRR, errors=errors)
        assert not np.array_equal(_bits(wrong[0]), _bits(right[0])), errors
    ones = {m: (np.ones((2, 2, 3), F32), T.NEAREST) for m in range(oracle_scene.n_mat)}      # an all-ones texture changes nothing
    same = TC.compose(oracle_scene, ones, uv, None, None, W, H, px, SPP, MRR)
    assert all(np.array_equal(_bits(a) if a.dtype == F32 else a, _bits(b) if b.dtype == F32 else b) for a, b in zip(same, plain))


# ---- the per-triangle record ----------------------------------------------------------------------------------------------------------
def test_the_barycentric_record_is_its_restatement_bit_for_bit(models_dir):
    s = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    tri, _ = s.triangles()
    assert np.array_equal(_bits(s.texture_records()), _bits(T.bary_records(tri)))
    s.close()
    tri = S.sliver_scene()                                  # slivers of aspect up to 10^6 and one collinear triangle
    s = pt.Scene.create(tri, np.zeros(len(tri), np.int32), np.zeros((1, 10), F32), device=-1)
    got, want = s.texture_records(), T.bary_records(tri)
    assert np.array_equal(_bits(got), _bits(want)) and not got[40].any()
    assert got[:40].any(axis=1).sum() >= 30                 # (the thinnest slivers' den rounds to 0 too: the zero record, as stated)
    s.close()
    # what the record is for: at the corners b = (0, 0), (1, 0), (0, 1), within the rounding of a well-shaped triangle's record
    tri, _ = O.Scene.load(models_dir, "Tor.obj").triangles()
    rec = T.bary_records(tri)
    for k, (w1, w2) in enumerate(((0, 0), (1, 0), (0, 1))):
        b1, b2 = T.barycentrics(rec, tri[:, 4 + 3 * k:7 + 3 * k])
        assert np.abs(b1 - w1).max() < 1e-3 and np.abs(b2 - w2).max() < 1e-3, k


# ---- every scene of the GPU tests stays under the taint cap with the composition alone -------------------------------------------------
def _taint(osc, textures, uv, w, h, px=None, env=None, **kw):
    tally = {}
    TC.compose(osc, textures, uv, None, env, w, h, S.all_pixels(w, h) if px is None else px, 4, 8, stats=tally, **kw)
    return tally["tainted"].mean()


def test_the_chosen_scenes_stay_under_the_taint_cap(models_dir, tmp_path):
    d = str(tmp_path) + "/"
    osc, uv = S.tor(models_dir)
    _, _, _, room, room_uv = S.room(d)
    for w, h in ((32, 16), (24, 20), (17, 9)):
        assert _taint(osc, S.TOR_TWO, uv, w, h) == 0.0                                   # Tor.obj: expected and measured 0
        assert _taint(room, S.room_textures(3, 5, T.BILINEAR), room_uv, w, h) == 0.0       # the closed room: expected and measured 0
    for view in S.VIEWS:
        kw = S.set_view(pt, None, view, 24, 20)
        assert _taint(osc, S.TOR_TWO, uv, 24, 20, **kw) <= S.TAINT_CAP, view
        assert _taint(room, S.room_textures(1, 1, T.NEAREST), room_uv, 24, 20, **kw) <= S.TAINT_CAP, view
    opened, open_uv = S.open_tor(d)
    for view in S.VIEWS:
        assert _taint(opened, S.TOR_TWO, open_uv, 24, 20, env=S.env_map(3), **S.set_view(pt, None, view, 24, 20)) <= S.TAINT_CAP, view
    big, big_uv, big_tex = S.box_tree(d)
    px = S.all_pixels(24, 20)[::3]
    assert _taint(big, big_tex, big_uv, 24, 20, px=px) <= S.TAINT_CAP
    assert _taint(big, big_tex, big_uv, 24, 20, px=px, **S.set_view(pt, None, "camera", 24, 20)) <= S.TAINT_CAP


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"), reason="g++ or the HIP headers are not available")
def test_the_host_code_is_clean_under_asan_and_ubsan(trio):
    """pt_texture_capi.cpp and pt_scene.cpp with a stand-alone main, on host-only handles: the setters with every refusal, the frame's
    setters, the lookup at the special coordinates, the BMP decode and the MTL's map_Kd reader.  Host code only, a program of its own."""
    d, _ = trio
    exe = d + "texture_san"
    csrc = os.path.join(ROOT, "path-tracing_amd", "csrc")
    build = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                            os.path.join(ROOT, "tests", "native", "texture_sanitizer_main.cpp"), os.path.join(csrc, "pt_texture_capi.cpp"),
                            os.path.join(csrc, "pt_scene.cpp"), "-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-ldl", "-lpthread", "-Wl,-rpath,/opt/rocm/lib"],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")      # (the HIP runtime's own start-up allocations are not ours to judge)
    run = subprocess.run([exe, d], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    assert "texture host ok" in run.stdout
