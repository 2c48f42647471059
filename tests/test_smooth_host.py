"""Smooth shading on the host (pt_hip.h: smooth shading): pt.shading_normal_at against tests/smooth_restatement.py bit for bit at
corners, edges, centres, far outside, with zero and cancelling normals, on a collinear triangle and at NaN and infinite points; the
normal generator on Tor.obj against a numpy generator; the loader's vn and PT_LOAD_GEOMETRIC_PLANES; every refusal and the round trip
on scene and frame handles (host-only); the host code under ASan + UBSan as a program of its own; and the composition: every frame the
GPU test renders is composed here first and marks no pixel tainted, and a frame tells each of five single errors from the stated step."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import smooth_composition as SC
import smooth_restatement as SR
import smooth_scenes as SS
import texture_restatement as T
import texture_scenes as S

pt = importlib.import_module("path-tracing_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

OBJ = ("mtllib n.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nvn 0 0 2\nvn 1 0 1\nvn 0 1 1\n"
       "usemtl 0\nf 1//1 2//2 3\nf 2//3 4/7 3//0\n")
MTL = "newmtl a\nKd 0.5 0.5 0.5\n"


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("smooth")) + "/"
    open(d + "n.mtl", "w").write(MTL)
    open(d + "n.obj", "w").write(OBJ)
    open(d + "bad.obj", "w").write(OBJ.replace("f 2//3 4/7 3//0", "f 2//3 4/7 3//4"))
    open(d + "back.obj", "w").write("mtllib n.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0.6 -0.8\nusemtl 0\nf 1//1 2//1 3//1\nf 1 2 3\n")
    open(d + "plain.obj", "w").write("mtllib n.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nusemtl 0\nf 1 2 3\n")
    return d


@pytest.fixture(scope="module")
def tor(models_dir):
    osc, uv = S.tor(models_dir)
    return osc, uv, SS.tor_normals(osc)


def test_shading_normal_at_equals_the_restatement_bit_for_bit():
    rng = np.random.default_rng(1)
    nan, inf = np.nan, np.inf
    for case in range(8):
        v = rng.uniform(-5, 5, (3, 3)).astype(F32)
        if case == 6:
            v = np.array([[-3, 1, -3], [0, 2, -3], [3, 3, -3]], F32)             # collinear: the zero record
        N = np.cross(v[1] - v[0], v[2] - v[0]) if case != 6 else np.array([0, 0, -1.0])
        N = (N / np.linalg.norm(N)).astype(F32)
        n9 = (N + rng.normal(size=(3, 3)) * 0.6).astype(F32)
        if case == 3:
            n9[:] = 0                                                           # "use N"
        if case == 4:
            n9[1], n9[2] = -n9[0], n9[0] * 0                                    # opposing normals cancel on an edge
        if case == 5:
            n9 = -n9                                                            # the flip
        b = rng.uniform(-0.2, 1.2, (40, 2))
        pts = [v[0], v[1], v[2], (v[0] + v[1]) / 2, (v[1] + v[2]) / 2, v.mean(0), v[0] + 1e5 * (v[1] - v[0]), [nan, 0, 0], [inf, 0, 0], [-inf, inf, 1], [3e38, 3e38, 3e38]]
        pts += [v[0] + x * (v[1] - v[0]) + y * (v[2] - v[0]) for x, y in b]
        pts = np.array(pts, F32)
        tri = np.zeros((1, 14), F32)
        tri[0, 0:3], tri[0, 4:13] = N, v.ravel()
        got, own = pt.shading_normal_at(v, N, n9, pts, want_interpolated=True)
        want, usable = SR.normal_at(tri, n9[None], np.zeros(len(pts), np.int64), pts)
        assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(own, usable), case
        assert own.any() != (case in (3,)) or case == 6


def test_the_generator_on_tor(tor):
    osc, _, want = tor
    tri, tri_mat = osc.triangles()
    n9 = pt.smooth_normals(tri)
    assert np.abs(n9 - want).max() <= 1e-6
    assert np.abs(np.linalg.norm(n9, axis=2) - 1).max() <= 1e-6
    torus = tri_mat == 4
    verts = tri[:, 4:13].reshape(-1, 3, 3)
    seen = {}
    for t in np.nonzero(torus)[0]:
        for k in range(3):
            key = verts[t, k].tobytes()
            assert np.array_equal(seen.setdefault(key, n9[t, k]), n9[t, k])      # one welded torus vertex, one normal
    assert len(seen) < 3 * torus.sum() / 3
    c = np.cross(verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]).astype(np.float64)
    fn = c / np.linalg.norm(c, axis=1, keepdims=True)
    assert np.abs(n9[~torus] - fn[~torus, None]).max() <= 1e-6                   # every wall corner: its face normal at 60 degrees
    assert np.abs(n9[torus] - fn[torus, None]).max() > 0.05                      # the torus is rounded
    assert np.abs(pt.smooth_normals(tri, 0.0) - fn[:, None]).max() <= 1e-6       # crease 0: face normals everywhere
    all_ = pt.smooth_normals(tri, 180.0)
    assert np.abs(all_ - SS.tor_normals(osc, 180.0)).max() <= 1e-6
    seen = {}
    for t in range(len(tri)):
        for k in range(3):
            assert np.array_equal(seen.setdefault(verts[t, k].tobytes(), all_[t, k]), all_[t, k])      # crease 180 welds everything
    with pytest.raises(pt.PtError):
        pt.smooth_normals(tri, 181.0)


def test_the_loader_keeps_three_vn_per_face(files, models_dir):
    sc = pt.Scene.load_obj(files, "n.obj", device=-1)
    vn, tri = sc.vertex_normals(), sc.triangles()[0]
    assert np.array_equal(vn[0], [[0, 0, 2], [1, 0, 1], tri[0, 0:3]])            # a missing index: the stored normal
    assert np.array_equal(vn[1], [[0, 1, 1], tri[1, 0:3], tri[1, 0:3]])          # a zero index likewise
    assert np.allclose(tri[1, 0:3], np.array([0, 1, 1]) / np.sqrt(2)) and sc.shading_normals() is None     # the reference's plane: the first corner's vn
    geo = pt.Scene.load(files, "n.obj", device=-1, geometric_planes=True)
    assert np.array_equal(geo.triangles()[0][:, 0:3], [[0, 0, 1], [0, 0, 1]]) and np.array_equal(geo.vertex_normals()[0, :2], vn[0, :2])
    back = pt.Scene.load(files, "back.obj", device=-1, geometric_planes=True)   # wound against its vn: the cross product, on the vn's side
    assert np.array_equal(back.triangles()[0][:, 0:4], [[0, 0, -1, 0], [0, 0, 1, 0]])
    assert np.array_equal(back.triangles()[0][:, 4:], pt.Scene.load_obj(files, "back.obj", device=-1).triangles()[0][:, 4:])
    with pytest.raises(pt.PtError) as e:
        pt.Scene.load_obj(files, "bad.obj", device=-1)
    assert e.value.status == 3                                                   # PT_ERR_PARSE
    plain = pt.Scene.load_obj(files, "plain.obj", device=-1)
    assert np.array_equal(plain.vertex_normals()[0], np.repeat(plain.triangles()[0][:, 0:3], 3, 0))
    assert pt.Scene.create(tri, sc.triangles()[1], np.zeros((1, 10), F32), device=-1).vertex_normals() is None
    tor_ = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    assert tor_.vertex_normals().shape == (tor_.counts()[0], 3, 3)


def test_the_tools_scene_keeps_every_face_on_its_side_and_names_the_generators_normals(tmp_path, models_dir):
    """tools/make_smooth_scene.py: TorSmooth.obj under PT_LOAD_GEOMETRIC_PLANES faces as Tor.obj does, the lamp included (Tor.obj winds it
    against its vn), and its torus corners name the generator's normals."""
    import make_smooth_scene as MS                                               # (tests/smooth_scenes.py put tools/ on the path)
    d = str(tmp_path) + "/"
    MS.generate(models_dir, d)
    ref = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    geo = pt.Scene.load_obj(d, "TorSmooth.obj", device=-1, geometric_planes=True)
    (tri, tri_mat), (gtri, gmat) = ref.triangles(), geo.triangles()
    assert np.array_equal(tri[:, 4:13], gtri[:, 4:13]) and np.array_equal(tri_mat, gmat)
    assert ((tri[:, 0:3] * gtri[:, 0:3]).sum(1) > 0.999).all()
    c = np.cross(tri[:, 7:10] - tri[:, 4:7], tri[:, 10:13] - tri[:, 4:7])
    against = (c * tri[:, 0:3]).sum(1) < 0
    assert against.any() and set(tri_mat[against]) == {0}                        # the lamp is what the orientation rule is for
    vn, torus = geo.vertex_normals(), tri_mat == 4
    assert np.array_equal(_bits(vn[torus]), _bits(SS.numpy_normals(tri[torus, 4:13])))
    assert np.array_equal(_bits(vn[~torus]), _bits(ref.vertex_normals()[~torus]))
    assert ((vn * gtri[:, None, 0:3]).sum(2) > 0).all()                          # every corner's normal on its plane's side


def test_refusals_and_the_round_trip(files):
    sc = pt.Scene.load_obj(files, "n.obj", device=-1)
    n9 = np.arange(18, dtype=F32).reshape(2, 3, 3)
    sc.set_shading_normals(n9)
    assert np.array_equal(sc.shading_normals(), n9)
    for bad in (np.nan, np.inf, -np.inf):
        b = n9.copy()
        b[1, 2, 1] = bad
        with pytest.raises(pt.PtError) as e:
            sc.set_shading_normals(b)
        assert e.value.status == 1 and np.array_equal(sc.shading_normals(), n9)  # PT_ERR_INVALID_ARGUMENT; nothing changed
    with pytest.raises(ValueError):
        sc.set_shading_normals(n9[:1])
    sc.set_shading_normals(np.zeros_like(n9))                                    # zeros are allowed
    sc.set_shading_normals(None)
    assert sc.shading_normals() is None
    L = pt.lib()
    assert L.pt_scene_set_shading_normals(None, None) == 1 and L.pt_frame_set_shading_normals(None, None) == 1
    assert L.pt_shading_normal_at(None, None, None, 0, None, None, None) == 1


EXE = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")


@pytest.mark.parametrize("flags", [["-SMOOTH", "yes"], ["-SMOOTH", "AUTO"], ["-SMOOTH", "auto", "-CREASE", "181"], ["-SMOOTH", "auto", "-CREASE", "-1"],
                                   ["-SMOOTH", "auto", "-CREASE", "x"], ["-SMOOTH", "vn", "-CREASE", "30"], ["-CREASE", "30"]])
def test_the_parser_ends_with_status_2(flags, models_dir):
    assert os.path.exists(EXE), "pt_render is not built: the build is broken, the parser is not checked"   # (refused before any HIP call)
    r = subprocess.run([EXE, "--W", "8", "--H", "8", "-RPP", "1", "-MODEL_PATH", models_dir, "-QUIET", "1"] + flags, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stderr)


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"), reason="g++ or the HIP headers are not available")
def test_the_host_code_is_clean_under_asan_and_ubsan(files):
    """pt_smooth_capi.cpp, pt_smooth_normals.cpp and pt_scene.cpp with a stand-alone main, on host-only handles.  Host code only."""
    exe = files + "smooth_san"
    csrc = os.path.join(ROOT, "path-tracing_amd", "csrc")
    build = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                            os.path.join(ROOT, "tests", "native", "smooth_sanitizer_main.cpp"), os.path.join(csrc, "pt_smooth_capi.cpp"),
                            os.path.join(csrc, "pt_smooth_normals.cpp"), os.path.join(csrc, "pt_scene.cpp"), "-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-ldl",
                            "-lpthread", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")      # (the HIP runtime's own start-up allocations are not ours to judge)
    run = subprocess.run([exe, files], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    assert "smooth host ok" in run.stdout


def _compose(osc, n9, uv, w, h, spp, mrr, **kw):
    kw.pop("stats", None)
    tally = {}
    out = SC.compose(osc, n9, kw.pop("textures", None), uv, kw.pop("glass", None), kw.pop("env", None), w, h, kw.pop("px", S.all_pixels(w, h)), spp, mrr, stats=tally, **kw)
    return out, tally


@pytest.mark.parametrize("name", list(SS.TOR_FRAMES))
def test_every_tor_frame_of_the_gpu_test_composes_without_a_tainted_pixel(tor, name):
    osc, uv, n9 = tor
    (w, h), spp, mrr, kw = SS.TOR_FRAMES[name]
    _, tally = _compose(osc, n9, uv, w, h, spp, mrr, **dict(kw))
    assert not tally["tainted"].any() and tally["smooth_steps"] > 0
    if name == "glass":
        assert min(tally["events"].values()) > 0, tally["events"]


@pytest.mark.parametrize("view", SS.VIEWS)
def test_every_view_composes_without_a_tainted_pixel(tor, view):
    osc, uv, n9 = tor
    _, tally = _compose(osc, n9, uv, 40, 28, 4, 3, **S.set_view(pt, None, view, 40, 28))
    assert not tally["tainted"].any() and tally["smooth_steps"] > 0


def test_a_frame_tells_each_single_error_from_the_stated_step(tor):
    osc, uv, n9 = tor
    W, H, SPP = 40, 28, 8
    good, tally = _compose(osc, n9, uv, W, H, SPP, 8, glass=SS.GLASS_TORUS)
    assert tally["fallbacks"] > 0 and not tally["tainted"].any()
    flat, _ = _compose(osc, None, uv, W, H, SPP, 8, glass=SS.GLASS_TORUS)
    assert not np.array_equal(_bits(good[0]), _bits(flat[0]))
    for error in ("no_fallback", "no_normalise", "swap_b", "emissive_on_ns", "origin_on_ns"):
        n = n9
        if error == "emissive_on_ns":                                            # the emitter needs normals of its own to tell the two tests apart
            n = n9.copy()
            lamp = osc.triangles()[1] == 0
            n[lamp] = (n9[lamp] + np.array([1.5, 0, 0], F32)).astype(F32)
            good_e, _ = _compose(osc, n, uv, W, H, SPP, 8, glass=SS.GLASS_TORUS)
        ref = good_e if error == "emissive_on_ns" else good
        kw = {}
        if error == "origin_on_ns":              # at -EPS 1e-4 the offset's direction moves no accumulator of this frame (the diffuse
            kw = dict(eps=0.02)                  # walls forget where a ray came from): the scene is rendered with a wider offset
            ref, tally = _compose(osc, n, uv, W, H, SPP, 8, glass=SS.GLASS_TORUS, **kw)
            assert not tally["tainted"].any()
        bad, _ = _compose(osc, n, uv, W, H, SPP, 8, glass=SS.GLASS_TORUS, errors={error: True}, **kw)
        assert not (np.array_equal(_bits(bad[0]), _bits(ref[0])) and np.array_equal(bad[2], ref[2])), error
