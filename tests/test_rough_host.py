"""Rough specular reflection on the host (pt_hip.h: rough specular): pt.rough_step against tests/rough_restatement.py bit for bit on
random and axis-aligned normals (n.z = +-1 and -0.0 among them), at grazing and back-side incidence, at both bounds of alpha and with
the words 0 and 2^32 - 1; the step's exact properties; the sampled distribution of the microfacet normal against a quadrature of the
distribution of visible normals by a chi-square test, which three planted errors fail; the loader's Pr, -ROUGH's parser and every
refusal; the host code under ASan + UBSan as a program of its own; and the composition: every frame the GPU tests render is composed
here first and marks no pixel tainted, and a frame of the room tells each of four single errors from the stated step."""
import importlib
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import rough_composition as RC
import rough_restatement as RR
import rough_scenes as RS
import smooth_scenes as SS
import texture_scenes as S

pt = importlib.import_module("path-tracing_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _unit(v):
    v = np.asarray(v, np.float64)
    return RR.G.normalize((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32))


def _cases():
    """normals, directions, alpha, w1, w2: random ones, then every special normal against every special incidence, alpha and word."""
    rng = np.random.default_rng(7)
    k = 4000
    n = _unit(rng.normal(size=(k, 3)))
    d = _unit(rng.normal(size=(k, 3)))                                           # both sides of n: front and back incidence
    alpha = np.exp(rng.uniform(np.log(2.0 ** -10), 0.0, k)).astype(F32)
    w1, w2 = rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32), rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
    special_n = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [1, 0, -0.0], [0, 1, -0.0], [0.6, 0.8, 0.0],
                          [-0.0, -0.0, 1], [0.28, -0.96, -0.0]], F32)
    words = np.array([0, 2 ** 32 - 1, 1 << 9, 0x80000000, 0x12345678], np.uint32)
    ns, ds, als, a1, a2 = [], [], [], [], []
    for sn in special_n:
        t = np.cross(sn, [0.3, -0.5, 0.8])
        t = t / np.linalg.norm(t)
        for cosine in (1.0, 0.5, 1e-3, 1e-7, 0.0, -1e-7, -0.5, -1.0):            # head-on ... grazing ... from behind
            dd = -cosine * sn.astype(np.float64) + math.sqrt(max(0.0, 1 - cosine * cosine)) * t
            for al in (2.0 ** -10, 0.05, 0.3, 1.0):
                for x in words:
                    for y in words[:3]:
                        ns.append(sn); ds.append(dd); als.append(al); a1.append(x); a2.append(y)
    return (np.vstack([n, np.array(ns, F32)]), np.vstack([d, _unit(np.array(ds))]), np.concatenate([alpha, np.array(als, F32)]),
            np.concatenate([w1, np.array(a1, np.uint32)]), np.concatenate([w2, np.array(a2, np.uint32)]))


def test_rough_step_equals_the_restatement_bit_for_bit_and_has_its_exact_properties():
    n, d, alpha, w1, w2 = _cases()
    l, g1, h = pt.rough_step(n, d, alpha, w1, w2, want_microfacet=True)
    wl, wg, wh = RR.step(n, d, alpha, w1, w2)
    assert np.array_equal(_bits(l), _bits(wl)) and np.array_equal(_bits(g1), _bits(wg)) and np.array_equal(_bits(h), _bits(wh))
    assert np.isfinite(l).all() and np.isfinite(g1).all() and np.isfinite(h).all()
    assert (g1 >= 0).all() and (g1 <= 1).all()
    # unit length to the last bits of normalize3: the sum of squares, its root, the reciprocal and the product each round once (half an
    # ulp of 2^-24 relative each, the sum's error halved by the root): under 4 x 2^-24 in all
    assert np.abs(np.linalg.norm(l.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22
    turned = np.where((RR.dot(n, d) > 0)[:, None], -n, n).astype(F32)
    nl = RR.dot(turned, l)
    assert np.array_equal(g1 == 0, ~(nl > 0))                                    # G1 == 0 exactly where n . l <= 0
    assert (g1 == 0).any() and (g1 == 1).any() and ((g1 > 0) & (g1 < 1)).any()
    assert (h[:, 2] >= 0).all()
    with pytest.raises(pt.PtError):
        pt.rough_step(n[:1], d[:1], 2.0 ** -11, w1[:1], w2[:1])
    with pytest.raises(pt.PtError):
        pt.rough_step(n[:1], d[:1], np.nan, w1[:1], w2[:1])


# ---- the sampled distribution --------------------------------------------------------------------------------------------------------
GRID, DRAWS, P_VALUE, SUB = 16, 1 << 20, 1e-6, 128


def _chi2_isf(p, dof):
    """x with P(chi-square_dof > x) = p: the regularised upper incomplete gamma function Q(dof / 2, x / 2) (Lentz's continued fraction,
    valid for x > dof + 1, which every p below 1/2 gives) solved for x by bisection."""
    a = dof / 2.0

    def q(x):
        x = x / 2.0
        tiny = 1e-300
        b = x + 1.0 - a
        c, dd = 1.0 / tiny, 1.0 / b
        hh = dd
        for i in range(1, 10000):
            an = -i * (i - a)
            b += 2.0
            dd = an * dd + b
            dd = tiny if abs(dd) < tiny else dd
            c = b + an / c
            c = tiny if abs(c) < tiny else c
            dd = 1.0 / dd
            delta = dd * c
            hh *= delta
            if abs(delta - 1.0) < 1e-15:
                break
        return math.exp(-x + a * math.log(x) - math.lgamma(a)) * hh

    lo, hi = dof + 2.0, dof + 2.0
    while q(hi) > p:
        hi *= 1.5
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if q(mid) > p else (lo, mid)
    return hi


def _expected(theta, alpha):
    """The probability of every cell of the GRID x GRID grid over the projected hemisphere (h.x, h.y in [-1, 1]) under the density of
    visible normals  D(h) G1(v) max(0, v . h) / (n . v)  per solid angle, n = z, v = (-sin theta, 0, cos theta): midpoint rule on SUB x SUB
    points per cell in double precision (d omega = dx dy / h.z)."""
    m = GRID * SUB
    edges = np.arange(m + 1) * (2.0 / m) - 1.0
    x = 0.5 * (edges[1:] + edges[:-1])
    X, Y = np.meshgrid(x, x, indexing="ij")
    Z = np.sqrt(np.maximum(1.0 - (X * X + Y * Y), 0.0))
    # 1 / h.z, which grows without bound at the rim, is integrated exactly along x: the integral of dx / sqrt(rho^2 - x^2) is asin(x / rho)
    rho = np.sqrt(1.0 - x * x)
    weight = np.diff(np.arcsin(np.clip(edges[:, None] / rho[None, :], -1.0, 1.0)), axis=0) * (2.0 / m)
    a2 = alpha * alpha
    D = a2 / (math.pi * ((a2 - 1.0) * Z * Z + 1.0) ** 2)
    vx, vz = -math.sin(theta), math.cos(theta)
    g1v = 2.0 * vz / (vz + math.sqrt(a2 + (1.0 - a2) * vz * vz))
    dens = D * g1v * np.maximum(0.0, vx * X + vz * Z) / vz * weight
    return dens.reshape(GRID, SUB, GRID, SUB).sum(axis=(1, 3))


def _chi_square(h, expected):
    """(statistic, bound at P_VALUE) of the draws' microfacet normals h against the cells' probabilities.  Cells that expect fewer than
    10 draws are pooled into one (the chi-square approximation wants expected counts of several draws per cell); the quadrature is
    normalised to 1, its total having been checked."""
    ix = np.clip(((h[:, 0].astype(np.float64) + 1.0) * (GRID / 2)).astype(np.int64), 0, GRID - 1)
    iy = np.clip(((h[:, 1].astype(np.float64) + 1.0) * (GRID / 2)).astype(np.int64), 0, GRID - 1)
    seen = np.bincount(ix * GRID + iy, minlength=GRID * GRID).astype(np.float64)
    want = (expected / expected.sum()).ravel() * len(h)
    small = want < 10.0
    seen = np.append(seen[~small], seen[small].sum())
    want = np.append(want[~small], want[small].sum())
    if want[-1] == 0:
        assert seen[-1] == 0
        seen, want = seen[:-1], want[:-1]
    stat = float((((seen - want) ** 2) / want).sum())
    return stat, _chi2_isf(P_VALUE, len(want) - 1), len(want)


def _draws(theta, alpha, seed, step):
    rng = np.random.default_rng(seed)
    w1 = rng.integers(0, 2 ** 32, DRAWS, dtype=np.uint64).astype(np.uint32)
    w2 = rng.integers(0, 2 ** 32, DRAWS, dtype=np.uint64).astype(np.uint32)
    n = np.tile(np.array([0, 0, 1], F32), (DRAWS, 1))
    d = np.tile(np.array([math.sin(theta), 0.0, -math.cos(theta)], F32), (DRAWS, 1))
    return step(n, d, F32(alpha), w1, w2)


def test_the_chi_square_bound_is_the_distributions():
    for dof, want in ((1, 23.92813), (50, 112.60809), (255, 377.07812)):          # (the distribution's quantiles at p = 10^-6)
        assert abs(_chi2_isf(1e-6, dof) - want) < 1e-6 * want, (dof, _chi2_isf(1e-6, dof))


@pytest.mark.parametrize("alpha", [0.05, 0.3, 1.0])
@pytest.mark.parametrize("degrees", [0.0, 60.0, 85.0])
def test_the_sampled_microfacet_normals_follow_the_distribution_of_visible_normals(degrees, alpha):
    theta = math.radians(degrees)
    expected = _expected(theta, alpha)
    assert abs(expected.sum() - 1.0) < 1e-4, expected.sum()                      # the density integrates to 1: the quadrature is sound
    h = _draws(theta, alpha, 1000 + int(degrees) + int(alpha * 100), lambda *a: pt.rough_step(*a, want_microfacet=True))[2]
    stat, bound, cells = _chi_square(h, expected)
    print(f"theta {degrees} alpha {alpha}: chi-square {stat:.1f} on {cells} cells, bound {bound:.1f}, quadrature total {expected.sum():.6f}")
    assert stat < bound, (stat, bound, cells)


@pytest.mark.parametrize("error", ["alpha_squared", "no_warp", "no_unstretch"])
def test_each_planted_error_fails_the_chi_square_test(error):
    theta, alpha = math.radians(60.0), 0.3
    expected = _expected(theta, alpha)
    good = _draws(theta, alpha, 5, RR.step)[2]
    stat, bound, _ = _chi_square(good, expected)
    assert stat < bound, (stat, bound)                                           # the restatement itself passes
    bad = _draws(theta, alpha, 5, lambda *a: RR.step(*a, **{error: True}))[2]
    stat, bound, _ = _chi_square(bad, expected)
    assert stat > bound, (error, stat, bound)


# ---- the loader, the setters, the parser ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("rough")) + "/"
    return d, RS.room(d)


def test_the_loader_records_pr_and_applies_nothing(room_dir, models_dir):
    d, _ = room_dir
    sc = pt.Scene.load_obj(d, "rough_room.obj", device=-1)
    assert np.array_equal(sc.mtl_roughness(), np.array(RS.ROOM_PR, F32)) and sc.roughness() == []
    tor = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    assert np.array_equal(tor.mtl_roughness(), np.full(5, -1, F32))
    tri, tri_mat = sc.triangles()
    made = pt.Scene.create(tri, tri_mat, sc.materials(), device=-1)
    assert np.array_equal(made.mtl_roughness(), np.full(6, -1, F32))
    open(d + "odd.mtl", "w").write("newmtl a\nKd 1 1 1\nPr x\nnewmtl b\nPr nan\nKd 1 1 1\nnewmtl c\nKd 0.5 0.5 0.5\nPr -3\n")
    open(d + "odd.obj", "w").write("mtllib odd.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nusemtl 0\nf 1 2 3\n")
    odd = pt.Scene.load_obj(d, "odd.obj", device=-1)
    assert np.array_equal(odd.mtl_roughness(), np.array([-1, -1, -3], F32)) and np.array_equal(odd.materials()[2, 0:3], [0.5, 0.5, 0.5])


def _entries(sc):
    return [(e.material, e.alpha) for e in sc.roughness()]


def test_every_refusal_changes_nothing_and_both_orders_with_the_dielectrics(room_dir):
    d, _ = room_dir
    sc = pt.Scene.load_obj(d, "rough_room.obj", device=-1)
    sc.set_roughness([pt.rough(2, 0.25), pt.rough(5, 2.0 ** -10), pt.rough(3, 1.0)])
    kept = [(2, 0.25), (5, 2.0 ** -10), (3, 1.0)]
    assert _entries(sc) == kept
    for bad in ([pt.rough(6, 0.3)], [pt.rough(-1, 0.3)], [pt.rough(2, 0.3), pt.rough(2, 0.4)], [pt.rough(2, np.nan)], [pt.rough(2, np.inf)],
                [pt.rough(2, 2.0 ** -11)], [pt.rough(2, 1.0000001)], [pt.rough(2, 0.0)], [pt.rough(2, -0.3)],
                [pt.rough(1, 0.3)], [pt.rough(4, 0.3)], [pt.rough(0, 0.3)]):      # Ns == 0 (twice), emissive
        with pytest.raises(pt.PtError) as e:
            sc.set_roughness(bad)
        assert e.value.status == 1 and _entries(sc) == kept, bad
    with pytest.raises(pt.PtError):                                              # the dielectric setter refuses a rough material ...
        sc.set_dielectrics([pt.dielectric(5, 1.5)])
    assert sc.dielectrics() == [] and _entries(sc) == kept
    sc.set_roughness(None)
    assert sc.roughness() == []
    sc.set_dielectrics([pt.dielectric(5, 1.5)])
    with pytest.raises(pt.PtError):                                              # ... and the roughness setter a dielectric
        sc.set_roughness([pt.rough(5, 0.3)])
    assert sc.roughness() == [] and len(sc.dielectrics()) == 1
    sc.set_roughness([pt.rough(2, 0.3)])
    sc.set_roughness([])
    assert sc.roughness() == []
    no_ks = pt.Scene.create(sc.triangles()[0], sc.triangles()[1], np.array([[1, 1, 1, 0, 0, 0, 0, 0, 0, 500]] * 6, F32), device=-1)
    with pytest.raises(pt.PtError):                                              # Ks == 0
        no_ks.set_roughness([pt.rough(2, 0.3)])
    L = pt.lib()
    assert L.pt_scene_set_roughness(None, None, 0) == 1 and L.pt_frame_set_roughness(None, None, 0) == 1
    assert L.pt_scene_get_roughness(None, None, None) == 1 and L.pt_scene_get_mtl_roughness(None, None) == 1
    assert L.pt_rough_step(1, None, None, None, None, None, None, None, None) == 1 and L.pt_abi_version() == 5


@pytest.mark.parametrize("flags", [["-ROUGH", "4"], ["-ROUGH", "4:"], ["-ROUGH", ":0.3"], ["-ROUGH", "4:0.3:1"], ["-ROUGH", "x:0.3"], ["-ROUGH", "4:x"],
                                   ["-ROUGH", "-4:0.3"], ["-ROUGH", "4.5:0.3"], ["-ROUGH", "4:0.3,"], ["-ROUGH", "4:0"], ["-ROUGH", "4:1.5"],
                                   ["-ROUGH", "4:nan"], ["-ROUGH", "MTL"], ["-ROUGH", "9:0.3"], ["-ROUGH", "0:0.3"], ["-ROUGH", "4:0.3,4:0.2"],
                                   ["-ROUGH", "4:0.3", "-GLASS", "4:1.5"]])
def test_the_parser_ends_with_status_2(flags, models_dir):
    assert os.path.exists(EXE), "pt_render is not built: the build is broken, the parser is not checked"   # (refused before any HIP call)
    r = subprocess.run([EXE, "--W", "8", "--H", "8", "-RPP", "1", "-MODEL_PATH", models_dir, "-QUIET", "1"] + flags, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stderr)


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"), reason="g++ or the HIP headers are not available")
def test_the_host_code_is_clean_under_asan_and_ubsan(room_dir):
    """pt_rough_capi.cpp, pt_glass_capi.cpp and pt_scene.cpp with a stand-alone main, on host-only handles.  Host code only."""
    d, _ = room_dir
    exe = d + "rough_san"
    csrc = os.path.join(ROOT, "path-tracing_amd", "csrc")
    build = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                            os.path.join(ROOT, "tests", "native", "rough_sanitizer_main.cpp"), os.path.join(csrc, "pt_rough_capi.cpp"),
                            os.path.join(csrc, "pt_glass_capi.cpp"), os.path.join(csrc, "pt_scene.cpp"), "-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-ldl",
                            "-lpthread", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")      # (the HIP runtime's own start-up allocations are not ours to judge)
    run = subprocess.run([exe, d], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    assert "rough host ok" in run.stdout


# ---- the composition -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tor(models_dir):
    osc, uv = S.tor(models_dir)
    return osc, uv, SS.tor_normals(osc)


def _compose(osc, rough, n9, uv, w, h, spp, mrr, **kw):
    kw.pop("stats", None)
    if not kw.pop("smooth", False):
        n9 = None
    tally = {}
    out = RC.compose(osc, rough, n9, kw.pop("textures", None), uv, kw.pop("glass", None), kw.pop("env", None), w, h, kw.pop("px", S.all_pixels(w, h)), spp, mrr,
                     stats=tally, **kw)
    return out, tally


@pytest.mark.parametrize("name", list(RS.TOR_FRAMES))
def test_every_tor_frame_of_the_gpu_test_composes_without_a_tainted_pixel(tor, name):
    osc, uv, n9 = tor
    (w, h), spp, mrr, kw = RS.TOR_FRAMES[name]
    kw = dict(kw)
    _, tally = _compose(osc, kw.pop("rough"), n9, uv, w, h, spp, mrr, **kw)
    assert tally["tainted"].sum() == 0 and tally["rough_steps"] > 0
    if name == "smooth_normals":
        assert tally["fallbacks"] > 0 and tally["smooth_steps"] > 0


@pytest.mark.parametrize("view", RS.VIEWS)
def test_every_view_composes_without_a_tainted_pixel(tor, view):
    osc, uv, n9 = tor
    _, tally = _compose(osc, RS.ROUGH_ALL, n9, uv, 40, 28, 4, 4, **S.set_view(pt, None, view, 40, 28))
    assert tally["tainted"].sum() == 0 and tally["rough_steps"] > 0


def test_the_room_composes_without_a_tainted_pixel_and_tells_each_single_error_from_the_stated_step(room_dir):
    _, osc = room_dir
    (W, H), SPP, MRR = RS.ROOM_FRAME
    good, tally = _compose(osc, RS.ROOM_ROUGH, None, None, W, H, SPP, MRR)
    assert tally["tainted"].sum() == 0 and tally["rough_steps"] > W * H and tally["rough_zero"] > 0
    mtl, tally = _compose(osc, RS.ROOM_MTL_LIST, None, None, W, H, SPP, MRR)     # the list -ROUGH mtl makes (tests/test_gpu_rough_cli.py)
    assert tally["tainted"].sum() == 0 and tally["rough_steps"] > W * H
    for error in ("w23", "drop_g1", "origin_on_h", "mirror"):
        ref, kw = good, {}
        if error == "origin_on_h":               # at the default eps of 1e-4 the offset's direction moves a hit point by less than the
            kw = dict(eps=0.05)                  # accumulators can see (throughputs depend on directions only): a wider offset shows it
            ref, tally = _compose(osc, RS.ROOM_ROUGH, None, None, W, H, SPP, MRR, **kw)
            assert tally["tainted"].sum() == 0
        bad, _ = _compose(osc, RS.ROOM_ROUGH, None, None, W, H, SPP, MRR, errors={error: True}, **kw)
        assert not (np.array_equal(_bits(bad[0]), _bits(ref[0])) and np.array_equal(_bits(bad[1]), _bits(ref[1])) and np.array_equal(bad[2], ref[2])), error
