"""Dielectric materials on the host (pt_hip.h: pt_dielectric; no GPU): exact and analytic properties of the restated shading step
(tests/glass_restatement.py), the composition with an empty list against environment_composition, the interface on host-only scenes
with every refusal, pt_render's -GLASS parser, and the setters in a stand-alone program under AddressSanitizer + UBSan.

THE TOLERANCE of the direction tests, TOL(eta) = (16 + 8 eta^2) u with u = 2^-24, the unit roundoff of a float.  The tangential part of
r = d eta + n (eta ci - ct) takes three roundings per component (the product d eta, the product n k, the sum), each at most u times a
magnitude of at most eta + |k| <= 2 max(1, eta): 6 max(1, eta) u.  An error of k itself lies along n and moves only |r|: k = eta ci - ct
carries the error of ct, and ct dct = ds2 / 2 where s2 = (eta eta)(1 - ci ci) takes four roundings, the one of ci ci (absolute u)
multiplied by eta^2, so |r| is off by at most (2 + 2 eta^2) u and the normalisation adds three roundings more.  The inputs are
float roundings of unit vectors (|d| - 1, |N| - 1 <= 2 u each), which the step treats as unit: 4 u (1 + eta^2) more.  Summed and rounded up."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import glass_restatement as G

pt = importlib.import_module("path-tracing_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U = 2.0 ** -24
PT_ERR_INVALID_ARGUMENT = 1
IORS = [0.125, 0.5, 0.75, 1.0, 1.33, 1.5, 2.4, 8.0]


def _tol(eta):
    return (16.0 + 8.0 * np.asarray(eta, np.float64) ** 2) * U


def _ulps(a, b):
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.spacing(np.abs(np.asarray(b, F32)).astype(F32)).astype(np.float64)


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def _grid(n=2000, seed=0):
    """Unit normals and directions: random pairs, and for every normal directions at angles from grazing to normal incidence, both sides."""
    rng = np.random.default_rng(seed)
    N = _unit(rng.normal(size=(n, 3)))
    d = _unit(rng.normal(size=(n, 3)))
    Na, da = [N, N[:200], N[:200]], [d, N[:200], -N[:200]]            # random; exactly along and against the normal (ci rounds to >= 1)
    t = _unit(np.cross(N[:200].astype(np.float64), rng.normal(size=(200, 3))))
    for ang in (0.0, 1e-7, 1e-4, 0.01, 0.3, 0.7, 1.2, 1.5, 1.5707, np.pi / 2):
        for side in (1.0, -1.0):
            Na.append(N[:200])
            da.append(_unit(side * np.cos(ang) * N[:200].astype(np.float64) + np.sin(ang) * t.astype(np.float64)))
    Na.append(np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], F32)); da.append(np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], F32))   # ci == 0 exactly
    return np.concatenate(Na).astype(F32), np.concatenate(da).astype(F32)


def test_normal_incidence_grazing_incidence_and_total_internal_reflection():
    for ior in (1.5, 1.33):
        want = ((ior - 1.0) / (ior + 1.0)) ** 2
        for eta in (F32(ior), G.inv_ior([ior])[0]):                    # leaving and entering: the same reflectance
            F = G.fresnel([1.0], [eta])[0][0]
            assert _ulps(F, want) <= 4, (ior, eta, F, want)
    for ior in IORS:
        for eta in (F32(ior), G.inv_ior([ior])[0]):
            assert G.fresnel([0.0], [eta])[0][0] == F32(1.0)           # ci = 0: exactly 1, in both directions
    for ior in (1.33, 1.5, 2.4, 8.0):                                  # leaving the denser medium: beyond the critical angle F is 1
        crit = np.arcsin(1.0 / ior)
        ang = np.linspace(crit + 1e-3, np.pi / 2, 500)
        F, ct, total = G.fresnel(np.cos(ang).astype(F32), np.full(500, ior, F32))
        assert total.all() and (F == F32(1.0)).all() and not ct.any()


def test_the_reflectance_lies_in_0_1_and_nothing_is_nan():
    N, d = _grid()
    for ior in IORS:
        n, ci, eta = G.incidence(N, d, np.full(len(N), ior, F32))
        assert (ci >= 0).all() and (ci <= 1).all()
        F, ct, total = G.fresnel(ci, eta)
        assert np.isfinite(F).all() and (F >= 0).all() and (F <= 1).all(), ior
        for w3 in (0, 0xFFFFFFFF, 0x80000000):                          # the ray reflected where it can be, transmitted where it can be
            o, dn, col = G.step(N, np.zeros_like(N), d, np.ones(len(N), F32), np.ones_like(N), np.full(len(N), w3, np.uint32),
                                np.full(len(N), ior, F32), np.full_like(N, 0.5), 1e-4)
            assert np.isfinite(o).all() and np.isfinite(dn).all() and np.isfinite(col).all(), (ior, w3)
            assert np.abs(np.linalg.norm(dn.astype(np.float64), axis=1) - 1.0).max() <= 4 * U


def test_snells_law_and_the_law_of_reflection():
    N, d = _grid(seed=1)
    N64, d64 = N.astype(np.float64), d.astype(np.float64)
    for ior in IORS:
        r, n, reflected, F = G.scatter(N, d, np.full(len(N), ior, F32), np.full(len(N), 0xFFFFFFFF, np.uint32))      # u = 1 - 2^-24: transmitted unless F == 1
        _, ci, eta = G.incidence(N, d, np.full(len(N), ior, F32))
        assert (reflected == (F == 1)).all()
        out = G.normalize(r).astype(np.float64)
        n64 = n.astype(np.float64)
        sin_i = np.linalg.norm(np.cross(d64, n64), axis=1)
        sin_o = np.linalg.norm(np.cross(out, n64), axis=1)
        tr = ~reflected
        assert tr.any() or ior > 1
        assert (np.abs(sin_o[tr] - eta[tr].astype(np.float64) * sin_i[tr]) <= _tol(eta[tr])).all(), ior
        assert (np.einsum("ij,ij->i", out[tr], n64[tr]) <= 0).all()     # through the surface
        r2, n2, refl2, _ = G.scatter(N, d, np.full(len(N), ior, F32), np.zeros(len(N), np.uint32))                   # u = 2^-24: reflected unless F < 2^-24
        o2 = G.normalize(r2).astype(np.float64)[refl2]
        mirror = d64[refl2] - 2.0 * np.einsum("ij,ij->i", d64[refl2], N64[refl2])[:, None] * N64[refl2]
        assert np.abs(o2 - mirror).max() <= _tol(1.0)


def test_a_slab_with_parallel_faces_returns_the_direction():
    N, d = _grid(seed=2)
    for ior in IORS:
        iors = np.full(len(N), ior, F32)
        w = np.full(len(N), 0xFFFFFFFF, np.uint32)
        r1, _, refl1, _ = G.scatter(N, d, iors, w)
        d1 = G.normalize(r1)
        r2, _, refl2, _ = G.scatter(-N, d1, iors, w)                    # the far face's outward normal is -N: now the ray leaves
        ci = np.abs(np.einsum("ij,ij->i", N.astype(np.float64), d.astype(np.float64)))
        ok = ~refl1 & ~refl2 & (ci >= 0.01)
        assert ok.sum() > len(N) // 4
        # Each face moves the tangential part by at most TOL of its eta, the first face's error scaled by the second's eta; the
        # normal part of the unit direction that leaves is sqrt(1 - |tangential|^2), whose slope is tan(angle) <= 1 / ci -- the
        # angle at which the ray leaves is the one it came in at -- so a grazing ray amplifies the error by 1 / ci.
        eta = np.maximum(ior, 1.0 / ior)
        err = np.abs(G.normalize(r2)[ok].astype(np.float64) - d[ok].astype(np.float64)).max(axis=1)
        assert (err <= 2 * _tol(eta) * eta / ci[ok]).all(), ior


def test_index_1_changes_nothing():
    N, d = _grid(seed=3)
    one = np.ones(len(N), F32)
    n, ci, eta = G.incidence(N, d, one)
    F, _, total = G.fresnel(ci, eta)
    r, _, reflected, _ = G.scatter(N, d, one, np.full(len(N), 0xFFFFFFFF, np.uint32))
    tr = ~total
    # rs = (ci - ct) / (ci + ct) with ct = sqrt(1 - (1 - ci ci)): ct equals ci to the four roundings of its argument, relative
    # 2 u / ci^2 at worst, so F = 0.5 (rs^2 + rp^2) stays below (2 u / ci^2)^2 -- below a few ulps of the smallest F that counts, 2^-24
    assert (F[tr] <= np.maximum((2 * U / ci[tr].astype(np.float64) ** 2) ** 2, 4 * U * U)).all()
    assert (~reflected[tr]).all()
    # The direction is d + n (ci - ct): what ct misses of ci, u / ci (the argument 1 - (1 - ci ci) is off by 2 u absolutely, the root
    # halves and divides by ct), lies along n and turns the ray by at most that: a few units in the last place of a unit vector's
    # components from ci = 0.5 up, TOL(1) / ci down to grazing incidence.
    err = np.abs(G.normalize(r)[tr].astype(np.float64) - d[tr].astype(np.float64)).max(axis=1)
    assert (err <= _tol(1.0) / ci[tr]).all()
    assert (err[ci[tr] >= 0.5] <= 8 * U).all()
    head_on = ci == 1
    assert (F[head_on] == 0).all() and (_ulps(G.normalize(r)[head_on], d[head_on])[np.abs(d[head_on]) > 0.1] <= 4).all()


def test_the_composition_with_an_empty_list_is_environment_compositions(oracle_scene):
    import environment_composition as EC
    import glass_composition as GC
    env = np.random.default_rng(0).uniform(0.1, 2.0, (8, 8, 3)).astype(F32)
    px = np.array([(x, y) for y in range(0, 12, 3) for x in range(0, 16, 3)])
    want = EC.compose(oracle_scene, env, 16, 12, px, 3, 4)
    for glass in (None, {}):
        got = GC.compose(oracle_scene, glass, env, 16, 12, px, 3, 4)
        assert all(np.array_equal(a.view(np.uint32) if a.dtype == F32 else a, b.view(np.uint32) if b.dtype == F32 else b) for a, b in zip(got, want))
    lit = GC.compose(oracle_scene, {4: (1.5, (1, 1, 1)), 1: (1.5, (1, 1, 1))}, env, 16, 12, px, 3, 4)
    assert not np.array_equal(lit[0], want[0])


def _entries(s):
    return [(e.material, e.ior, tuple(e.tint)) for e in s.dielectrics()]


def test_the_interface_on_a_host_only_scene(models_dir):
    s = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    assert s.dielectrics() == []
    first = [pt.dielectric(4, 1.5, (0.9, 1.0, 0.9)), pt.dielectric(2, 0.5, (0.0, 0.0, 0.0))]
    s.set_dielectrics(first)
    kept = [(4, 1.5, (F32(0.9), 1.0, F32(0.9))), (2, 0.5, (0.0, 0.0, 0.0))]
    assert _entries(s) == kept
    nan, inf = float("nan"), float("inf")
    refused = [[pt.dielectric(5, 1.5)], [pt.dielectric(-1, 1.5)], [pt.dielectric(3, 1.5), pt.dielectric(3, 1.3)],          # outside the scene, twice
               [pt.dielectric(3, 0.12)], [pt.dielectric(3, 8.5)], [pt.dielectric(3, nan)], [pt.dielectric(3, inf)], [pt.dielectric(3, -1.5)],
               [pt.dielectric(3, 1.5, (1, -0.1, 1))], [pt.dielectric(3, 1.5, (1, 1, 1.1))], [pt.dielectric(3, 1.5, (nan, 1, 1))], [pt.dielectric(3, 1.5, (1, inf, 1))],
               [pt.dielectric(1, 1.5), pt.dielectric(0, 1.5)]]                                                              # material 0 emits
    for bad in refused:
        with pytest.raises(pt.PtError) as e:
            s.set_dielectrics(bad)
        assert e.value.status == PT_ERR_INVALID_ARGUMENT and _entries(s) == kept, bad
    L = s._L
    arr = (pt.Dielectric * 2)(*first)
    assert L.pt_scene_set_dielectrics(s._h, arr, -1) == PT_ERR_INVALID_ARGUMENT and L.pt_scene_set_dielectrics(s._h, None, 2) == PT_ERR_INVALID_ARGUMENT
    assert L.pt_scene_set_dielectrics(None, arr, 2) == PT_ERR_INVALID_ARGUMENT and _entries(s) == kept
    s.set_dielectrics([pt.dielectric(1, 0.125, (0, 1, 0)), pt.dielectric(2, 8.0), pt.dielectric(3, 1.0)])                   # the limits are allowed
    assert [e[:2] for e in _entries(s)] == [(1, 0.125), (2, 8.0), (3, 1.0)]
    clone = s.clone_to_device(-1)                                       # a clone inherits; clearing it leaves the original alone
    assert _entries(clone) == _entries(s)
    clone.set_dielectrics(None)
    assert clone.dielectrics() == [] and len(s.dielectrics()) == 3
    s.set_dielectrics([])
    assert s.dielectrics() == []
    clone.close()
    s.close()


def test_pt_render_refuses_a_bad_glass_flag(tmp_path, models_dir):
    exe = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
    model = ["-MODEL_PATH", models_dir, "-MODEL_NAME", "Tor.obj"]
    cases = [("4", "-GLASS takes"), ("4:", "-GLASS takes"), ("x:1.5", "-GLASS takes"), ("4:1.5:1:1", "-GLASS takes"), ("4:1.5:1:1:1:1", "-GLASS takes"),
             ("4:1.5,", "-GLASS takes"), ("4:glass", "-GLASS takes"), ("4.5:1.5", "-GLASS takes"), ("-1:1.5", "-GLASS takes"),
             ("4:0.1", "ior must lie"), ("4:9", "ior must lie"), ("4:nan", "-GLASS takes"), ("4:1.5:1:2:1", "tint component"), ("4:1.5:-0.5:1:1", "tint component"),
             ("5:1.5", "outside the scene"), ("4:1.5,4:1.3", "listed twice"), ("0:1.5", "emissive")]
    for text, message in cases:
        run = subprocess.run([exe] + model + ["-GLASS", text], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
        assert run.returncode == 2 and message in run.stderr + run.stdout, (text, run.returncode, run.stderr)


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"), reason="g++ or the HIP headers are not available")
def test_the_setters_are_clean_under_asan_and_ubsan(tmp_path):
    """pt_glass_capi.cpp alone with a stand-alone main, on host-only handles: every refusal, a refused call leaving the list as it was,
    the frame's setters, clear and get.  Host code only, run as a program of its own."""
    exe = str(tmp_path / "glass_san")
    csrc = os.path.join(ROOT, "path-tracing_amd", "csrc")
    build = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                            os.path.join(ROOT, "tests", "native", "glass_sanitizer_main.cpp"), os.path.join(csrc, "pt_glass_capi.cpp"), "-o", exe,
                            "-L/opt/rocm/lib", "-lamdhip64", "-ldl", "-lpthread", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")      # (the HIP runtime's own start-up allocations are not ours to judge)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    assert "glass host ok" in run.stdout
