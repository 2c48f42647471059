"""CPU checks of the thin lens (pt_hip.h: pt_lens): the host composition against the oracle, the handle's lens and its checks,
clones, the culling envelope a lens implies, pt_render's lens flags, and the compiler's report on the lens kernels."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import view_composition as V

pt = importlib.import_module("path-tracing_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_RENDER = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
KU = 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _all_pixels(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs.ravel(), ys.ravel()], 1)


def _same(a, b):
    return all(np.array_equal(_bits(x) if x.dtype == np.float32 else x, _bits(y) if y.dtype == np.float32 else y) for x, y in zip(a, b))


# ---- 1. the composition is the oracle's frame for the reference camera -----------------------------------------------------
@pytest.mark.parametrize("mrr", [1, 3, 8])
@pytest.mark.parametrize("err", [-1.0, 0.02])
def test_composition_of_the_reference_view_is_the_oracle_frame(oracle_scene, mrr, err):
    W, H, spp = 24, 16, 20   # (passes > 10: the adaptive skip has something to do at -ERR 0.02)
    want = O.render(oracle_scene, W, H, spp, mrr, error=err, seed=7, rng=O.RNG_COUNTER, trig=O.TRIG_PORTABLE)[:3]
    got = V.compose(oracle_scene, W, H, _all_pixels(W, H), spp, mrr, error=err, seed=7)
    assert want[2].sum() > 0
    assert _same(got, (want[0].reshape(-1, 3), want[1].reshape(-1, 3), want[2]))
    if err > 0:   # the skip really ran: some pixel has fewer samples than passes
        assert (want[2] < spp).any() or mrr == 1


def test_composition_of_the_reference_view_under_a_skybox_is_the_oracle_frame(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_open_scene as MO
    d = str(tmp_path) + "/"
    MO.generate(os.path.join(ROOT, "models"), d, name="Open.obj")
    sc = O.Scene.load(d, "Open.obj")
    sc.set_skybox(d + "sky.bmp")
    W, H, spp = 24, 16, 12
    for mrr in (1, 8):
        want = O.render(sc, W, H, spp, mrr, error=-1.0, seed=42, rng=O.RNG_COUNTER, trig=O.TRIG_PORTABLE)[:3]
        got = V.compose(sc, W, H, _all_pixels(W, H), spp, mrr)
        assert _same(got, (want[0].reshape(-1, 3), want[1].reshape(-1, 3), want[2])), mrr


def test_composition_of_a_pixel_subset_is_the_same_as_of_the_frame(oracle_scene):
    W, H = 40, 30
    cam = pt.look_at((3, 2, -12), (0, 0, 0), fov_y=50.0).as_array()
    full = V.compose(oracle_scene, W, H, _all_pixels(W, H), 6, 8, camera=cam, lens=(0.4, 12.0))
    pick = np.array([7, 100, 555, 1199])
    part = V.compose(oracle_scene, W, H, _all_pixels(W, H)[pick], 6, 8, camera=cam, lens=(0.4, 12.0))
    assert _same(part, (full[0][pick], full[1][pick], full[2][pick]))


def test_the_lens_ray_passes_through_the_focal_point_of_its_pinhole_ray():
    cam = pt.look_at((6, 3, -15), (0, 0, 0), fov_y=45.0, aspect=1.5).as_array()
    rng = np.random.default_rng(3)
    words = rng.integers(0, 2 ** 32, size=(500, 4), dtype=np.uint64).astype(np.uint32)
    x, y = rng.integers(0, 300, 500), rng.integers(0, 200, 500)
    focus = 16.0
    o0, d0 = V.primary_rays(x, y, 300, 200, words, cam)
    o1, d1 = V.primary_rays(x, y, 300, 200, words, cam, (0.5, focus))
    f = V.lens_axes(cam)[2].astype(np.float64)
    p0 = o0 + d0 * (focus / (d0.astype(np.float64) @ f))[:, None]        # where the pinhole ray meets the focal plane
    p1 = o1 + d1 * ((focus - (o1 - cam[0]).astype(np.float64) @ f) / (d1.astype(np.float64) @ f))[:, None]
    assert np.abs(p0 - p1).max() < 1e-4 * focus
    assert np.abs((o1 - cam[0]).astype(np.float64) @ f).max() < 1e-6        # the lens lies in the right-up plane
    r = np.linalg.norm(o1 - cam[0], axis=1)
    assert r.max() <= 0.5 * (1 + 1e-6) and r.max() > 0.45


# ---- 2. the handle's lens -------------------------------------------------------------------------------------------------
@pytest.fixture()
def tor(models_dir):
    s = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    yield s
    s.close()


def test_lens_round_trips_and_resets(tor):
    assert tor.lens() is None
    tor.set_lens(0.5, 16.0)
    assert tor.lens() == pt.Lens(0.5, 16.0)
    tor.set_lens(pt.Lens(0.25, 3.0))
    assert tor.lens() == pt.Lens(0.25, 3.0)
    tor.set_lens(0.0, 10.0)          # radius 0: a pinhole
    assert tor.lens() is None
    tor.set_lens(0.3, 5.0)
    tor.set_lens(None)
    assert tor.lens() is None


@pytest.mark.parametrize("bad,status", [
    ((float("nan"), 10.0), "PT_ERR_INVALID_ARGUMENT"),
    ((0.5, float("inf")), "PT_ERR_INVALID_ARGUMENT"),
    ((-0.1, 10.0), "PT_ERR_INVALID_ARGUMENT"),
    ((0.5, 0.0), "PT_ERR_INVALID_ARGUMENT"),
    ((0.5, -3.0), "PT_ERR_INVALID_ARGUMENT"),
    ((4100.0, 20.0), "PT_ERR_UNSUPPORTED"),     # the disc reaches beyond PT_CAMERA_MAX_ORIGIN
])
def test_bad_lenses_are_refused_and_leave_the_handle_alone(tor, bad, status):
    tor.set_lens(0.2, 7.0)
    with pytest.raises(pt.PtError) as e:
        tor.set_lens(*bad)
    assert e.value.status == getattr(pt, status)
    assert tor.lens() == pt.Lens(0.2, 7.0)
    tor.set_lens(None)
    with pytest.raises(pt.PtError):
        tor.set_lens(*bad)
    assert tor.lens() is None


# forward in the plane of right and up but not in their span's null direction: D . f^ can reach 0 in the image
GRAZING = ((0, 0, -20), (1, 0, 0.8), (0, 1, 0), (0, 0, 0.5))


def test_a_camera_whose_view_can_reach_the_lens_plane_is_refused_with_a_lens(tor):
    tor.set_camera(GRAZING)                       # a pinhole camera of this kind is fine
    with pytest.raises(pt.PtError) as e:
        tor.set_lens(0.5, 10.0)
    assert e.value.status == pt.PT_ERR_INVALID_ARGUMENT and tor.lens() is None
    tor.set_camera(None)
    tor.set_lens(0.5, 10.0)
    with pytest.raises(pt.PtError) as e:          # and the camera is checked against the lens the handle has
        tor.set_camera(GRAZING)
    assert e.value.status == pt.PT_ERR_INVALID_ARGUMENT
    assert tor.camera() is None and tor.lens() == pt.Lens(0.5, 10.0)


def test_a_camera_is_checked_against_the_lens_origin_bound(tor):
    tor.set_camera(((0, 0, -4000.0), (1, 0, 0), (0, 1, 0), (0, 0, 1)))
    tor.set_lens(100.0, 10.0)                     # the disc lies in x and y: z stays at 4000
    far_x = ((4000.0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))
    with pytest.raises(pt.PtError) as e:          # this one would put lens origins at |x| = 4100
        tor.set_camera(far_x)
    assert e.value.status == pt.PT_ERR_UNSUPPORTED
    assert tor.camera().as_array()[0, 2] == -4000.0


def test_clones_inherit_the_lens_of_the_handle_they_are_made_from(tor):
    tor.set_lens(0.5, 16.0)
    c1 = tor.clone_to_device(-1)
    assert c1.lens() == pt.Lens(0.5, 16.0) and c1.camera() is None
    c1.set_lens(None)                             # a copy's lens is its own
    assert tor.lens() == pt.Lens(0.5, 16.0) and c1.lens() is None
    tor.set_lens(None)
    c2 = tor.clone_to_device(-1)
    assert c2.lens() is None
    c1.close()
    c2.close()


# ---- 3. the envelope ------------------------------------------------------------------------------------------------------
def _tables(scene, eps=1e-4):
    t = scene.cull_tables(eps)
    lay = scene.cull_layout(eps)
    return [t["cluster_sphere"], t["spheres"], t["bary"], np.array(list(t["constants"].values()), np.float32),
            lay["slot_triangle"], lay["bvh"]]


def _r_org(scene, eps=1e-4):
    """k2 = kU (24 sqrt(3) + 8) r_org (pt_cull_tables.cpp, margins of the barycentric test)."""
    return scene.cull_tables(eps)["constants"]["k2"] / (KU * (24 * np.sqrt(3) + 8))


def _extreme_origins(cam, lens):
    """Lens origins at the rim (w2 = 0xFFFFFFFF: the largest unit_float) in every quadrant of phi and on its boundaries."""
    w3 = np.array([0, 1, 2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, 2 ** 31 - 1, 2 ** 31, 3 * 2 ** 30 - 1, 3 * 2 ** 30, 2 ** 32 - 1] +
                  list(np.linspace(0, 2 ** 32 - 1, 301).astype(np.uint64)), np.uint64).astype(np.uint32)
    words = np.stack([np.full_like(w3, 12345), np.full_like(w3, 54321), np.full_like(w3, 0xFFFFFFFF), w3], 1)
    o, _ = V.primary_rays(np.zeros(len(w3), int), np.zeros(len(w3), int), 64, 64, words, cam, lens)
    return o


@pytest.mark.parametrize("eye,target,radius", [((6, 3, -15), (0, 0, 0), 0.5), ((19.0, -19.0, 5.0), (0, 0, 0), 2.0),
                                               ((0, 0, -200), (3, 1, 0), 30.0), ((100, 50, -20), (0, 0, 0), 7.0)])
def test_the_envelope_covers_extreme_lens_samples(tor, eye, target, radius):
    cam = pt.look_at(eye, target, fov_y=40.0)
    tor.set_camera(cam)
    tor.set_lens(radius, 10.0)
    o = _extreme_origins(cam.as_array(), (radius, 10.0))
    r_max = _r_org(tor) - 1.0
    assert np.abs(o).max() <= r_max, (np.abs(o).max(), r_max)
    assert np.linalg.norm(o - cam.as_array()[0], axis=1).max() > radius * (1 - 1e-6)   # the samples reach the rim


def test_a_small_lens_near_the_reference_eye_shares_the_camera_free_tables(models_dir):
    plain = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    want = _tables(plain)
    for cam, radius in ((None, 0.5), (pt.look_at((5, -7, 12), (0, 1, 3), fov_y=70.0), 0.5)):
        s = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
        if cam is not None:
            s.set_camera(cam)
        s.set_lens(radius, 20.0)
        for a, b in zip(want, _tables(s)):
            assert a.shape == b.shape and a.tobytes() == b.tobytes()
        s.close()
    plain.close()


def test_a_large_lens_widens_the_envelope(tor):
    r_default = _r_org(tor)
    tor.set_lens(30.0, 20.0)          # the reference camera: the disc spans x and y up to 30
    r_wide = _r_org(tor)
    assert r_wide >= 31.0 and r_wide <= 31.0 * (1 + 1e-4), r_wide
    assert r_default < r_wide
    tor.set_lens(None)
    assert _r_org(tor) == pytest.approx(r_default, rel=1e-7)


# ---- 4. pt_render ---------------------------------------------------------------------------------------------------------
def _print_camera(*flags, ok=True):
    env = dict(os.environ, PT_RENDER_PRINT_CAMERA="1")
    out = subprocess.run([PT_RENDER, *flags], env=env, capture_output=True, text=True, timeout=60)
    if ok:
        assert out.returncode == 0, out.stderr
    return out


def test_pt_render_prints_the_lens_its_flags_resolve_to():
    assert _print_camera("-APERTURE", "0").stdout.strip() == "camera none"           # no lens
    assert _print_camera("-APERTURE", "0", "-FOCUS", "3").stdout.strip() == "camera none"
    out = _print_camera("-APERTURE", "0.5").stdout
    assert out == "camera none\nlens 0.5 20\n"                                       # the reference camera: focus 20
    out = _print_camera("-EYE", "6,3,-15", "-LOOKAT", "0,0,0", "-APERTURE", "0.5").stdout.splitlines()
    assert out[0].startswith("origin 6 3 -15") and out[-1].split()[0] == "lens"
    assert float(out[-1].split()[1]) == 0.5
    assert np.float32(out[-1].split()[2]) == np.float32(np.sqrt(36 + 9 + 225))        # |LOOKAT - EYE|
    out = _print_camera("-EYE", "6,3,-15", "-APERTURE", "0.25", "-FOCUS", "7.5").stdout.splitlines()
    assert out[-1] == "lens 0.25 7.5"


@pytest.mark.parametrize("bad", [["-APERTURE", "-0.1"], ["-APERTURE", "abc"], ["-APERTURE", "0.5x"], ["-APERTURE", "nan"],
                                 ["-APERTURE", "0.5", "-FOCUS", "0"], ["-APERTURE", "0.5", "-FOCUS", "-2"],
                                 ["-APERTURE", "0.5", "-FOCUS", "inf"], ["-APERTURE", "0.5", "-FOCUS", ""]])
def test_pt_render_refuses_malformed_lens_flags(bad):
    out = _print_camera(*bad, ok=False)
    assert out.returncode != 0


def test_pt_render_lens_flags_leave_the_config_printout_alone():
    env = dict(os.environ, PT_RENDER_PRINT_CONFIG="1")
    a = subprocess.run([PT_RENDER, "-MRR", "3"], env=env, capture_output=True, text=True, timeout=60)
    b = subprocess.run([PT_RENDER, "-MRR", "3", "-APERTURE", "0.5", "-FOCUS", "12"], env=env, capture_output=True, text=True, timeout=60)
    assert a.returncode == b.returncode == 0 and a.stdout == b.stdout


# ---- 5. the compiler's report on the lens kernels (make asm; the resource test's parser) -----------------------------------
USAGE = os.path.join(ROOT, "path-tracing_amd", "lib", "asm", "resource_usage.txt")
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
LENS = "_ZN2pt21integrate_kernel_lens"
TWIN = "_ZN2pt16integrate_kernel"
# The skybox (path regeneration) lens kernels compiled for one wave per SIMD fewer than their twins (pt_kernels.hip: lens_waves):
# at the twins' 5 waves they spilled 6 VGPRs.  Template arguments SKY, BIG, STATS, ENV.
FEWER_WAVES = {"Lb1ELb1ELb1ELb0", "Lb1ELb0ELb1ELb1", "Lb1ELb0ELb1ELb0", "Lb1ELb1ELb0ELb1", "Lb1ELb0ELb0ELb1", "Lb1ELb0ELb0ELb0"}


@pytest.fixture(scope="module")
def usage():
    srcs = [os.path.join(CSRC, f) for f in ("pt_kernels.hip", "pt_integrator_body.inc", "pt_kernels.hpp", "pt_fastfp.hpp",
                                            "pt_scene.hpp", "Makefile")]
    if not os.path.exists(USAGE) or os.path.getmtime(USAGE) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    out, name = {}, None
    for line in open(USAGE):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def _adapt(name):
    return int(re.search(r"ELi(\d+)EEEvNS_10RenderArgsE$", name).group(1))


def test_every_camera_twin_has_exactly_one_lens_kernel(usage):
    twins = sorted(k for k in usage if k.startswith(TWIN) and _adapt(k) % 2 == 1)
    lens = sorted(k for k in usage if k.startswith(LENS))
    assert len(twins) == 22, len(twins)
    assert sorted(k.replace(LENS, TWIN) for k in lens) == twins


def test_lens_kernels_keep_the_budgets_of_their_camera_twins(usage):
    seen = set()
    for k, r in usage.items():
        if not k.startswith(LENS):
            continue
        base = usage[k.replace(LENS, TWIN)]
        args = re.search(r"I(Lb\dELb\dELb\dELb\d)", k).group(1)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (k, r)
        assert r["SGPRs Spill"] <= 64, (k, r)
        assert r["LDS Size"] == base["LDS Size"], (k, r, base)
        if args in FEWER_WAVES:
            seen.add(args)
            assert r["Occupancy"] == base["Occupancy"] - 1 == 4, (k, r, base)
        else:
            assert r["Occupancy"] == base["Occupancy"], (k, r, base)
    assert seen == FEWER_WAVES
