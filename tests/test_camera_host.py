"""CPU checks of the configurable camera (pt_hip.h: pt_camera): look_at, the handle's camera and its checks, clones, the
culling envelope it implies, pt_render's camera flags, and the compiler's report on the camera twins of the integrator."""
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

pt = importlib.import_module("path-tracing_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_RENDER = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
KU = 2.0 ** -24


@pytest.fixture()
def tor(models_dir):
    s = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    yield s
    s.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_look_at_with_the_reference_inputs_is_the_reference_camera():
    cam = pt.look_at((0, 0, -20), (0, 0, 0), (0, 1, 0), math.degrees(2 * math.atan(0.5)), 0.0)
    assert cam == pt.Camera.of(*pt.REFERENCE_CAMERA), cam
    assert cam == pt.look_at((0, 0, -20), (0, 0, 0))            # the defaults are the reference's


@pytest.mark.parametrize("fov,aspect", [(53.13010235415598, 0.0), (40.0, 16 / 9), (90.0, 0.5), (10.0, 1.0)])
def test_look_at_axes_follow_fov_and_aspect(fov, aspect):
    eye, target = np.array([3.0, -2.0, 5.0]), np.array([-1.0, 4.0, 0.5])
    cam = pt.look_at(eye, target, (0.2, 1.0, 0.1), fov, aspect)
    o, r, u, f = cam.as_array().astype(np.float64)
    assert np.array_equal(o, eye.astype(np.float32))
    fwd = (target - eye) / np.linalg.norm(target - eye)
    assert np.allclose(f, fwd, atol=1e-7)
    s = 2 * math.tan(math.radians(fov) / 2)
    assert abs(np.linalg.norm(u) - s) <= 1e-6 * s
    assert abs(np.linalg.norm(r) - s * (aspect if aspect > 0 else 1.0)) <= 1e-6 * s * max(aspect, 1.0)
    for a, b in ((r, u), (r, f), (u, f)):
        assert abs(a @ b) <= 1e-6 * np.linalg.norm(a) * np.linalg.norm(b)
    # right-handed as the reference's (1,0,0), (0,1,0), (0,0,1): det(right, up, forward) > 0, and up leans to the given up
    assert np.linalg.det(np.stack([r, u, f])) > 0
    assert u @ np.array([0.2, 1.0, 0.1]) > 0


@pytest.mark.parametrize("args", [
    ((0, 0, 0), (0, 0, 0), (0, 1, 0), 50.0),          # eye == target
    ((0, 0, 0), (0, 5, 0), (0, 1, 0), 50.0),          # up parallel to the view direction
    ((0, 0, 0), (0, 0, 1), (0, 0, 0), 50.0),          # zero up
    ((0, float("nan"), 0), (0, 0, 1), (0, 1, 0), 50.0),
    ((0, 0, 0), (0, 0, 1), (0, 1, 0), 0.0),           # no field of view
    ((0, 0, 0), (0, 0, 1), (0, 1, 0), 180.0),
])
def test_look_at_refuses_degenerate_input(args):
    with pytest.raises(pt.PtError) as e:
        pt.look_at(*args)
    assert e.value.status == pt.PT_ERR_INVALID_ARGUMENT


def test_scene_camera_round_trips_and_resets(tor):
    assert tor.camera() is None
    cam = pt.look_at((1.5, -2.0, -15.0), (0.5, 0.25, 3.0), fov_y=35.0, aspect=1.5)
    tor.set_camera(cam)
    assert tor.camera() == cam
    tor.set_camera(pt.REFERENCE_CAMERA)            # a tuple of four triples works too
    assert tor.camera() == pt.Camera.of(*pt.REFERENCE_CAMERA)
    tor.set_camera(None)
    assert tor.camera() is None


@pytest.mark.parametrize("bad,status", [
    (((0, 0, -20), (1, 0, 0), (0, 1, 0), (0, 0, 0)), "PT_ERR_INVALID_ARGUMENT"),                  # zero forward
    (((0, 0, -20), (1, 0, 0), (0, 1, 0), (0, 1, 0)), "PT_ERR_INVALID_ARGUMENT"),                  # up parallel to forward
    (((0, 0, -20), (1, 0, 0), (2, 0, 0), (0, 0, 1)), "PT_ERR_INVALID_ARGUMENT"),                  # right parallel to up
    (((0, 0, -20), (1, 0, 0), (0, 1, 0), (1, 1, 0)), "PT_ERR_INVALID_ARGUMENT"),                  # forward in the right-up plane
    (((0, 0, -20), (1e-3, 0, 0), (0, 1e-3, 0), (1e-3, 1e-3, 1e-12)), "PT_ERR_INVALID_ARGUMENT"),  # nearly coplanar (relative test)
    (((0, float("nan"), -20), (1, 0, 0), (0, 1, 0), (0, 0, 1)), "PT_ERR_INVALID_ARGUMENT"),
    (((0, 0, -20), (1, 0, 0), (0, float("inf"), 0), (0, 0, 1)), "PT_ERR_INVALID_ARGUMENT"),
    (((0, 0, -5000), (1, 0, 0), (0, 1, 0), (0, 0, 1)), "PT_ERR_UNSUPPORTED"),                     # beyond PT_CAMERA_MAX_ORIGIN
    (((4096.5, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)), "PT_ERR_UNSUPPORTED"),
])
def test_bad_cameras_are_refused_and_leave_the_handle_alone(tor, bad, status):
    good = pt.look_at((2, 3, -12), (0, 0, 0), fov_y=45.0)
    tor.set_camera(good)
    with pytest.raises(pt.PtError) as e:
        tor.set_camera(bad)
    assert e.value.status == getattr(pt, status)
    assert tor.camera() == good
    tor.set_camera(None)
    with pytest.raises(pt.PtError):
        tor.set_camera(bad)
    assert tor.camera() is None


def test_the_origin_bound_is_inclusive(tor):
    tor.set_camera(((0, 0, -4096.0), (1, 0, 0), (0, 1, 0), (0, 0, 1)))
    assert tor.camera().as_array()[0, 2] == -4096.0


def test_clones_inherit_the_camera_of_the_handle_they_are_made_from(tor):
    cam = pt.look_at((4, 1, -18), (0, -1, 0), fov_y=60.0, aspect=2.0)
    tor.set_camera(cam)
    c1 = tor.clone_to_device(-1)
    assert c1.camera() == cam
    c1.set_camera(None)                       # a copy's camera is its own
    assert tor.camera() == cam and c1.camera() is None
    tor.set_camera(None)
    c2 = tor.clone_to_device(-1)
    assert c2.camera() is None
    c1.close()
    c2.close()


def _tables(scene, eps=1e-4):
    t = scene.cull_tables(eps)
    lay = scene.cull_layout(eps)
    return [t["cluster_sphere"], t["spheres"], t["bary"], np.array(list(t["constants"].values()), np.float32),
            lay["slot_triangle"], lay["bvh"]]


def _r_org(scene, eps=1e-4):
    """k2 = kU (24 sqrt(3) + 8) r_org (pt_cull_tables.cpp, margins of the barycentric test)."""
    return scene.cull_tables(eps)["constants"]["k2"] / (KU * (24 * math.sqrt(3) + 8))


@pytest.mark.parametrize("eye", [(0, 0, -20), (5, -7, 12), (19.5, 19.5, -19.5), (0, 0, 0)])
def test_an_eye_inside_the_default_envelope_shares_the_camera_free_tables(models_dir, eye):
    plain = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    want = _tables(plain)
    s = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    s.set_camera(pt.look_at(eye, (0, 1, 3), fov_y=70.0))
    got = _tables(s)
    for a, b in zip(want, got):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    plain.close()
    s.close()


def test_a_far_eye_widens_the_envelope(tor):
    r_default = _r_org(tor)
    assert 20.9 < r_default < 40.0
    tor.set_camera(pt.look_at((0, 0, -200), (0, 0, 0), fov_y=10.0))
    r_far = _r_org(tor)
    assert r_far >= 201.0 * (1 - 1e-6), r_far
    assert r_far <= 201.0 * (1 + 1e-6), r_far
    tor.set_camera(None)                      # and back: the default tables again
    assert _r_org(tor) == pytest.approx(r_default, rel=1e-7)


def _print_camera(*flags):
    env = dict(os.environ, PT_RENDER_PRINT_CAMERA="1")
    out = subprocess.run([PT_RENDER, *flags], env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return out.stdout


def test_pt_render_prints_the_camera_its_flags_resolve_to():
    assert _print_camera().strip() == "camera none"
    assert _print_camera("-MRR", "3", "--W", "64").strip() == "camera none"
    ref = _print_camera("-EYE", "0,0,-20", "-LOOKAT", "0,0,0", "-UP", "0,1,0", "-FOV", "53.13010235415598", "-ASPECT", "0")
    assert ref == "origin 0 0 -20\nright 1 0 0\nup 0 1 0\nforward 0 0 1\n"
    assert _print_camera("-FOV", "53.13010235415598") == ref            # any one flag sets a camera, the others default
    out = _print_camera("-EYE", "3,4,-10", "-LOOKAT", "0,0,1", "-FOV", "40", "-ASPECT", "1.5")
    rows = {ln.split()[0]: np.array(ln.split()[1:], np.float64) for ln in out.strip().splitlines()}
    want = pt.look_at((3, 4, -10), (0, 0, 1), fov_y=40.0, aspect=1.5).as_array()
    for k, name in enumerate(("origin", "right", "up", "forward")):
        assert np.array_equal(rows[name].astype(np.float32), want[k]), name


def test_pt_render_camera_flags_leave_the_config_printout_alone():
    env = dict(os.environ, PT_RENDER_PRINT_CONFIG="1")
    a = subprocess.run([PT_RENDER, "-MRR", "3"], env=env, capture_output=True, text=True, timeout=60)
    b = subprocess.run([PT_RENDER, "-MRR", "3", "-EYE", "1,2,-30", "-FOV", "30"], env=env, capture_output=True, text=True, timeout=60)
    assert a.returncode == b.returncode == 0 and a.stdout == b.stdout


@pytest.mark.parametrize("bad", [["-EYE", "1,2"], ["-LOOKAT", "1,2,3,4"], ["-UP", "a,b,c"], ["-EYE", "0,0,0", "-LOOKAT", "0,0,0"]])
def test_pt_render_refuses_malformed_camera_flags(bad):
    env = dict(os.environ, PT_RENDER_PRINT_CAMERA="1")
    out = subprocess.run([PT_RENDER, *bad], env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode != 0


# ---- the compiler's report on the camera twins (make asm; the resource test's parser) --------------------------------------
USAGE = os.path.join(ROOT, "path-tracing_amd", "lib", "asm", "resource_usage.txt")
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")


@pytest.fixture(scope="module")
def usage():
    srcs = [os.path.join(CSRC, f) for f in ("pt_kernels.hip", "pt_kernels.hpp", "pt_fastfp.hpp", "pt_scene.hpp", "Makefile")]
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


def test_every_instantiation_has_its_camera_twin(usage):
    kernels = [k for k in usage if k.startswith("_ZN2pt16integrate_kernel")]
    plain = [k for k in kernels if _adapt(k) % 2 == 0]
    twins = [k for k in kernels if _adapt(k) % 2 == 1]
    assert len(plain) == len(twins) >= 20, (len(plain), len(twins))   # (22: the box tree has no narrow variant)
    assert sorted(re.sub(r"ELi(\d+)E", lambda m: "ELi%dE" % (int(m.group(1)) & ~1), k) for k in twins) == sorted(plain)


def test_camera_twins_keep_the_budgets_of_their_camera_free_kernels(usage):
    for k, r in usage.items():
        if not k.startswith("_ZN2pt16integrate_kernel") or _adapt(k) % 2 == 0:
            continue
        base = usage[re.sub(r"ELi(\d+)E", lambda m: "ELi%dE" % (int(m.group(1)) & ~1), k)]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (k, r)
        assert r["SGPRs Spill"] <= 64, (k, r)
        assert r["Occupancy"] == base["Occupancy"] and r["LDS Size"] == base["LDS Size"], (k, r, base)
