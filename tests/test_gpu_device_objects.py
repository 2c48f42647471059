"""Every device allocation, event and stream of the host layer has one owner (csrc/pt_device_mem.hpp) and the test-hook build
counts the owners that hold something: after each cycle of create / use / destroy below the count must be back where it was,
exactly.  (The library's own count, not a reading of free device memory, which other users of a shared card would disturb.)
The cases are the smallest that reach each owner; two of them also pin that the results did not move."""
import contextlib
import importlib

import numpy as np
import pytest

import denoise_restatement as R
import oracle_lib as O
import temporal_restatement as T

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
C = pt.C


@pytest.fixture(scope="module")
def hooks():
    assert pt.device_count() >= 1, "no HIP device: there is no CPU fallback"
    L = pt.load_library(pt.TESTHOOKS_LIB_PATH)
    L.pt_test_set_mutation(b"reset", 0.0)
    return L


@contextlib.contextmanager
def balanced(L):
    before = L.pt_test_live_device_objects()
    yield before
    assert L.pt_test_live_device_objects() == before


def _tor(L, models_dir):
    return pt.Scene.load_obj(models_dir, "Tor.obj", device=0, library=L)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _denoise(L, W, H, s, s2, c, f, levels):
    """pt_denoise_host of library L (pt.denoise calls the product library); returns the status and the outputs."""
    n = W * H
    prm = pt.DenoiseParams(levels, 0.0, 0.0, 0, 0)
    mean, cout, ms = np.zeros((n, 3), np.float32), np.zeros(n, np.int32), C.c_float()
    rc = L.pt_denoise_host(0, W, H, pt._fp(s), pt._fp(s2), pt._ip(c), pt._fp(f["position"]), pt._fp(f["normal"]), pt._fp(f["albedo"]),
                           pt._ip(f["hit_index"]), C.byref(prm), pt._fp(mean), pt._ip(cout), C.byref(ms))
    return rc, mean, cout


def test_scene_render_host_cycle(hooks, models_dir, oracle_scene, tmp_path):
    sky = str(tmp_path / "sky.bmp")
    O.write_bmp(sky, np.random.default_rng(2).integers(0, 256, (6, 9, 3)).astype(np.uint8))
    with balanced(hooks) as before:
        g = _tor(hooks, models_dir)
        g.render_host(16, 8, 2, 8)
        s, s2, c, st = g.render_host(24, 16, 2, 8)
        assert hooks.pt_test_live_device_objects() > before        # the count sees the scene's tables, band, stream, events
        g.render_host(40, 24, 2, 8)                                 # the band and the scheduler words regrow
        g.render_host(24, 16, 2, 8, eps=1e-3)                       # the cull tables are replaced
        g.set_skybox(sky)
        g.render_host(24, 16, 2, 8, want_stats=False)
        g.set_skybox(None)
        g.render_host(24, 16, 2, 8, want_stats=False)
        g.close()
    # the results did not move: the counter-policy oracle, bit for bit
    rs, rs2, rc, rst = O.render(oracle_scene, 24, 16, 2, 8, error=-1.0, seed=42, rng=O.RNG_COUNTER, trig=O.TRIG_PORTABLE)
    assert st["segments"] == rst["segments"] and np.array_equal(c, rc)
    assert np.array_equal(_bits(s), _bits(rs)) and np.array_equal(_bits(s2), _bits(rs2))


def test_session_with_owned_planes_cycle(hooks, models_dir):
    g = _tor(hooks, models_dir)
    whole = g.render_host(24, 16, 2, 8, rows=(8, 16), want_stats=False)      # (the scene's own cull tables exist from here on)
    with balanced(hooks):
        ses = pt.Session(g, 24, 16, rows=(8, 16))
        st = [ses.render(k, 1, 8, want_stats=True) for k in range(2)]
        s, s2, c = ses.read()
        ses.close()
    assert st[0]["samples_traced"] == st[1]["samples_traced"] == 8 * 24 and c.any()
    assert np.array_equal(_bits(s), _bits(whole[0])) and np.array_equal(_bits(s2), _bits(whole[1])) and np.array_equal(c, whole[2])
    g.close()


def test_one_shot_entry_points_cycle(hooks, models_dir):
    g = _tor(hooks, models_dir)
    g.render_host(16, 8, 1, 8, want_stats=False)                    # (the scene's own lazily made objects exist from here on)
    rng = np.random.default_rng(3)
    with balanced(hooks):
        for n in (1, 65):
            d = rng.normal(size=(n, 3)).astype(np.float32)
            d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
            idx, t = g.trace_rays(np.tile(np.float32([0, 0, -20]), (n, 1)), d)
            assert (idx >= -1).all()
    img = (rng.random((7, 9, 3), dtype=np.float32) * 255).astype(np.float32)
    with balanced(hooks):
        for gauss, median in ((1, 0), (0, 3), (1, 3)):
            out = img.copy()
            assert hooks.pt_post_filter_host(0, 9, 7, pt._fp(out), gauss, median) == pt.PT_OK
            assert np.isfinite(out).all() and not np.array_equal(out, img)
    W, H = 17, 9
    s, s2, c, _ = g.render_host(W, H, 2, 8, want_stats=False)
    with balanced(hooks):
        f = g.render_features(W, H)
        assert (f["hit_index"] >= -1).all()
        for levels in (0, 1, 3):
            rc, mean, cout = _denoise(hooks, W, H, s, s2, c, f, levels)
            assert rc == pt.PT_OK and np.isfinite(mean).all() and (levels > 0 or np.array_equal(cout, c))
    # the image-space stages alone on a 9 x 7 mean image (one pixel without samples), each with the stage on and -- where its
    # parameters can say so -- off: PT_OK (anything else raises), finite output, and a kernel time only where kernels ran
    mean = (rng.random((7, 9, 3), dtype=np.float32) * np.float32(4)).astype(np.float32)
    cnt = np.ones((7, 9), np.int32)
    cnt[3, 4] = 0
    stages = {"bloom": lambda on: pt.bloom(0, mean, cnt, strength=0.5 if on else 0.0, want_ms=True, library=hooks),
              "local": lambda on: pt.local_exposure(0, mean, cnt, strength=1.0 if on else 0.0, want_ms=True, library=hooks),
              "optics": lambda on: pt.optics(0, mean, cnt, k1=-0.1 if on else 0.0, ca=0.01 if on else 0.0, want_ms=True, library=hooks)}
    for name, run in stages.items():
        for on in (True, False):
            with balanced(hooks):
                *out, ms = run(on)
            assert all(np.isfinite(o).all() for o in out) and out[0].shape == mean.shape, (name, on)
            assert (ms > 0) if on else (ms == 0 and np.array_equal(_bits(out[0]), _bits(mean))), (name, on, ms)
    with balanced(hooks):                                           # (the meter and the upsampler have no "off")
        hist, ms = pt.meter(mean, cnt, want_ms=True, library=hooks)
    assert ms > 0 and int(hist.sum()) == 9 * 7 - 1
    lo, clo = np.ascontiguousarray(mean[:4, :6].reshape(-1, 3)), np.ascontiguousarray(cnt[:4, :6].reshape(-1))
    with balanced(hooks):
        f = g.render_features(12, 8)
        prm = pt.UpsampleParams(2, 0.0, 0, 0)
        up, cup, ms = np.zeros((12 * 8, 3), np.float32), np.zeros(12 * 8, np.int32), C.c_float()
        rc = hooks.pt_upsample_host(0, 12, 8, pt._fp(lo), pt._ip(clo), pt._fp(f["position"]), pt._fp(f["normal"]), pt._fp(f["albedo"]),
                                    pt._ip(f["hit_index"]), C.byref(prm), pt._fp(up), pt._ip(cup), C.byref(ms))
    assert rc == pt.PT_OK and np.isfinite(up).all() and ms.value > 0
    g.close()


def test_temporal_cycle_and_restatement(hooks, models_dir, oracle_scene):
    W, H = 24, 16
    g = _tor(hooks, models_dir)
    frames = [g.render_host(W, H, 2, 8, pass_begin=2 * i, want_stats=False)[:3] for i in range(4)]
    moved = pt.look_at((2.0, 0.5, -19.0), (0.0, 0.0, 0.0), fov_y=55.0, aspect=W / H, library=hooks)
    ref = T.Temporal(W, H)
    # (camera, denoise, reset first): the first frame, a static one with the lazily made denoiser planes, one after the eye moved,
    # and a first frame again after a reset -- with the unfiltered mean (levels 0)
    steps = ((None, None, False), (None, {"levels": 2}, False), (moved, {"levels": 2}, False), (moved, {"levels": 0}, True))
    with balanced(hooks):
        t = pt.Temporal(g, W, H)
        for i, (cam, dn, reset) in enumerate(steps):
            if reset:
                t.reset()
                ref.reset()
            g.set_camera(cam)
            arr = None if cam is None else cam.as_array()
            got = t.push(*frames[i], denoise=dn)
            want = ref.push(*frames[i], R.features(oracle_scene, W, H, camera=arr), arr)
            for k in ("count", "history_frames", "sum", "sum2"):
                assert np.array_equal(_bits(got[k]), _bits(want[k])), (i, k)
            if dn is not None:
                assert np.isfinite(got["mean_rgb"]).all()
        t.close()
    # the mean image of the last push is the merged accumulators' own mean
    cnt = want["count"].astype(np.float32)[:, None]
    mean = np.where(cnt != 0, want["sum"] / np.where(cnt != 0, cnt, np.float32(1)), want["sum"]).astype(np.float32)
    assert np.array_equal(_bits(got["mean_rgb"]), _bits(mean)) and np.array_equal(got["mean_count"], want["count"])
    g.close()


@pytest.mark.parametrize("W,H,stride", [(16, 16, 2), (16, 8, 1)])
def test_rehearsed_frame_cycle(hooks, models_dir, W, H, stride):
    """Two bands on device 0: 16 x 16 is split by interleaved tile rows (no staging: both bands are on the root); 16 x 8 has one
    tile row, so contiguous bands, the root's rendering into the frame's own planes."""
    g = _tor(hooks, models_dir)
    whole = g.render_host(W, H, 2, 8, want_stats=False)
    with balanced(hooks):
        fr = pt.Frame(g, [0, 0], W, H, flags=pt.FRAME_REHEARSE)
        info = fr.info()
        assert info["bands"] == 2 and info["row_stride"] == stride and info["transport"] == "device_copies"
        fr.render(0, 2, 8)
        fr.gather()
        s, s2, c = fr.read()
        fr.close()
    for a, b in zip((s, s2, c), whole[:3]):
        assert np.array_equal(_bits(a), _bits(b))
    g.close()


def test_refused_calls_leave_the_count_alone(hooks, models_dir):
    g = _tor(hooks, models_dir)
    h = C.c_void_p()
    W, H = 17, 9
    z3, zi = np.zeros((W * H, 3), np.float32), np.zeros(W * H, np.int32)
    f = {"position": z3, "normal": z3, "albedo": z3, "hit_index": zi}
    devs = np.array([9999], np.int32)
    with balanced(hooks):
        assert hooks.pt_session_create(g._h, 24, 16, 8, 17, C.byref(h)) == pt.PT_ERR_INVALID_ARGUMENT and not h.value
        assert hooks.pt_temporal_create(g._h, 0, 16, 1e-4, C.byref(h)) == pt.PT_ERR_INVALID_ARGUMENT and not h.value
        assert _denoise(hooks, W, H, z3, z3, zi, f, 9)[0] == pt.PT_ERR_INVALID_ARGUMENT
        assert hooks.pt_frame_create(g._h, pt._ip(devs), 1, 16, 16, 0, C.byref(h)) == 4 and not h.value     # PT_ERR_NO_DEVICE
    g.close()


def test_display_reaches_every_lazy_plane_set_of_one_handle(hooks, models_dir):
    """One display, every plane set it allocates on demand: the filter planes, the temporal stage with its denoiser planes, the
    scaled planes at two scales (the second replaces the first), the bloom pyramids of both output sizes, local exposure's planes,
    the optics stage's mean image, the LUT's device copy (a larger LUT replaces it) -- and all of the stages' sets again for the
    scaled output.  All of it goes with the handle, and what an earlier present allocated does not reach a later result."""
    W, H = 24, 16
    g = _tor(hooks, models_dir)
    ses = pt.Session(g, W, H)
    ses.render(0, 2, 8)                                             # (the scene's own cull tables exist from here on)
    look = {"grade": {"curve": "aces", "auto_exposure": True}, "bloom": {"strength": 0.5}}
    stages, lens = {"local": {"strength": 1.0}}, {"k1": -0.1, "ca": 0.01, "vignette": 0.5}
    grids = [np.stack(np.meshgrid(*[np.linspace(0, 1, n, dtype=np.float32)] * 3, indexing="ij")[::-1], axis=-1) for n in (2, 5)]
    luts = [pt.Lut.create(np.sqrt(a), library=hooks) for a in grids]           # [blue, green, red] -> (r, g, b), brightened
    with balanced(hooks):
        d = pt.Display(ses)
        created = hooks.pt_test_live_device_objects()
        assert d.present()[0].shape == (H, W, 3)
        d.present(denoise={"levels": 2})
        d.present(temporal=True, denoise={"levels": 2})
        scaled, _ = d.present(upsample={"scale": 2})
        assert d.present(upsample={"scale": 3})[0].shape == (3 * H, 3 * W, 3)
        d.present(**look)
        assert d.present(upsample={"scale": 2}, **look)[0].shape == (2 * H, 2 * W, 3)
        assert hooks.pt_test_live_device_objects() > created
        held = hooks.pt_test_live_device_objects()
        d.present(**look, **stages)                                 # local exposure's planes
        d.present(**look, **stages, optics=lens)                    # the optics stage's mean image
        assert hooks.pt_test_live_device_objects() == held + 2
        assert d.present(**look, **stages, optics=lens, colour={"saturation": 0.8, "lut": luts[0]})[0].any()
        assert hooks.pt_test_live_device_objects() == held + 3      # the LUT's device copy; the 5^3 one takes its place
        everything, _ = d.present(**look, **stages, optics=lens, colour={"saturation": 0.8, "lut": luts[1]})
        assert hooks.pt_test_live_device_objects() == held + 3
        assert d.present(upsample={"scale": 2}, **look, **stages, optics=lens, colour={"lut": luts[1]})[0].shape == (2 * H, 2 * W, 3)
        assert hooks.pt_test_live_device_objects() == held + 6      # the scaled output's local, optics and LUT sets (its bloom's exist)
        fresh = pt.Display(ses)
        want, _ = fresh.present(upsample={"scale": 2})
        want_everything, _ = fresh.present(**look, **stages, optics=lens, colour={"saturation": 0.8, "lut": luts[1]})
        fresh.close()
        d.reset()
        d.close()
    assert scaled.shape == (2 * H, 2 * W, 3) and scaled.any() and np.array_equal(scaled, want)
    assert everything.shape == (H, W, 3) and everything.any() and np.array_equal(everything, want_everything)
    for lut in luts:
        lut.close()
    ses.close()
    g.close()
