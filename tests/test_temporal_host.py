"""Temporal accumulation without a GPU: struct layout, symbols, argument checks and status codes of pt_temporal_*, and the numpy
restatement of include/pt_hip.h's text (tests/temporal_restatement.py) on oracle frames and on analytic scenes -- what the
stage must do before any device is asked to reproduce it bit for bit (tests/test_gpu_temporal.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import denoise_restatement as R
import oracle_lib as O
import temporal_restatement as T

pt = importlib.import_module("path-tracing_amd")
F32 = np.float32
INF = float("inf")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frame(W, H, seed=3):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 5, W * H).astype(np.int32)
    s = (rng.random((W * H, 3), dtype=np.float32) * c[:, None]).astype(np.float32)
    return s, (s * s).astype(np.float32), c


# ---- the ABI ----------------------------------------------------------------------------------------------------------

def test_struct_layout_and_symbols():
    assert C.sizeof(pt.TemporalParams) == 12
    assert [n for n, _ in pt.TemporalParams._fields_] == ["max_frames", "sigma_plane", "min_normal_dot"]
    for name in ("pt_temporal_create", "pt_temporal_push_host", "pt_temporal_reset", "pt_temporal_destroy"):
        assert name in pt.ABI_SYMBOLS and getattr(pt.lib(), name) is not None
    assert pt.lib().pt_abi_version() == 5
    assert (T.DEFAULT_MAX_FRAMES, T.DEFAULT_SIGMA_PLANE, T.DEFAULT_MIN_NORMAL_DOT) == (F32(32), F32(0.1), F32(0.9))


def test_create_argument_checks(models_dir):
    L = pt.lib()
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    h = C.c_void_p()
    assert L.pt_temporal_create(None, 8, 8, 1e-4, C.byref(h)) == 1
    assert L.pt_temporal_create(sc._h, 8, 8, 1e-4, None) == 1
    assert L.pt_temporal_create(sc._h, 0, 8, 1e-4, C.byref(h)) == 1 and L.pt_temporal_create(sc._h, 8, -1, 1e-4, C.byref(h)) == 1
    assert L.pt_temporal_create(sc._h, 8, 8, float("nan"), C.byref(h)) == 1
    assert L.pt_temporal_create(sc._h, 1 << 15, 1 << 15, 1e-4, C.byref(h)) == 1          # too large
    assert not h.value
    with pytest.raises(pt.PtError) as e:                 # a host-only scene: no device, and no CPU fallback
        pt.Temporal(sc, 8, 8)
    assert e.value.status == 4 and "fallback" in str(e.value)
    assert L.pt_temporal_reset(None) == 1
    assert L.pt_temporal_push_host(None, None, None, None, None, None, None, None, None, None, None, None, None) == 1
    L.pt_temporal_destroy(None)                          # a no-op


# ---- the restatement: first frame, static camera ----------------------------------------------------------------------

def _flat_features(W, H, camera=None, z=5.0):
    """A wall facing +z's viewers at depth z: features from the centre rays of `camera`."""
    o, d = R.centre_rays(W, H, camera)
    t = ((F32(z) - o[:, 2]) / d[:, 2]).astype(np.float32)
    return {"hit_index": np.zeros(W * H, np.int32), "position": (o + d * t[:, None]).astype(np.float32),
            "normal": np.tile(np.array([0, 0, -1], np.float32), (W * H, 1))}


def test_first_frame_is_the_frame():
    W, H = 23, 17
    s, s2, c = _frame(W, H)
    t = T.Temporal(W, H)
    for _ in range(2):
        out = t.push(s, s2, c, _flat_features(W, H))
        assert np.array_equal(_bits(out["sum"]), _bits(s)) and np.array_equal(_bits(out["sum2"]), _bits(s2))
        assert np.array_equal(out["count"], c) and (out["history_frames"] == 1).all()
        t.reset()


def test_static_sequence_is_progressive_rendering(oracle_scene):
    """K oracle frames of Tor.obj with disjoint pass ranges, the camera at rest, no cap: the merged accumulators are the frames'
    sums added in frame order, the counts add up exactly, and the mean is that of ONE K * spp render up to the reordering of the
    float sums (relative 1e-5: float32 sums of at most a few hundred terms carry a few 1e-7 each way)."""
    W, H, spp, K = 48, 36, 12, 4
    f = R.features(oracle_scene, W, H)
    t = T.Temporal(W, H)
    acc_s, acc_c = np.zeros((W * H, 3), np.float32), np.zeros(W * H, np.int32)
    for i in range(K):
        s, s2, c, _ = O.render(oracle_scene, W, H, spp, 8, error=-1.0, seed=42, pass_begin=i * spp)
        assert (c == 0).any()
        if i == 0:
            first_live = c > 0
        out = t.push(s, s2, c, f, max_frames=INF)
        acc_s, acc_c = (s + acc_s if i else s.copy()), acc_c + c
        assert np.array_equal(out["count"], acc_c)
        assert np.array_equal(_bits(out["sum"]), _bits(acc_s))
        assert (out["history_frames"][first_live] == i + 1).all()      # (a pixel without any sample so far has nothing to keep)
    ws, _, wc, _ = O.render(oracle_scene, W, H, K * spp, 8, error=-1.0, seed=42)
    assert np.array_equal(out["count"], wc)
    live = wc > 0
    m, wm = out["sum"][live] / wc[live, None], ws[live] / wc[live, None]
    assert np.all(np.abs(m - wm) <= 1e-5 * np.abs(wm))


def test_static_sequence_with_a_cap():
    """max_frames = 2: from the fourth frame on the history is scaled to two frames' worth -- the output count stops growing
    and history_frames settles at 3."""
    W, H = 9, 7
    c = np.full(W * H, 8, np.int32)
    s = np.tile(np.array([2.0, 4.0, 1.0], np.float32), (W * H, 1))
    f = _flat_features(W, H)
    t = T.Temporal(W, H)
    counts, frames = [], []
    for i in range(7):
        out = t.push(s, s * s, c, f, max_frames=2.0)
        counts.append(int(out["count"][0]))
        frames.append(float(out["history_frames"][0]))
        assert (out["count"] == counts[-1]).all()
        mean = out["sum"] / out["count"][:, None].astype(np.float32)
        assert np.allclose(mean, s / 8, rtol=1e-6)             # scaling sums and counts alike keeps the mean
    assert counts == [8, 16, 24, 24, 24, 24, 24] and frames == [1, 2, 3, 3, 3, 3, 3]


# ---- the restatement: geometry on analytic scenes ------------------------------------------------------------------------

def _radiance(P):
    """A smooth function of the world position."""
    return np.stack([0.5 + 0.3 * np.sin(0.35 * P[:, 0]), 0.5 + 0.3 * np.cos(0.3 * P[:, 1]), 0.4 + 0.02 * P[:, 0]], 1).astype(np.float32)


def _variation(img, W, H):
    """The largest change of `img` [n, 3] between a pixel and any of its 8 neighbours."""
    a = img.reshape(H, W, 3).astype(np.float64)
    d = [np.abs(a[1:, :] - a[:-1, :]).max(), np.abs(a[:, 1:] - a[:, :-1]).max(), np.abs(a[1:, 1:] - a[:-1, :-1]).max(),
         np.abs(a[1:, :-1] - a[:-1, 1:]).max()]
    return max(d)


def _history_mean(out, s, c):
    """Mean of the history part of a push's outputs (pixels with history)."""
    n = (out["count"] - c).astype(np.float32)
    with np.errstate(all="ignore"):
        return (out["sum"] - s) / n[:, None], n > 0


@pytest.mark.parametrize("move", ["translate", "rotate"])
def test_history_arrives_at_the_right_pixels(move):
    """A wall, radiance a smooth function of the world position, one sample per pixel.  After the camera moves, the history a
    pixel receives is the bilinear interpolation of that function over the previous frame's pixel grid: it misses the function
    at the pixel's own position by no more than the function changes across one pixel of that grid."""
    W, H = 64, 48
    cam0 = pt.look_at((0.0, 0.0, -20.0), (0.0, 0.0, 5.0), fov_y=50.0, aspect=W / H).as_array()
    cam1 = (pt.look_at((1.7, -0.6, -20.0), (1.7, -0.6, 5.0), fov_y=50.0, aspect=W / H) if move == "translate"
            else pt.look_at((0.0, 0.0, -20.0), (2.5, 1.0, 5.0), fov_y=50.0, aspect=W / H)).as_array()
    f0, f1 = _flat_features(W, H, cam0), _flat_features(W, H, cam1)
    c = np.ones(W * H, np.int32)
    s0, s1 = _radiance(f0["position"]), _radiance(f1["position"])
    t = T.Temporal(W, H)
    t.push(s0, s0 * s0, c, f0, cam0)
    out = t.push(s1, s1 * s1, c, f1, cam1)
    got, have = _history_mean(out, s1, c)
    assert np.array_equal(have, out["history_frames"] == 2)
    assert have.mean() > 0.8                                         # the views overlap; the pixels that entered the image have none
    assert (out["history_frames"][~have] == 1).all()
    bound = _variation(s0, W, H)
    assert bound < 0.1                                               # ... of values that span 0.6: the bound means something
    assert np.abs(got[have].astype(np.float64) - s1[have]).max() <= bound
    assert (out["count"][have] == 2).all()
    # and the pixels without history are exactly those whose position the previous camera did not see
    inv = T.camera_inverse(cam0).astype(np.float64)
    e = f1["position"].astype(np.float64) - cam0[0]
    fx, fy = (inv[0] @ e.T / (inv[2] @ e.T) + 0.5) * W, (0.5 - inv[1] @ e.T / (inv[2] @ e.T)) * H
    well_inside = (fx > 0.01) & (fx < W - 1.01) & (fy > 0.01) & (fy < H - 1.01)
    outside = (fx < -1.01) | (fx > W + 0.01) | (fy < -1.01) | (fy > H + 0.01)
    assert have[well_inside].all() and not have[outside].any()


STRIP_Z, STRIP_HALF = -10.0, 3.0


def _strip_features(W, H, camera):
    """The wall at z = 5 and, in front of it, a strip |x| < 3 at z = -10 (both facing the camera)."""
    o, d = R.centre_rays(W, H, camera)
    t_strip = ((F32(STRIP_Z) - o[:, 2]) / d[:, 2]).astype(np.float32)
    x_strip = o[:, 0] + d[:, 0] * t_strip
    on = np.abs(x_strip) < STRIP_HALF
    t = np.where(on, t_strip, (F32(5) - o[:, 2]) / d[:, 2]).astype(np.float32)
    return {"hit_index": np.where(on, 1, 0).astype(np.int32), "position": (o + d * t[:, None]).astype(np.float32),
            "normal": np.tile(np.array([0, 0, -1], np.float32), (W * H, 1))}, on


def test_disocclusion_has_no_history():
    """A nearer strip moves with parallax when the camera translates: the wall pixels it uncovers find only the strip where they
    were -- 15 units off their tangent plane -- and start over."""
    W, H = 96, 32
    cam0 = pt.look_at((0.0, 0.0, -20.0), (0.0, 0.0, 5.0), fov_y=40.0, aspect=W / H).as_array()
    cam1 = pt.look_at((4.0, 0.0, -20.0), (4.0, 0.0, 5.0), fov_y=40.0, aspect=W / H).as_array()
    (f0, on0), (f1, on1) = _strip_features(W, H, cam0), _strip_features(W, H, cam1)
    c = np.ones(W * H, np.int32)
    s0, s1 = _radiance(f0["position"]), _radiance(f1["position"])
    t = T.Temporal(W, H)
    t.push(s0, s0 * s0, c, f0, cam0)
    out = t.push(s1, s1 * s1, c, f1, cam1)
    # where the previous camera's line of sight to a wall point crosses the strip's plane
    P = f1["position"].astype(np.float64)
    depth = STRIP_Z + 20.0
    cross = cam0[0, 0] + (P[:, 0] - cam0[0, 0]) * (depth / (P[:, 2] + 20.0))
    pixel = 2 * depth * np.tan(np.radians(20.0)) * (W / H) / W            # one pixel's width at the strip's depth
    uncovered = ~on1 & (np.abs(cross) < STRIP_HALF - 2 * pixel)
    clear = ~on1 & (np.abs(cross) > STRIP_HALF + 2 * pixel)
    assert uncovered.sum() >= 3 * H
    assert (out["history_frames"][uncovered] == 1).all() and (out["count"][uncovered] == 1).all()
    middle = lambda a: a.reshape(H, W)[:, 12:-12].reshape(-1)              # (the image's edges saw something else before)
    assert (middle(out["history_frames"])[middle(clear)] == 2).all()
    assert (middle(out["history_frames"])[middle(on1)] == 2).mean() > 0.7   # the strip itself keeps its history, but for its edges


def test_the_sky_is_reprojected_by_rotation():
    """All-miss frames: the history follows the view direction, whatever the translation."""
    W, H = 60, 40
    cam0 = pt.look_at((0.0, 0.0, -20.0), (0.0, 0.0, 0.0), fov_y=60.0, aspect=W / H).as_array()
    cam1 = pt.look_at((3.0, 1.0, -18.0), (5.0, 2.0, 2.0), fov_y=60.0, aspect=W / H).as_array()
    zeros = np.zeros((W * H, 3), np.float32)
    feat = {"hit_index": np.full(W * H, -1, np.int32), "position": zeros, "normal": zeros}

    def sky(cam):
        _, d = R.centre_rays(W, H, cam)
        return np.stack([0.5 + 0.4 * d[:, 0], 0.5 + 0.4 * d[:, 1], 0.5 + 0.3 * d[:, 0] * d[:, 1]], 1).astype(np.float32)

    c = np.ones(W * H, np.int32)
    s0, s1 = sky(cam0), sky(cam1)
    t = T.Temporal(W, H)
    t.push(s0, s0 * s0, c, feat, cam0)
    out = t.push(s1, s1 * s1, c, feat, cam1)
    got, have = _history_mean(out, s1, c)
    assert have.mean() > 0.6 and np.array_equal(have, out["history_frames"] == 2)
    assert np.abs(got[have].astype(np.float64) - s1[have]).max() <= _variation(s0, W, H)
    # a wall pixel never takes history from the sky
    fw = _flat_features(W, H, cam1)
    sw = _radiance(fw["position"])
    assert (t.push(sw, sw * sw, c, fw, cam0)["history_frames"] == 1).all()


# ---- the restatement: what it is worth ---------------------------------------------------------------------------------

def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def test_merged_and_denoised_beats_the_last_frame_denoised(oracle_scene):
    """Static oracle sequence, 4 frames x 16 spp of Tor.obj, 128 x 128, -ERR -1, against 1024 spp of the same view (the recipe of
    tests/test_denoise_host.py): the merged frame, denoised, is closer to the truth than the last frame denoised alone (RMSE on
    the tone-mapped float image, 0 .. 255 scale).  Measured: see DESIGN.md section 11."""
    W = H = 128
    gs, gs2, gc, _ = O.render(oracle_scene, W, H, 1024, 8, error=-1.0, seed=1234)
    truth = O.resolve_float(W, H, gs, gs2, gc)[0]
    f = R.features(oracle_scene, W, H)
    t = T.Temporal(W, H)
    for i in range(4):
        s, s2, c, _ = O.render(oracle_scene, W, H, 16, 8, error=-1.0, seed=42, pass_begin=16 * i)
        out = t.push(s, s2, c, f)
    e = {}
    for tag, (a, a2, n) in (("last", (s, s2, c)), ("merged", (out["sum"], out["sum2"], out["count"]))):
        e[tag + " undenoised"] = _rmse(O.resolve_float(W, H, a, a2, n)[0], truth)
        mean, cout = R.denoise(W, H, a, a2, n, f, levels=5)
        e[tag + " denoised"] = _rmse(pt.tonemap(W, H, mean, cout), truth)
    print(e)
    assert e["merged denoised"] < e["last denoised"]
    assert e["merged undenoised"] < e["last undenoised"]
