"""The feature-guided upsampler without a GPU: the two properties the header's choice of base makes exact and the fallback, on the
numpy restatement (tests/upsample_restatement.py); the argument checks of pt_upsample_host, which all come before the device."""
import ctypes as C
import importlib

import numpy as np
import pytest

import upsample_restatement as U

pt = importlib.import_module("path-tracing_amd")
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _features(W, H, hit, normal=(0.0, 0.0, -1.0), position=None, albedo=0.5):
    """Feature buffers of a W x H image: hit [H, W] bool, one normal or [H, W, 3], positions (default: a plane facing the normal)."""
    N = np.broadcast_to(np.asarray(normal, np.float32), (H, W, 3)).copy()
    if position is None:
        y, x = np.mgrid[0:H, 0:W]
        position = np.stack([x * 0.05, y * 0.05, np.full((H, W), 2.0)], -1)
    return {"hit_index": np.where(hit, 5, -1).astype(np.int32).reshape(-1), "position": np.asarray(position, np.float32).reshape(-1, 3),
            "normal": N.reshape(-1, 3), "albedo": np.full((H * W, 3), albedo, np.float32)}


@pytest.mark.parametrize("s", U.SCALES)
def test_a_constant_low_image_comes_back_bit_for_bit(s):
    """Without demodulation: every difference c_Q - b is 0, so b + 0 / Wt = b, whatever the weights are."""
    rng = np.random.default_rng(s)
    w, h = 13, 7
    W, H = s * w, s * h
    hit = rng.random((H, W)) < 0.6                                  # random guides: every mix of classes among a pixel's taps
    N = rng.normal(size=(H, W, 3)).astype(np.float32)
    N = N / np.sqrt((N * N).sum(-1, keepdims=True, dtype=np.float32))   # unit normals: every weight is finite
    P = rng.uniform(-3, 3, (H, W, 3)).astype(np.float32)
    feat = _features(W, H, hit, normal=N, position=P)
    const = np.array([0.7231, 1e-3, 41.5], np.float32)
    mean_lo = np.broadcast_to(const, (w * h, 3)).copy()
    mean, count = U.upsample(W, H, mean_lo, np.full(w * h, 3, np.int32), feat, scale=s, demodulate_albedo=-1)
    assert (count == 1).all()
    assert np.array_equal(_bits(mean), _bits(np.broadcast_to(const, (W * H, 3))))


@pytest.mark.parametrize("s", U.SCALES)
def test_two_perpendicular_planes_keep_their_own_constants(s):
    """A fold at a full-resolution column that is no multiple of s: the low image is constant on each side BY GUIDE, the guide
    normals across the fold are perpendicular to the pixel's (w_n = 0 exactly), so every output pixel gets its own side's constant
    exactly -- the edge stays at output resolution."""
    w, h = 9, 5
    W, H = s * w, s * h
    fold = 4 * s + 1                                                  # not a multiple of s
    assert fold % s != 0
    y, x = np.mgrid[0:H, 0:W]
    left = x < fold
    N = np.where(left[..., None], np.array([0, 0, -1], np.float32), np.array([-1, 0, 0], np.float32)).astype(np.float32)
    # the floor z = 2 on the left, the wall x = fold * 0.05 on the right: each side lies in its own plane
    P = np.where(left[..., None], np.stack([x * 0.05, y * 0.05, np.full((H, W), 2.0)], -1),
                 np.stack([np.full((H, W), fold * 0.05), y * 0.05, 2.0 - (x - fold) * 0.05], -1))
    feat = _features(W, H, np.ones((H, W), bool), normal=N, position=P)
    a, b = np.array([0.25, 0.5, 0.75], np.float32), np.array([3.0, 2.0, 1.0], np.float32)
    Y, X = np.mgrid[0:h, 0:w]
    guide_left = (s * X + s // 2) < fold
    mean_lo = np.where(guide_left[..., None], a, b).astype(np.float32).reshape(-1, 3)
    mean, count = U.upsample(W, H, mean_lo, np.ones(w * h, np.int32), feat, scale=s, demodulate_albedo=-1)
    want = np.where(left[..., None], a, b).astype(np.float32).reshape(-1, 3)
    assert (count == 1).all()
    assert np.array_equal(_bits(mean), _bits(want))
    # the fold cuts the footprint of low column 4, whose guide lies right of it: the footprint's first column still gets the left value
    assert left[0, 4 * s] and not left[0, 4 * s + 1] and not guide_left[0, 4]


def test_a_pixel_without_a_usable_tap_takes_the_low_pixel_that_contains_it():
    s, w, h = 2, 4, 3
    W, H = s * w, s * h
    hit = np.ones((H, W), bool)
    hit[2, 3] = False                                                 # a lone miss pixel: no guide is of its class (guides sit at odd x, y)
    feat = _features(W, H, hit)
    rng = np.random.default_rng(0)
    mean_lo = rng.uniform(0.1, 2, (h * w, 3)).astype(np.float32)
    count_lo = np.ones(h * w, np.int32)
    mean, count = U.upsample(W, H, mean_lo, count_lo, feat, scale=s)
    p = 2 * W + 3
    assert count[p] == 1 and np.array_equal(_bits(mean[p]), _bits(mean_lo[(2 // s) * w + 3 // s]))      # m_R as it is
    # ... and nothing at all where that low pixel has no data either
    count_lo[(2 // s) * w + 3 // s] = 0
    mean, count = U.upsample(W, H, mean_lo, count_lo, feat, scale=s)
    assert count[p] == 0 and not mean[p].any()
    assert count[p + 1] == 1 and count[p - 1] == 1                    # its neighbours are hits and it is nobody's guide
    # no data anywhere: nothing anywhere
    mean, count = U.upsample(W, H, mean_lo, np.zeros(h * w, np.int32), feat, scale=s)
    assert not count.any() and not mean.any()


def test_demodulation_follows_the_full_resolution_albedo():
    """A material boundary inside a low pixel's footprint: constant irradiance, two albedos -- the output shows each pixel's own."""
    s, w, h = 2, 6, 4
    W, H = s * w, s * h
    y, x = np.mgrid[0:H, 0:W]
    alb = np.where((x < 5)[..., None], F(0.8), F(0.2)).astype(np.float32) * np.ones(3, np.float32)
    feat = _features(W, H, np.ones((H, W), bool))
    feat["albedo"] = alb.reshape(-1, 3)
    Y, X = np.mgrid[0:h, 0:w]
    E = F(1.5)                                                        # irradiance; the low mean is albedo(guide) * E
    mean_lo = (alb[s * Y + 1, s * X + 1] * E).astype(np.float32).reshape(-1, 3)
    mean, count = U.upsample(W, H, mean_lo, np.ones(w * h, np.int32), feat, scale=s)
    assert (count == 1).all()
    assert np.allclose(mean.reshape(H, W, 3), alb * E, rtol=1e-6)


def _call(device, W, H, prm, drop=None):
    s = max(prm.scale, 1)
    n, n_lo = max(W * H, 1), max((W // s) * (H // s), 1)
    bufs = {"mean_lo": np.zeros((n_lo, 3), np.float32), "count_lo": np.ones(n_lo, np.int32), "position": np.zeros((n, 3), np.float32),
            "normal": np.zeros((n, 3), np.float32), "albedo": np.zeros((n, 3), np.float32), "hit_index": np.zeros(n, np.int32),
            "mean_rgb": np.zeros((n, 3), np.float32), "count_out": np.zeros(n, np.int32)}
    ptr = lambda k: None if k == drop else (pt._ip if bufs[k].dtype == np.int32 else pt._fp)(bufs[k])
    ms = C.c_float()
    return pt.lib().pt_upsample_host(device, W, H, ptr("mean_lo"), ptr("count_lo"), ptr("position"), ptr("normal"), ptr("albedo"),
                                     ptr("hit_index"), None if drop == "params" else C.byref(prm), ptr("mean_rgb"), ptr("count_out"),
                                     C.byref(ms))


INVALID, NO_DEVICE = 1, 4


def test_invalid_arguments_are_refused_before_the_device_is_looked_at():
    ok = lambda **kw: pt.UpsampleParams(**{"scale": 2, **kw})
    for drop in ("mean_lo", "count_lo", "position", "normal", "albedo", "hit_index", "params", "mean_rgb"):
        assert _call(-1, 8, 4, ok(), drop=drop) == INVALID, drop
    for W, H in ((0, 4), (8, 0), (-2, 4)):
        assert _call(-1, W, H, ok()) == INVALID, (W, H)
    for scale in (-1, 0, 1, 5, 8):
        assert _call(-1, 8 * max(scale, 1), 4 * max(scale, 1), ok(scale=scale)) == INVALID, scale
    for W, H, scale in ((9, 4, 2), (8, 5, 2), (8, 4, 3), (9, 8, 3), (10, 8, 4), (8, 10, 4)):
        assert _call(-1, W, H, ok(scale=scale)) == INVALID, (W, H, scale)
        assert b"multiples" in pt.lib().pt_last_error()
    for bad in (dict(sigma_plane=-0.5), dict(sigma_plane=float("nan")), dict(sigma_plane=float("inf")), dict(normal_power_log2=-1),
                dict(normal_power_log2=17)):
        assert _call(-1, 8, 4, ok(**bad)) == INVALID, bad


@pytest.mark.parametrize("scale", U.SCALES)
def test_a_valid_call_needs_a_device(scale):
    prm = pt.UpsampleParams(scale, 0.0, 0, 0)
    assert _call(-1, 4 * scale, 2 * scale, prm) == NO_DEVICE          # there is no CPU fallback
    assert _call(-1, 4 * scale, 2 * scale, pt.UpsampleParams(scale, 0.3, 16, -1)) == NO_DEVICE
    if pt.device_count() == 0:
        assert _call(0, 4 * scale, 2 * scale, prm) == NO_DEVICE
    assert _call(-1, 4 * scale, 2 * scale, prm, drop="count_out") == NO_DEVICE      # count_out may be NULL


def test_the_binding_knows_the_struct_and_the_limit():
    assert C.sizeof(pt.UpsampleParams) == 16
    hdr = open(pt.os.path.join(pt.os.path.dirname(pt._HERE), "include", "pt_hip.h")).read()
    assert "#define PT_UPSAMPLE_MAX_SCALE %d" % pt.UPSAMPLE_MAX_SCALE in hdr
    assert max(U.SCALES) == pt.UPSAMPLE_MAX_SCALE
    assert {"pt_upsample_host", "pt_display_present_scaled"} <= set(pt.ABI_SYMBOLS)
