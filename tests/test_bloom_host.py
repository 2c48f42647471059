"""Bloom without a device (include/pt_hip.h: pt_bloom_host, pt_display_present_bloom): the argument checks, which come before the
device is looked at; the struct layout; and exact properties of the numpy restatement of the header's text that do not depend on
reading the header the same way twice -- constants stay constant, flips commute, dim images and empty pixels pass through.  The
host chain restatement -> pt_grade_host -> pt_tonemap -> pt_quantize on an oracle frame; tests/test_gpu_bloom_cli.py compares
pt_render's files with it (pt_render's bloom runs on the device on either path, so that half needs one)."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import bloom_restatement as B

pt = importlib.import_module("path-tracing_amd")
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = 4


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _call(device, w, h, m, c, e, prm, out):
    return pt.lib().pt_bloom_host(device, w, h, None if m is None else pt._fp(m), None if c is None else pt._ip(c), C.c_float(e),
                                  None if prm is None else C.byref(prm), None if out is None else pt._fp(out), None)


BAD_PARAMS = [dict(strength=-0.5), dict(strength=float("nan")), dict(strength=float("inf")), dict(strength=0.5, threshold=-1.0),
              dict(strength=0.5, threshold=float("nan")), dict(strength=0.5, threshold=float("inf")), dict(strength=0.5, levels=-1),
              dict(strength=0.5, levels=9), dict(levels=9), dict(threshold=-1.0)]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=[str(b) for b in BAD_PARAMS])
def test_invalid_parameters_are_refused_before_the_device_is_looked_at(bad):
    m, c, out = np.ones(3, F), np.ones(1, np.int32), np.full(3, 7, F)
    prm = pt._bloom_params(dict(bad))
    assert _call(-1, 1, 1, m, c, 1.0, prm, out) == pt.PT_ERR_INVALID_ARGUMENT
    assert (out == 7).all()
    gp, bgr = pt.GradeParams(), np.full(3, 9, np.uint8)
    rc = pt.lib().pt_display_present_bloom(None, None, None, C.byref(gp), C.byref(prm), bgr.ctypes.data_as(C.POINTER(C.c_uint8)), None, None)
    assert rc == pt.PT_ERR_INVALID_ARGUMENT and (bgr == 9).all()


def test_null_buffers_empty_images_bad_exposures_and_no_device():
    m, c, out = np.ones(3, F), np.ones(1, np.int32), np.full(3, 7, F)
    ok = pt.BloomParams(0.0, 0.5, 0)
    assert _call(-1, 1, 1, None, c, 1.0, ok, out) == pt.PT_ERR_INVALID_ARGUMENT
    assert _call(-1, 1, 1, m, None, 1.0, ok, out) == pt.PT_ERR_INVALID_ARGUMENT
    assert _call(-1, 1, 1, m, c, 1.0, ok, None) == pt.PT_ERR_INVALID_ARGUMENT
    assert _call(-1, 1, 1, m, c, 1.0, None, out) == pt.PT_ERR_INVALID_ARGUMENT
    assert _call(-1, 0, 1, m, c, 1.0, ok, out) == pt.PT_ERR_INVALID_ARGUMENT
    assert _call(-1, 1, 0, m, c, 1.0, ok, out) == pt.PT_ERR_INVALID_ARGUMENT
    assert _call(-1, -3, 1, m, c, 1.0, ok, out) == pt.PT_ERR_INVALID_ARGUMENT
    for e in (0.0, -1.0, float("nan"), float("inf")):                       # 0 is not a default here
        assert _call(-1, 1, 1, m, c, e, ok, out) == pt.PT_ERR_INVALID_ARGUMENT, e
    assert _call(-1, 1, 1, m, c, 1.0, ok, out) == NO_DEVICE                 # everything valid: there is no CPU fallback
    assert _call(-1, 1, 1, m, c, 1.0, pt.BloomParams(), out) == NO_DEVICE   # ... for the copy of strength 0 either
    assert _call(-1, 1, 1, m, c, 1.0, pt.BloomParams(3.0, 2.0, 8), out) == NO_DEVICE
    assert (out == 7).all()


def test_struct_layout_matches_the_header():
    P = pt.BloomParams
    assert C.sizeof(P) == 12 and [k for k, _ in P._fields_] == ["threshold", "strength", "levels"]
    assert [getattr(P, k).offset for k, _ in P._fields_] == [0, 4, 8]
    assert pt.BLOOM_MAX_LEVELS == B.MAX_LEVELS == 8
    header = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    assert "#define PT_BLOOM_MAX_LEVELS 8" in header and "#define PT_ABI_VERSION 5" in header
    assert "float threshold;\n    float strength;\n    int32_t levels;\n} pt_bloom_params;" in header


# ---- exact properties of the restatement ----------------------------------------------------------------------------------

SHAPES = [(1, 1), (2, 3), (9, 33), (19, 67), (48, 64)]          # (H, W)


@pytest.mark.parametrize("levels", [1, 2, 5, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % (w, h) for h, w in SHAPES])
def test_a_constant_image_above_threshold_stays_constant(shape, levels):
    """Every clamp repeats the same value and every weight is dyadic, so each pass of a constant plane is the same few operations
    on one number wherever the pixel lies: the whole pyramid is a scalar recurrence, restated here without a single index."""
    h, w = shape
    m = np.empty((h, w, 3), F)
    m[:] = np.array([3.0, 2.5, 1.75], F)
    c = np.ones((h, w), np.int32)
    for e, T in ((1.0, 1.0), (0.5, 0.25), (4.0, 2.0)):          # t = T / e is a power of two: l - t is exact enough not to matter
        out = B.bloom(m, c, e, T, 0.5, levels)
        assert (_bits(out) == _bits(out[0, 0])).all(), (shape, levels, e)
        assert (out > m).all()                                   # above the threshold something is added
        # ... and exactly what the scalar recurrence gives
        pass4 = lambda v: ((v + v) * F(0.375)) + ((v + v) * F(0.125))
        pass2 = lambda v: (v * F(0.75)) + (v * F(0.25))
        d = [B.bright_pass(m, c, F(e), F(T))[0, 0]]
        for _ in range(levels):
            d.append(pass4(pass4(d[-1])))
        u = d[levels]
        for k in range(levels - 1, 0, -1):
            u = d[k] + pass2(pass2(u))
        a = pass2(pass2(u))
        assert (_bits(out[0, 0]) == _bits(m[0, 0] + (a * F(F(0.5) / F(levels))))).all()


@pytest.mark.parametrize("flip", [1, 0], ids=["left-right", "top-bottom"])
def test_flipping_an_impulse_image_flips_the_output(flip):
    """64 x 64 with L = 3: every level size is even, so the pyramid has no odd column to break the symmetry, and float addition
    commutes -- the mirrored taps give the same bits."""
    rng = np.random.default_rng(5)
    m = np.full((64, 64, 3), 0.25, F)
    for y, x in [(0, 0), (63, 63), (0, 31), (32, 0), (17, 40), (7, 8), (8, 7), (31, 32), (63, 1)]:
        m[y, x] = np.exp2(rng.uniform(1, 8, 3)).astype(F)
    c = np.ones((64, 64), np.int32)
    out = B.bloom(m, c, 1.0, 1.0, 0.7, 3)
    assert (_bits(out) != _bits(m)).any()
    flipped = B.bloom(np.flip(m, flip), c, 1.0, 1.0, 0.7, 3)
    assert (_bits(flipped) == _bits(np.flip(out, flip))).all()


def test_an_image_at_or_below_the_threshold_comes_back_bit_identical():
    rng = np.random.default_rng(6)
    m = np.exp2(rng.uniform(-20, 0, (19, 35, 3))).astype(F)
    m[3, 4] = 0.0
    m[5, 6] = [1.0, 1.0, 1.0]                                    # l = 1 exactly at most: not above t = 1
    m[7, 8] = [1e-45, 1e-40, 0.0]
    c = np.ones((19, 35), np.int32)
    e = F(0.5)
    assert (B.luminance(m) <= F(2.0)).all()
    for levels in (1, 4, 8):
        out = B.bloom(m * F(2), c, e, 1.0, 3.0, levels)           # means up to 2 at e = 1/2: t = 2
        assert (_bits(out) == _bits(m * F(2))).all(), levels


def test_pixels_without_samples_keep_their_value_and_add_nothing():
    rng = np.random.default_rng(8)
    m = np.exp2(rng.uniform(-3, 4, (21, 37, 3))).astype(F)
    c = np.ones((21, 37), np.int32)
    holes = rng.uniform(size=c.shape) < 0.2
    c[holes] = 0
    c[2, 2] = -5                                                 # any count but 0 is "has samples"
    out = B.bloom(m, c, 1.0, 1.0, 0.5, 4)
    assert (_bits(out[holes]) == _bits(m[holes])).all()
    dark = m.copy()
    dark[holes] = 0.0                                            # the same image with the holes black and counted
    other = B.bloom(dark, np.where(holes, 1, c).astype(np.int32), 1.0, 1.0, 0.5, 4)
    assert (_bits(out[~holes]) == _bits(other[~holes])).all()
    bright = m.copy()
    bright[holes] = 1e6                                          # whatever an empty pixel holds, nobody sees it
    again = B.bloom(bright, c, 1.0, 1.0, 0.5, 4)
    assert (_bits(again[~holes]) == _bits(out[~holes])).all()


def test_strength_zero_and_the_defaults():
    m = np.full((5, 7, 3), 4.0, F)
    c = np.ones((5, 7), np.int32)
    assert (_bits(B.bloom(m, c, 1.0, 0.0, 0.0, 0)) == _bits(m)).all()
    assert B.defaults() == (F(1), F(0), 5) and B.defaults(0.5, 2.0, 3) == (F(0.5), F(2), 3)
    assert (_bits(B.bloom(m, c, 1.0, 0.0, 0.5, 0)) == _bits(B.bloom(m, c, 1.0, 1.0, 0.5, 5))).all()


# ---- the host chain on an oracle frame -------------------------------------------------------------------------------------

def host_chain(mean, count, e, curve, gamma, bloom):
    """What pt_render -BLOOM writes for a linear mean and count: restatement -> pt_grade_host -> pt_tonemap -> pt_quantize."""
    h, w, _ = mean.shape
    b = B.bloom(mean, count, e, **bloom)
    g = pt.grade(b, count, e, curve)
    return pt.quantize(pt.tonemap(w, h, g, count.reshape(-1)), count.reshape(h, w))


def test_the_host_chain_on_an_oracle_frame():
    g = np.load(os.path.join(ROOT, "tests", "golden", "tor_frame_64x64x16.npz"))
    s, c = g["sum_bits"].view(F).reshape(64, 64, 3), g["count"].reshape(64, 64).astype(np.int32)
    with np.errstate(all="ignore"):
        mean = np.where((c != 0)[..., None], s / c.astype(F)[..., None], s).astype(F)
    gamma = F(1) / F(2.2)
    e = F(4.0)
    plain = host_chain(mean, c, e, pt.CURVE_CLAMP, gamma, dict(strength=0.0))
    graded = pt.quantize(pt.tonemap(64, 64, pt.grade(mean, c, e, pt.CURVE_CLAMP), c.reshape(-1)), c)
    assert np.array_equal(plain, graded)                          # strength 0: the graded chain's bytes
    lit = B.luminance(mean) > F(1) / e
    assert 0 < np.count_nonzero(lit) < lit.size                   # the frame looks at the light, and not only at it
    bloomed = host_chain(mean, c, e, pt.CURVE_CLAMP, gamma, dict(strength=1.0, levels=4))
    assert (bloomed != graded).any()
    # the frame's means are not negative, so bloom only adds, and under the clamp curve no byte gets darker
    assert (mean[c != 0] >= 0).all() and (bloomed.astype(int) >= graded.astype(int)).all()
    assert (bloomed[c == 0] == graded[c == 0]).all()


# ---- the GPU test's images, on the restatement alone --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["impulses", "field"])
def test_the_gpu_cases_stay_comparable_and_bloom_something(name):
    """tests/test_gpu_bloom.py compares bit patterns except where the restatement says NaN: at least 90 % of every image must be
    left to compare, and the bloom must have changed it."""
    import bloom_cases as K
    for (w, h) in K.SHAPES:
        m, c = K.CASES[name](w, h)
        changed = False
        for levels in K.LEVELS:
            for e, T in K.SETTINGS:
                out = B.bloom(m, c, e, T, K.STRENGTH, levels)
                assert 1.0 - np.isnan(out).any(axis=-1).mean() >= 0.9, (name, w, h, levels, e)
                assert (_bits(out[c == 0]) == _bits(m[c == 0])).all()
                changed |= bool((_bits(out) != _bits(m)).any())
        assert changed, (name, w, h)
    m, c = K.field(257, 129)
    l = B.luminance(m[c != 0])
    assert 0.25 < np.mean(l[np.isfinite(l)] > 1) < 0.45 and np.isnan(m).any() and np.isinf(m).any() and (m < 0).any() and (c == 0).any()
