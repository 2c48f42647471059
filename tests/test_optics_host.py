"""Lens optics without a device (include/pt_hip.h: pt_optics_host, pt_display_present_optics): the argument checks, which come
before the device is looked at; the struct layout; and exact properties of the numpy restatement of the header's text -- the
identity with k1 = k2 = ca = 0, the vignette alone, a constant image, a hole of unsampled pixels, and where a barrel distortion
puts a straight line."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import optics_cases as K
import optics_restatement as R

pt = importlib.import_module("path-tracing_amd")
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = 4


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _call(device, w, h, m, c, prm, out, out_c):
    return pt.lib().pt_optics_host(device, w, h, None if m is None else pt._fp(m), None if c is None else pt._ip(c),
                                   None if prm is None else C.byref(prm), None if out is None else pt._fp(out),
                                   None if out_c is None else pt._ip(out_c), None)


def _present(g, b, l, c, o, out8):
    ref = lambda p: None if p is None else C.byref(p)
    return pt.lib().pt_display_present_optics(None, None, None, ref(g), ref(b), ref(l), ref(c), ref(o), out8, None, None)


def _beyond(v):
    return float(np.nextafter(F(v), F(np.inf) if v > 0 else F(-np.inf)))


# each parameter just outside its range, NaN and both infinities
BAD_PARAMS = [dict(k1=_beyond(4.0)), dict(k1=_beyond(-4.0)), dict(k2=_beyond(4.0)), dict(k2=_beyond(-4.0)), dict(ca=_beyond(0.25)),
              dict(ca=_beyond(-0.25)), dict(vignette=_beyond(64.0)), dict(vignette=-1e-30), dict(vignette=-1.0)]
BAD_PARAMS += [{k: v} for k in ("k1", "k2", "ca", "vignette") for v in (float("nan"), float("inf"), float("-inf"))]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=[str(b) for b in BAD_PARAMS])
def test_invalid_parameters_are_refused_before_the_device_is_looked_at(bad):
    m, c, out, out_c = np.ones(3, F), np.ones(1, np.int32), np.full(3, 7, F), np.full(1, 7, np.int32)
    prm = pt._optics_params(dict(bad))
    assert _call(-1, 1, 1, m, c, prm, out, out_c) == pt.PT_ERR_INVALID_ARGUMENT     # a bad argument with a bad device
    assert "optics" in pt.lib().pt_last_error().decode()
    assert (out == 7).all() and (out_c == 7).all()
    bgr = np.full(3, 9, np.uint8)
    rc = _present(pt.GradeParams(), pt.BloomParams(), pt.LocalParams(), pt.ColourParams(), prm, bgr.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == pt.PT_ERR_INVALID_ARGUMENT and (bgr == 9).all()


def test_the_ends_of_the_ranges_are_valid():
    m, c, out, out_c = np.ones(3, F), np.ones(1, np.int32), np.full(3, 7, F), np.full(1, 7, np.int32)
    for prm in (pt.OpticsParams(4.0, 4.0, 0.25, 64.0), pt.OpticsParams(-4.0, -4.0, -0.25, 0.0), pt.OpticsParams(), pt.OpticsParams(-0.0, 0.0, -0.0, 0.0)):
        assert _call(-1, 1, 1, m, c, prm, out, out_c) == NO_DEVICE      # everything valid: there is no CPU fallback, for the copy either
    assert (out == 7).all() and (out_c == 7).all()


def test_null_buffers_empty_images_aliasing_and_no_device():
    m, c, out, out_c = np.ones(12, F), np.ones(4, np.int32), np.full(12, 7, F), np.full(4, 7, np.int32)
    ok = pt.OpticsParams(-0.1, 0.0, 0.01, 1.0)
    bad = pt.PT_ERR_INVALID_ARGUMENT
    assert _call(-1, 2, 2, None, c, ok, out, out_c) == bad
    assert _call(-1, 2, 2, m, None, ok, out, out_c) == bad
    assert _call(-1, 2, 2, m, c, None, out, out_c) == bad
    assert _call(-1, 2, 2, m, c, ok, None, out_c) == bad
    assert _call(-1, 2, 2, m, c, ok, out, None) == bad
    assert _call(-1, 0, 2, m, c, ok, out, out_c) == bad
    assert _call(-1, 2, 0, m, c, ok, out, out_c) == bad
    assert _call(-1, -3, 2, m, c, ok, out, out_c) == bad
    assert _call(-1, 1 << 16, 1 << 16, m, c, ok, out, out_c) == bad     # too large
    # a gather: no output is an input, whole or in part, with a zeroed struct either
    for prm in (ok, pt.OpticsParams()):
        assert _call(-1, 2, 2, m, c, prm, m, out_c) == bad
        assert _call(-1, 2, 2, m, c, prm, out, c) == bad
        assert _call(-1, 2, 1, m, c, prm, m[3:], out_c) == bad           # overlapping by one pixel
        assert _call(-1, 2, 1, m, c, prm, out, c[1:]) == bad
    assert (m == 1).all() and (c == 1).all() and (out == 7).all() and (out_c == 7).all()
    assert _call(-1, 2, 2, m, c, ok, out, out_c) == NO_DEVICE
    assert _call(pt.device_count(), 2, 2, m, c, ok, out, out_c) == NO_DEVICE
    if pt.device_count() == 0:
        assert _call(0, 2, 2, m, c, ok, out, out_c) == NO_DEVICE
    # the present: every stage's block is required, and checked before the handle is
    g, b, l, col, bgr = pt.GradeParams(), pt.BloomParams(), pt.LocalParams(), pt.ColourParams(), np.zeros(3, np.uint8)
    out8 = bgr.ctypes.data_as(C.POINTER(C.c_uint8))
    for args in ((None, b, l, col, ok), (g, None, l, col, ok), (g, b, None, col, ok), (g, b, l, None, ok), (g, b, l, col, None), (g, b, l, col, ok)):
        assert _present(*args, out8) == bad                              # (the last: a NULL display)


def test_struct_layout_matches_the_header():
    P = pt.OpticsParams
    assert C.sizeof(P) == 16 and [k for k, _ in P._fields_] == ["k1", "k2", "ca", "vignette"]
    assert [getattr(P, k).offset for k, _ in P._fields_] == [0, 4, 8, 12]
    header = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    assert "#define PT_ABI_VERSION 5" in header
    assert "float k1, k2;\n    float ca;\n    float vignette;\n} pt_optics_params;" in header
    assert {"pt_optics_host", "pt_display_present_optics"} <= set(pt.ABI_SYMBOLS)
    assert pt.lib().pt_abi_version() == 5
    with pytest.raises(ValueError):
        pt._optics_params({"k3": 1.0})


# ---- exact properties of the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", K.SHAPES + [(257, 3)], ids=lambda s: "%dx%d" % s)
def test_without_distortion_the_source_is_the_pixel_and_the_resample_the_identity(shape):
    w, h = shape
    sx, sy = R.source(w, h, 0.0, 0.0, F(1))
    assert (sx == np.arange(w, dtype=F)[None, :]).all() and (sy == np.arange(h, dtype=F)[:, None]).all()
    for name in ("field", "hole", "empty", "cross"):
        m, c = K.CASES[name](w, h)
        out, n = R.optics(m, c)
        assert (_bits(out[c != 0]) == _bits(m[c != 0])).all(), name
        assert (n == (c != 0)).all() and (_bits(out[c == 0]) == 0).all(), name    # NaN and +inf in the hole: gone, and nowhere else
    m, c = K.field(w, h)
    sums = m * F(5)
    out, _ = R.optics(sums, np.full_like(c, 5), divide=True)
    assert (_bits(out) == _bits(sums / F(5))).all()


def test_sizes_near_2_to_the_22_still_map_every_pixel_to_itself():
    for w in (2 ** 22 - 1, 2 ** 22 - 2):
        cx = F(0.5) * F(w - 1)
        x = np.arange(w, dtype=F)
        px = x - cx
        assert ((cx + (px * F(1))) == x).all()


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_vignette_alone_is_the_mean_times_the_gain(shape):
    w, h = shape
    m, c = K.hole(w, h)
    for vig in (0.0, 1.5, 64.0):
        out, n = R.optics(m, c, vignette=vig)
        g = R.gain(w, h, 0.0, 0.0, vig)
        want = m * g[:, :, None]
        assert (_bits(out[c != 0]) == _bits(want[c != 0])).all() and (n == (c != 0)).all()
        assert ((g > 0) & (g <= 1)).all()
        if vig == 0.0:
            assert (_bits(g) == _bits(F(1))).all()
    if h > 2:   # darker towards the corners: the gain falls with the radius (2 x 2: every pixel is a corner)
        g = R.gain(w, h, 0.0, 0.0, 1.5)
        assert g[0, 0] < g[h // 2, w // 2] and g[0, 0] == g.min()
        r = np.sqrt(R.geometry(w, h, 0, 0)[4].astype(np.float64))
        cos4 = np.cos(np.arctan(np.sqrt(1.5) * r)) ** 4                 # the natural fall-off the header names
        assert np.abs(g / cos4 - 1).max() < 1e-6


@pytest.mark.parametrize("params", K.PARAMS, ids=str)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "%dx%d" % s)
def test_a_constant_image_stays_constant_to_the_bit(shape, params):
    w, h = shape
    m, c = K.constant(w, h)
    k1, k2, ca, _ = params
    out, n = R.optics(m, c, k1, k2, ca, 0.0)
    assert (n == 1).all() and (_bits(out) == _bits(m)).all()
    # ... over its valid pixels: with a hole in it, every pixel that is left holds the constant
    ys, xs = K.hole_box(w, h)
    c[ys, xs] = 0
    m[ys, xs] = np.nan
    out, n = R.optics(m, c, k1, k2, ca, 0.0)
    assert (_bits(out[n != 0]) == _bits(K.constant(w, h)[0][n != 0])).all() and (_bits(out[n == 0]) == 0).all()


def _exact_taps(w, h, k1, k2, mag):
    """In float64, from the formula: the four taps' columns, rows and whether each has a weight, and which pixels lie within 1e-3 of
    a position where float32 could decide otherwise (a source next to a pixel's column or row)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = 0.5 * (w - 1), 0.5 * (h - 1)
    px, py = x - cx, y - cy
    r2 = (px / (0.5 * h)) ** 2 + (py / (0.5 * h)) ** 2
    s = (1 + r2 * (k1 + k2 * r2)) * mag
    sx, sy = cx + px * s, cy + py * s
    def near(v):                                                        # (exactly on it -- no distortion, or the centre -- is exact in float32 too)
        return (np.abs(v - np.round(v)) < 1e-3) & (v != np.round(v))
    doubt = near(sx) | near(sy)
    sx, sy = np.clip(sx, 0, w - 1), np.clip(sy, 0, h - 1)
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    fx, fy = sx - x0, sy - y0
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    taps = [(x0, y0, (1 - fx) * (1 - fy)), (x1, y0, fx * (1 - fy)), (x0, y1, (1 - fx) * fy), (x1, y1, fx * fy)]
    return taps, doubt, sx, sy


@pytest.mark.parametrize("params", K.PARAMS[:5], ids=str)
@pytest.mark.parametrize("shape", [(33, 9), (64, 64), (97, 31)], ids=lambda s: "%dx%d" % s)
def test_a_hole_empties_a_pixel_only_where_all_taps_of_some_channel_fall_in_it(shape, params):
    w, h = shape
    m, c = K.hole(w, h)
    k1, k2, ca, vig = params
    out, n = R.optics(m, c, k1, k2, ca, vig)
    want_empty, doubt = np.zeros((h, w), bool), np.zeros((h, w), bool)
    for mag in (1 - ca, 1.0, 1 + ca):
        taps, d, _, _ = _exact_taps(w, h, k1, k2, mag)
        doubt |= d
        want_empty |= np.all([(c[yy, xx] == 0) | (wt == 0) for xx, yy, wt in taps], axis=0)
    assert want_empty.any() and want_empty.sum() <= 25 and (~doubt).mean() > 0.9           # the hole's image, a little larger at most
    assert ((n == 0) == want_empty)[~doubt].all()
    assert (_bits(out[n == 0]) == 0).all() and np.isfinite(out).all()                      # neither the NaN nor the +inf leaks
    again = m.copy()
    again[c == 0] = 123.0                                                                 # whatever the hole holds, nobody sees it
    out2, n2 = R.optics(again, c, k1, k2, ca, vig)
    assert (_bits(out2) == _bits(out)).all() and (n2 == n).all()


def test_a_barrel_bows_a_straight_vertical_line_outwards_as_the_formula_predicts():
    w, h, k1, k2 = 97, 65, -0.3, 0.05
    line = 70                                                            # right of the centre column 48
    m = np.zeros((h, w, 3), F)
    m[:, line] = 1.0
    out, n = R.optics(m, np.ones((h, w), np.int32), k1, k2)
    assert (n == 1).all()
    lit = out[:, :, 1] > 0
    # a pixel is lit exactly where its source lies within one pixel of the line (a tap with a weight is the line's)
    taps, doubt, sx, _ = _exact_taps(w, h, k1, k2, 1.0)
    predicted = np.abs(sx - line) < 1
    near = np.abs(np.abs(sx - line) - 1) < 1e-3
    assert (lit == predicted)[~(doubt | near)].all() and predicted.any(axis=1).all()
    # where the line's image lies in a row: the centroid of what is lit against the root of  cx + (x - cx) f(x, y) = line
    cx, cy = 0.5 * (w - 1), 0.5 * (h - 1)
    xs = np.arange(w, dtype=np.float64)
    centroid = (out[:, :, 1].astype(np.float64) * xs).sum(axis=1) / out[:, :, 1].astype(np.float64).sum(axis=1)
    fine = np.linspace(0, w - 1, 20 * (w - 1) + 1)
    for y in range(h):
        r2 = ((fine - cx) / (0.5 * h)) ** 2 + ((y - cy) / (0.5 * h)) ** 2
        root = fine[np.argmin(np.abs(cx + (fine - cx) * (1 + r2 * (k1 + k2 * r2)) - line))]
        assert abs(centroid[y] - root) < 0.75, (y, centroid[y], root)
    # barrel: f < 1 away from the centre, the source lies nearer the centre than the pixel, so the line's image lies further out --
    # and the more so the further the row is from the middle one: the line bows outwards
    assert centroid[h // 2] > line + 1 and centroid[0] > centroid[h // 4] > centroid[h // 2] and centroid[-1] > centroid[-1 - h // 4] > centroid[h // 2]
    # the pincushion of the cases does the opposite
    out, _ = R.optics(m, np.ones((h, w), np.int32), 0.25, 0.0)
    centroid = (out[:, :, 1].astype(np.float64) * xs).sum(axis=1) / out[:, :, 1].astype(np.float64).sum(axis=1)
    assert centroid[h // 2] < line and centroid[0] < centroid[h // 4] < centroid[h // 2]


def test_chromatic_aberration_moves_red_and_blue_apart_and_leaves_green():
    w, h = 97, 31
    m, c = K.cross(w, h)
    out, n = R.optics(m, c, ca=0.02)
    assert (n == 1).all()
    assert (_bits(out[:, :, 1]) == _bits(m[:, :, 1])).all()              # mag_g = 1: the identity
    xs = np.arange(w, dtype=np.float64)
    row = 3                                                              # away from the horizontal bar

    def column_of_the_bar(ch, lo, hi):
        v = out[row, lo:hi, ch].astype(np.float64) - 0.0625
        return (v * xs[lo:hi]).sum() / v.sum()
    # red reads nearer the centre (1 - ca): what it shows lies further out; blue the other way -- no fringe at the centre column
    assert abs(column_of_the_bar(0, 40, 57) - 48) < 1e-6 and abs(column_of_the_bar(2, 40, 57) - 48) < 1e-6
    m2 = np.full((h, w, 3), 0.0625, F)
    m2[:, 90] = 9.0
    out, _ = R.optics(m2, c, ca=0.02)
    red, blue = column_of_the_bar(0, 80, 97), column_of_the_bar(2, 80, 97)
    assert red > 90.5 and blue < 89.5 and abs(red - (48 + 42 / 0.98)) < 0.1 and abs(blue - (48 + 42 / 1.02)) < 0.1


# ---- the GPU test's images, on the restatement alone --------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(K.CASES))
def test_the_gpu_cases_are_changed_where_they_are_meant_to_be(name):
    for (w, h) in K.SHAPES:
        m, c = K.CASES[name](w, h)
        for params in K.PARAMS:
            out, n = K.reference(name, w, h, params)
            assert out.shape == m.shape and n.shape == c.shape and set(np.unique(n)) <= {0, 1}
            assert np.isfinite(out).all(), (name, w, h, params)          # the hole's NaN and +inf never leak
            assert (_bits(out[n == 0]) == 0).all()
            if name == "empty":
                assert (n == 0).all()
            elif name != "hole":
                assert (n == 1).all()
            if name == "field" and w > 2 and h > 2 and params[3] == 0.0:
                assert (_bits(out) != _bits(m)).any(), (name, w, h, params)
            if name == "constant" and params[3] == 0.0:
                assert (_bits(out) == _bits(m)).all()
    # at the extremes f is negative or huge: at r >= 1, half the height (15.5 pixels) from the centre, |f| = |1 +- 4 r2 (1 + r2)| >= 7
    # and |s| >= 0.75 * 7; such a pixel has |px| >= 10 or |py| >= 11, and 5.25 times that is beyond 48 or 15: a coordinate is clamped
    for params in K.PARAMS[5:]:
        sx, sy = R.source(97, 31, params[0], params[1], R.magnifications(params[2])[0])
        r2 = R.geometry(97, 31, 0, 0)[4]
        assert (((sx == 0) | (sx == 96)) | ((sy == 0) | (sy == 30)))[r2 >= 1].all() and (r2 >= 1).mean() > 0.6
        assert {(float(sx[y, x]), float(sy[y, x])) for y in (0, 30) for x in (0, 96)} == {(0.0, 0.0), (96.0, 0.0), (0.0, 30.0), (96.0, 30.0)}
        f = R.geometry(97, 31, params[0], params[1])[5]
        assert (f[0, 0] < 0) == (params[0] < 0) and abs(f[0, 0]) > 100
