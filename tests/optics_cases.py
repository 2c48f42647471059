"""The images tests/test_gpu_optics.py sends through pt_optics_host, the parameter sets, and how two results are compared.
Generated from seeds; tests/test_optics_host.py checks on the restatement alone that each of them is changed where it is meant to be."""
import numpy as np

import optics_restatement as R

F = np.float32
# (W, H): one pixel, one column, one row (cx or cy degenerate, every x1 or y1 clamped); the smallest with four distinct taps; one
# column past a 32 x 8 workgroup; whole workgroups; partial workgroups both ways.
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (33, 9), (64, 64), (97, 31)]
# (k1, k2, ca, vignette): barrel with a k2 term, pincushion, chromatic aberration alone, vignette alone, all together; and the
# extremes of the valid ranges, where f goes negative or huge and every source lands on the clamp.
PARAMS = [(-0.3, 0.05, 0.0, 0.0), (0.25, 0.0, 0.0, 0.0), (0.0, 0.0, 0.02, 0.0), (0.0, 0.0, 0.0, 1.5), (-0.3, 0.05, 0.02, 1.5),
          (4.0, 4.0, 0.25, 64.0), (-4.0, -4.0, -0.25, 0.0)]


def field(w, h):
    """A seeded random positive field over 2^-4 .. 2^4."""
    rng = np.random.default_rng(3000 * w + h)
    m = np.exp2(rng.uniform(-4, 4, (h, w, 1)) + rng.uniform(-0.5, 0.5, (h, w, 3))).astype(F)
    return m, np.ones((h, w), np.int32)


def hole_box(w, h):
    """Rows and columns of the 3 x 3 hole about the centre, cut to the image."""
    y, x = h // 2, w // 2
    return slice(max(y - 1, 0), min(y + 2, h)), slice(max(x - 1, 0), min(x + 2, w))


def hole(w, h):
    """The field with a 3 x 3 hole of count == 0 about the centre that carries NaN and +inf in its rgb."""
    m, c = field(w, h)
    ys, xs = hole_box(w, h)
    c[ys, xs] = 0
    m[ys, xs] = np.array([np.nan, np.inf, np.nan], F)
    return m, c


def empty(w, h):
    """No pixel has a sample; the rgb holds the field and a NaN."""
    m, c = field(w, h)
    m[0, 0, 1] = np.nan
    return m, np.zeros_like(c)


def constant(w, h):
    m = np.empty((h, w, 3), F)
    m[:] = np.array([0.3, 0.7, 0.1], F)          # (no power of two: w * c rounds)
    return m, np.ones((h, w), np.int32)


def cross(w, h):
    """A one-pixel-wide bright cross through the centre on a dim ground."""
    m = np.full((h, w, 3), 0.0625, F)
    m[h // 2, :] = np.array([9.0, 7.0, 5.0], F)
    m[:, w // 2] = np.array([9.0, 7.0, 5.0], F)
    return m, np.ones((h, w), np.int32)


CASES = {"field": field, "hole": hole, "empty": empty, "constant": constant, "cross": cross}
_cache = {}


def reference(name, w, h, params):
    """The restatement's (out, count_out) for a case, computed once per session and never written to."""
    key = (name, w, h, tuple(params))
    if key not in _cache:
        m, c = CASES[name](w, h)
        out, n = R.optics(m, c, *params)
        out.setflags(write=False)
        n.setflags(write=False)
        _cache[key] = (out, n)
    return _cache[key]


def compare(got, want, where):
    """Bit for bit; a NaN's payload is free, but only where the restatement says NaN too."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), (where, "a NaN of the restatement is a number on the device")
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())
