"""The images tests/test_gpu_local.py sends through pt_local_host, and how two results are compared.  Generated from seeds; the CPU
half of the suite (tests/test_local_host.py) checks on the restatement alone that each of them is changed where it is meant to be."""
import numpy as np

import local_restatement as R

F = np.float32
# (W, H): one pixel, one row, one column; a 32 x 8 tile less one, exactly, and one more, both ways; three tiles across and down with
# a rim; several tiles at odd sizes.  With 8 levels the taps reach 2 * 128 + ... = 510 pixels, beyond every one of them.
SHAPES = [(1, 1), (1, 7), (7, 1)] + [(w, h) for w in (31, 32, 33) for h in (7, 8, 9)] + [(65, 17), (257, 129)]
LEVELS = [1, 2, 3, 5, 8]                                         # both LDS-staged spacings, the first global one, the default, the deepest
EXPOSURES = [F(2.0 ** -3), F(1.0), F(2.0 ** 4)]
SIGMAS = [F(1e-20), F(0.5), F(1e20)]                             # no tap but equal ones; the default; no edge stop at all
STRENGTH, PIVOT = F(1.5), F(0.18)


def constant(w, h):
    m = np.empty((h, w, 3), F)
    m[:] = np.array([0.5, 0.3, 0.2], F)
    return m, np.ones((h, w), np.int32)


def zeros(w, h):
    return np.zeros((h, w, 3), F), np.ones((h, w), np.int32)


def impulses(w, h):
    """Single bright pixels on a dim ground: the corners, the middle of each edge, and either side of every tile seam (multiples of
    32 across and of 8 down) and of the staged regions' rims (2 and 4 pixels beyond a seam)."""
    rng = np.random.default_rng(1000 * w + h)
    m = np.full((h, w, 3), 0.25, F)
    xs = {0, w - 1, w // 2} | {x for x in (27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 63, 64, 127, 128) if x < w}
    ys = {0, h - 1, h // 2} | {y for y in (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 15, 16, 63, 64) if y < h}
    spots = [(y, x) for y in (0, h - 1, h // 2) for x in sorted(xs)] + [(y, x) for y in sorted(ys) for x in (0, w - 1, w // 2)]
    spots += [(y, x) for y in sorted(ys) for x in sorted(xs) if (x + y) % 3 == 0]
    for y, x in spots:
        m[y, x] = np.exp2(rng.uniform(1, 8, 3)).astype(F)
    return m, np.ones((h, w), np.int32)


def _step(ratio, vertical):
    def make(w, h):
        """Two flat halves, the second `ratio` times the first; along x (a vertical edge) or along y."""
        m = np.full((h, w, 3), 0.125, F)
        if vertical:
            m[:, w // 2:] *= F(ratio)
        else:
            m[h // 2:] *= F(ratio)
        return m, np.ones((h, w), np.int32)
    return make


def field(w, h):
    """A random field over 2^-8 .. 2^8; a tenth of the pixels without samples; and, where the image can spare them, pixels with a
    negative, a NaN, an infinite and a nearly overflowing channel, and luminances just below and just above 2^64."""
    rng = np.random.default_rng(2000 * w + h)
    m = np.exp2(rng.uniform(-8, 8, (h, w, 1)) + rng.uniform(-0.5, 0.5, (h, w, 3))).astype(F)
    c = rng.integers(1, 40, (h, w)).astype(np.int32)
    c[rng.uniform(size=(h, w)) < 0.1] = 0
    m[0, 0], c[0, 0] = [5.0, 3.0, 9.0], 2
    if w * h >= 200:
        spots = [(0.1, 0.2), (0.5, 0.5), (0.9, 0.1), (0.3, 0.97), (0.75, 0.6), (0.0, 0.45), (0.6, 0.0), (0.45, 0.3)]
        for k, (fy, fx) in enumerate(spots):
            y, x = int(fy * (h - 1)), int(fx * (w - 1))
            c[y, x] = 3
            m[y, x, k % 3] = [-4.0, np.nan, np.inf, -0.0, 3.0e38, -np.inf, -1e-3, np.nan][k]
        for (fy, fx), scale in (((0.2, 0.7), 0.99), ((0.8, 0.8), 1.01), ((0.55, 0.15), 0.5)):
            y, x = int(fy * (h - 1)), int(fx * (w - 1))
            c[y, x] = 1
            m[y, x] = F(2.0 ** 64) * F(scale)
    return m, c


# name -> (maker, whether the stage is meant to change the image)
CASES = {"constant": (constant, True), "zeros": (zeros, False), "impulses": (impulses, True), "step 2": (_step(2, True), True),
         "step 100": (_step(100, False), True), "step 1e6": (_step(1e6, True), True), "field": (field, True)}


def reference(cache, name, w, h, levels, sigma, e):
    """The restatement's output for a case; the base is computed once per (case, shape, levels, sigma) and session."""
    m, c = CASES[name][0](w, h)
    key = (name, w, h, levels, float(sigma))
    if key not in cache:
        cache[key] = R.base(m, c, levels, sigma)
    b, valid = cache[key]
    return R.apply(m, b, valid, F(e), STRENGTH, PIVOT)


def compare(got, want, where):
    """Bit for bit; a NaN's payload is free, but only where the restatement says NaN too."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), (where, "a NaN of the restatement is a number on the device")
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())
