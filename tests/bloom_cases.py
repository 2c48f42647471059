"""The images tests/test_gpu_bloom.py sends through pt_bloom_host, and how two results are compared.  Generated from seeds; the
CPU half of the suite (tests/test_bloom_host.py) checks that the restatement leaves at least 90 % of each of them comparable."""
import numpy as np

import bloom_restatement as B

F = np.float32
SHAPES = [(1, 1), (3, 2), (33, 9), (66, 18), (67, 19), (130, 70), (257, 129)]          # (W, H): see the GPU test's docstring
LEVELS = [1, 2, 5, 8]
SETTINGS = [(F(2.0 ** -3), F(1.0)), (F(1.0), F(0.5)), (F(2.0 ** 4), F(2.0))]           # (exposure, threshold)
STRENGTH = F(0.75)


def impulses(w, h):
    """Single bright pixels on a dim ground: the four corners, the middle of each edge, and either side of every tile seam of the
    first two levels (multiples of 32 and 64 across, 8 and 16 down) and of the 66 x 18 region's rim."""
    rng = np.random.default_rng(1000 * w + h)
    m = np.full((h, w, 3), 0.25, F)
    xs = {0, w - 1, w // 2} | {x for x in (31, 32, 63, 64, 65, 66, 127, 128) if x < w}
    ys = {0, h - 1, h // 2} | {y for y in (7, 8, 15, 16, 17, 18, 31, 32, 63, 64) if y < h}
    spots = [(y, x) for y in (0, h - 1, h // 2) for x in sorted(xs)] + [(y, x) for y in sorted(ys) for x in (0, w - 1, w // 2)]
    spots += [(y, x) for y in sorted(ys) for x in sorted(xs) if (x + y) % 3 == 0]
    for y, x in spots:
        m[y, x] = np.exp2(rng.uniform(1, 8, 3)).astype(F)
    return m, np.ones((h, w), np.int32)


def field(w, h):
    """A random field over 2^-8 .. 2^8, about a third of it above 1; a tenth of the pixels without samples; and, where the image
    is large enough to spare them, a few pixels with a negative, a NaN, an infinite and a nearly overflowing channel."""
    rng = np.random.default_rng(2000 * w + h)
    bright = rng.uniform(size=(h, w, 1)) < 1 / 3
    exponent = np.where(bright, rng.uniform(0, 8, (h, w, 1)), rng.uniform(-8, 0, (h, w, 1))) + rng.uniform(-0.5, 0.5, (h, w, 3))
    m = np.exp2(np.clip(exponent, -8, 8)).astype(F)
    c = rng.integers(1, 40, (h, w)).astype(np.int32)
    c[rng.uniform(size=(h, w)) < 0.1] = 0
    m[0, 0], c[0, 0] = [5.0, 3.0, 9.0], 2              # (the smallest images are lit too)
    if w * h >= 1000:
        for k, (fy, fx) in enumerate([(0.1, 0.2), (0.5, 0.5), (0.9, 0.1), (0.3, 0.97), (0.75, 0.6), (0.0, 0.45), (0.6, 0.0), (0.45, 0.3)]):
            y, x = int(fy * (h - 1)), int(fx * (w - 1))
            c[y, x] = 3
            m[y, x, k % 3] = [-4.0, np.nan, np.inf, -0.0, 3.0e38, -np.inf, -1e-3, np.nan][k]
    return m, c


CASES = {"impulses": impulses, "field": field}


def reference(cache, name, w, h, levels, e, T):
    """The restatement's output for a case, computed once per session."""
    key = (name, w, h, levels, float(e), float(T))
    if key not in cache:
        m, c = CASES[name](w, h)
        cache[key] = B.bloom(m, c, e, T, STRENGTH, levels)
    return cache[key]


def compare(got, want, where):
    """Bit for bit; a NaN's payload is free, but only where the restatement says NaN too.  Returns the comparable fraction."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), (where, "a NaN of the restatement is a number on the device")
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())
    return 1.0 - nan.any(axis=-1).mean()
