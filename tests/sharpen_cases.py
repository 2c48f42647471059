"""The images tests/test_gpu_sharpen.py sends through pt_sharpen_host, the parameter sets, and how two results are compared.
Generated from seeds; the CPU half of the suite (tests/test_sharpen_host.py) checks on the restatement alone that each of them is
changed where it is meant to be."""
import numpy as np

import sharpen_restatement as R

F = np.float32
# (W, H): one pixel; one column and one row (a ring with two of its four outside everywhere); 2 x 2 (every pixel a corner); a 32 x 8
# tile exactly, one more both ways, and several tiles at odd sizes with partial ones at both rims.
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (32, 8), (33, 9), (97, 31)]
# (strength, limit): full and a quarter, the default limit (0 = 0.1875) and a tight one
PARAMS = [(F(1.0), F(0.0)), (F(0.25), F(0.0)), (F(1.0), F(0.05)), (F(0.25), F(0.05))]
EXPOSURES = [F(2.0 ** -8), F(1.0), F(2.0 ** 8)]
BRIGHT = F(40000.0)                                                  # the checkerboard's bright value


def constant(w, h):
    m = np.empty((h, w, 3), F)
    m[:] = np.array([0.5, 0.3, 0.2], F)
    return m, np.ones((h, w), np.int32)


def ramp(w, h):
    """Two plateaux joined by a monotone ramp, along x where the image is wide enough and else along y; the colour is not grey."""
    profile = np.array([.1, .1, .1, .1, .15, .3, .6, .75, .8, .8, .8, .8], F)
    along_x = w >= h
    n = w if along_x else h
    idx = np.clip(np.arange(n) - max(0, (n - len(profile)) // 2), 0, len(profile) - 1)
    line = profile[idx]
    l = np.broadcast_to(line[None, :] if along_x else line[:, None], (h, w))
    m = (l[..., None] * np.array([1.25, 1.0, 0.5], F)).astype(F)
    return m, np.ones((h, w), np.int32)


def hdr(w, h):
    """Random HDR content over ten decades, a tenth of the pixels without samples (and anything in them)."""
    rng = np.random.default_rng(3000 * w + h)
    m = (10.0 ** (rng.uniform(-6, 4, (h, w, 1)) + rng.uniform(-0.3, 0.3, (h, w, 3)))).astype(F)
    c = rng.integers(1, 40, (h, w)).astype(np.int32)
    holes = rng.uniform(size=(h, w)) < 0.1
    c[holes] = 0
    m[holes] = (10.0 ** rng.uniform(-6, 30, (int(holes.sum()), 3))).astype(F)
    return m, c


def hostile(w, h):
    """A smooth field in which every seventh pixel or so is out of play -- a NaN, an infinity, a negative or an over-cap value in a
    pixel that has samples, or a hole holding one -- beside valid ones.  (The cap is on the EXPOSED luminance: 1e12 is beyond it at
    every exposure of the suite.)"""
    rng = np.random.default_rng(4000 * w + h)
    m = np.exp2(rng.uniform(-4, 4, (h, w, 1)) + rng.uniform(-0.5, 0.5, (h, w, 3))).astype(F)
    c = np.ones((h, w), np.int32)
    values = [[np.nan, 1, 1], [1, np.inf, 1], [-9, 0.5, 0.5], [1e12, 1e12, 1e12], [1, 1, -np.inf], [3e38, 3e38, 3e38], [-1e-3, 0, 0]]
    k = 0
    for y in range(h):
        for x in range(w):
            if (3 * x + 5 * y) % 7 == 3:
                m[y, x] = values[k % len(values)]
                c[y, x] = 0 if k % 3 == 2 else 2
                k += 1
    return m, c


def checker(w, h):
    """0 and a bright value: a black pixel's ring is all bright or its own black (mx == 0 at a 1 x 1 image and where the ring is
    substituted), a bright pixel's ring is all black: the guard of hmin, a lobe of -0, and a y' far below 0 that is clamped there.
    In the right half of an image of 8 columns or more the dark squares are 9 and not 0: the ring has headroom, the lobe is at its
    limit, a bright pixel's y' runs beyond Y1 and is clamped there, and a dark one is pulled down."""
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    on = ((xs + ys) % 2 == 1)
    dark = np.where((xs >= w // 2) & (w >= 8) & (ys >= 0), F(9.0), F(0.0)).astype(F)
    m = np.where(on[..., None], np.array([1.0, 0.9, 0.8], F) * BRIGHT, dark[..., None]).astype(F)
    if w * h >= 64:                                                  # ... and a block of 2 x 2 black, whose pixels see black and bright
        m[h // 2:h // 2 + 2, w // 4:w // 4 + 2] = 0
    if w >= 8 and h >= 3:                                            # ... and one dim square among bright ones: its y' < 0 is clamped, its gain 0
        m[1, 1] = F(0.05)
    return m, np.ones((h, w), np.int32)


# name -> (maker, the (W, H) at which the stage is meant to change the image): nowhere; where the ramp's foot fits; wherever a pixel has
# a neighbour; where the dark squares that are not black appear (between 0 and the bright value alone every lobe is 0 or every
# gain 1: there is no headroom, or nothing to scale)
CASES = {"constant": (constant, lambda w, h: False), "ramp": (ramp, lambda w, h: max(w, h) >= 7), "hdr": (hdr, lambda w, h: w * h > 1),
         "hostile": (hostile, lambda w, h: w * h > 1), "checker": (checker, lambda w, h: w >= 8)}


def reference(cache, name, w, h, strength, limit, e):
    """The restatement's output for a case, computed once per (case, shape, parameters, exposure) and session, and read-only."""
    key = (name, w, h, float(strength), float(limit), float(e))
    if key not in cache:
        m, c = CASES[name][0](w, h)
        out = R.sharpen(m, c, e, strength, limit)
        out.setflags(write=False)
        cache[key] = out
    return cache[key]


def compare(got, want, where):
    """Bit for bit; a NaN's payload is free, but only where the restatement says NaN too."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), (where, "a NaN of the restatement is a number on the device")
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())
