"""The inputs of the colour tests (tests/test_colour_host.py, tests/test_gpu_colour.py): images, LUTs and matrices, generated from
seeds, and the prediction of what the display kernel defers.  Every image shape meets every content once and every LUT appears
once; the matrices rotate through the cases."""
import numpy as np

import colour_restatement as R

F = np.float32
SHAPES = [(1, 1), (7, 5), (64, 48), (257, 131)]          # (W, H): one pixel; a tail group; whole groups; partial blocks both ways
CONTENTS = ["ramp", "random", "vertices", "ties", "planted"]
LUT_SIZES = [2, 3, 17, 33, 65]
LUT_KINDS = ["identity", "constant", "swap", "random", "wide"]
CONSTANT = np.array([0.25, 0.5, 0.75], F)
# wb / saturation / user matrix: None = not given
MATRICES = [dict(),
            dict(wb=(1.1, 1.0, 0.9), saturation=0.8),
            dict(wb=(0.9, 1.0, 1.2), saturation=1.3, matrix=[[0.9, 0.1, 0.0], [0.05, 0.9, 0.05], [0.0, 0.2, 0.8]])]
GAMMAS = [F(1) / F(2.2), F(0.5)]
DEFER_CAP = 0.01


def image(content, w, h):
    """mean [h, w, 3] float32, count [h, w] int32."""
    rng = np.random.default_rng(7000 + 31 * w + h + 1000 * CONTENTS.index(content))
    c = np.ones((h, w), np.int32)
    y, x = np.mgrid[0:h, 0:w]
    if content == "ramp":                 # red along x, green along y, through 0 .. 1.5; blue stays low
        m = np.stack([1.5 * x / max(w - 1, 1), 1.5 * y / max(h - 1, 1), 0.2 * (x + y) / max(w + h - 2, 1)], -1).astype(F)
    elif content == "random":
        m = rng.uniform(0.0, 1.2, (h, w, 3)).astype(F)
        c = rng.integers(1, 9, (h, w)).astype(np.int32)
        c[rng.uniform(size=(h, w)) < 0.1] = 0
    elif content == "vertices":           # multiples of 1/64: vertices of N = 65, and of 33, 17, 3 and 2 where the multiple allows
        m = (rng.integers(0, 65, (h, w, 3)) / 64.0).astype(F)
        m[0, 0] = [0.0, 1.0, 0.0]          # g exactly 0 and exactly 1
        m[-1, -1] = [1.0, 1.0, 1.0]
    elif content == "ties":               # two equal channels (each pair) and three; multiples of 1/128 make equal fractions too
        m = rng.uniform(0.0, 1.0, (h, w, 3)).astype(F)
        k = (x + 2 * y) % 5
        m[k == 0, 1] = m[k == 0, 0]
        m[k == 1, 2] = m[k == 1, 1]
        m[k == 2, 2] = m[k == 2, 0]
        m[k == 3] = m[k == 3, :1]
        m[k == 4] = (rng.integers(0, 129, (int((k == 4).sum()), 3)) / 128.0).astype(F)
    else:                                 # "planted": random colours with NaN, negative, +inf channels and pixels without samples
        m = rng.uniform(0.0, 1.2, (h, w, 3)).astype(F)
        c[rng.uniform(size=(h, w)) < 0.15] = 0
        bad = np.array([np.nan, -0.25, np.inf, -0.0, -np.inf, 3.0e38], F)
        n = max(1, (w * h) // 40)
        ys, xs, ks = rng.integers(0, h, n), rng.integers(0, w, n), rng.integers(0, 3, n)
        m[ys, xs, ks] = bad[np.arange(n) % len(bad)]
        c[ys[::2], xs[::2]] = 3           # (half of them certainly have samples)
    return np.ascontiguousarray(m), np.ascontiguousarray(c)


def lut(kind, n):
    """[n, n, n, 3] float32 indexed [b, g, r]."""
    b, g, r = np.meshgrid(*([np.arange(n) / (n - 1)] * 3), indexing="ij")
    ident = np.stack([r, g, b], -1).astype(F)
    rng = np.random.default_rng(100 * n + LUT_KINDS.index(kind))
    if kind == "identity":
        return ident
    if kind == "constant":
        return np.broadcast_to(CONSTANT, (n, n, n, 3)).astype(F).copy()
    if kind == "swap":                    # r <- g, g <- b, b <- r
        return np.ascontiguousarray(ident[..., [1, 2, 0]])
    if kind == "random":
        return rng.uniform(0.0, 1.0, (n, n, n, 3)).astype(F)
    # "wide": entries above 1 everywhere, and a negative vertex in the cyan corner, where neither the ramp nor much of the random
    # content lies: the pixels it pulls below zero are deferred, and stay few
    t = rng.uniform(0.06, 1.3, (n, n, n, 3)).astype(F)
    t[n - 1, n - 1, 0] = [-0.02, 0.4, -0.02]
    return t


def cases():
    """name -> (w, h, content, lut kind or None, N, matrix dict)."""
    out, k = {}, 0
    for n in LUT_SIZES:
        for kind in LUT_KINDS:
            (w, h), content = SHAPES[k % len(SHAPES)], CONTENTS[k % len(CONTENTS)]
            out["%s%d %s %dx%d m%d" % (kind, n, content, w, h, k % 3)] = (w, h, content, kind, n, MATRICES[k % 3])
            k += 1
    for j, content in enumerate(["ramp", "planted", "ties"]):          # the matrix alone
        w, h = SHAPES[3 - j % 2]
        out["matrix %s %dx%d m%d" % (content, w, h, 1 + j % 2)] = (w, h, content, None, 0, MATRICES[1 + j % 2])
    return out


CASES = cases()
PLANTED = {name for name, c in CASES.items() if c[2] == "planted"}


def build(name):
    """-> mean, count, M (float32 [3, 3]), lut array or None, the matrix dict."""
    w, h, content, kind, n, mat = CASES[name]
    m, c = image(content, w, h)
    return m, c, R.compose(**mat), (lut(kind, n) if kind else None), mat


def predict_deferred(out, count, table):
    """How many pixels the display kernel defers for the values `out` [h, w, 3] it searches the table with: a pixel with samples and a
    channel that is negative or NaN, at or above the last threshold, or inside a doubt band (pt_hip.h)."""
    v = np.asarray(out, F).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        bad = ~(v >= 0) | (v >= table["thresholds"][-1])
        for lo, hi in zip(table["doubt_lo"], table["doubt_hi"]):
            if lo != hi:
                bad |= (v >= lo) & (v < hi)
    return int((bad.any(axis=1) & (np.asarray(count).reshape(-1) != 0)).sum())
