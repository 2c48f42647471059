"""The images the grain tests quantize, their shapes and parameter sets, shared by tests/test_grain_host.py (pt_grain_quantize) and
tests/test_gpu_grain.py (pt_display_bytes_grain_host).  A case is a plane of VALUES: the host test reads it as the graded image g, the
GPU test as a mean image that the colour step turns into g.  Every case is made from the shape and the gamma's table alone.
No gamma the suite uses has a doubt band on this library's pow (pt_display_table says so; tests/test_grain_host.py asserts it), so
there is no case inside one; the restatement and both implementations handle a band as the header says."""
import numpy as np

import grain_restatement as R

F = np.float32
GAMMA = F(1) / F(2.2)
# (W, H): one pixel; a tail alone; widths that are no multiple of 4, so that a lane's four pixels straddle a row end (97 x 31 leaves a
# tail of 3 and fills more than one wave); an odd square; a width that is a multiple of 4
SHAPES = [(1, 1), (3, 1), (5, 3), (97, 31), (17, 15), (64, 4)]
SIZES = [1.0, 1.5, 2.0, 3.7, 8.0]
FRAMES = [0, 1, 2 ** 32 - 1]


def _plane(w, h, values):
    """Values [n] or [n, 3] repeated over a w x h plane, pixel by pixel."""
    values = np.asarray(values, F)
    if values.ndim == 1:
        values = np.repeat(values[:, None], 3, axis=1)
    idx = np.arange(w * h) % len(values)
    return np.ascontiguousarray(values[idx].reshape(h, w, 3)), np.ones((h, w), np.int32)


def grey(w, h):
    return _plane(w, h, [0.5])


def ramp(w, h):
    """A ramp across three levels in the mid-tones, along the flat plane; the channels a third of a level apart."""
    T, _ = R.table(GAMMA)
    t = np.linspace(0.0, 1.0, max(w * h, 2))[:w * h]
    v = (T[120] + (T[123] - T[120]) * t).astype(F)
    d = (T[121] - T[120]) / F(3)
    return _plane(w, h, np.stack([v, v + d, v + 2 * d], axis=1))


def thresholds(w, h):
    """Values exactly at a threshold and one ulp below it, at the table's foot, round the wrap and at its top."""
    T, _ = R.table(GAMMA)
    ks = np.array([0, 1, 2, 100, 253, 254, 255, 256, 348, 349, 510, 511, 4094], np.int64)   # (threshold k + 1 of the header)
    at = T[ks]
    below = (at.view(np.uint32) - np.uint32(1)).view(F)
    values = np.stack([at, below], axis=1).reshape(-1)
    return _plane(w, h, np.stack([values, np.roll(values, 1), np.roll(values, 2)], axis=1))


def named(w, h):
    """0, 1 and 2 (level 349 on the reference curve: the wrap), -0 and a denormal."""
    return _plane(w, h, [[0.0, 1.0, 2.0], [1.0, 2.0, 0.0], [2.0, 0.0, 1.0], [-0.0, 1e-40, 0.5], [0.25, 0.75, 1.0]])


def hostile(w, h):
    """Negative, NaN and infinite pixels beside valid ones: every third pixel is out of play in one channel."""
    rng = np.random.default_rng(5000 * w + h)
    m = rng.uniform(0.0, 1.0, (h, w, 3)).astype(F)
    bad = np.array([np.nan, -1.0, np.inf, -np.inf, -1e-30, 3e38], F)
    flat = m.reshape(-1, 3)
    for p in range(0, w * h, 3):
        flat[p, p % 3] = bad[(p // 3) % len(bad)]
    return m, np.ones((h, w), np.int32)


def holes(w, h):
    """A smooth field with a fifth of its pixels without samples, and anything in them."""
    rng = np.random.default_rng(6000 * w + h)
    m = rng.uniform(0.0, 1.0, (h, w, 3)).astype(F)
    c = rng.integers(1, 9, (h, w)).astype(np.int32)
    gone = rng.uniform(size=(h, w)) < 0.2
    if w * h > 1:
        gone.reshape(-1)[-1] = False
    c[gone] = 0
    m[gone] = np.array([np.nan, 1e30, -5.0], F)
    return m, c


def top(w, h):
    """Values at and above the last threshold, beside values just below it and mid-tones."""
    T, _ = R.table(GAMMA)
    last = T[-1]
    return _plane(w, h, [[last, 0.5, 0.5], [0.5, np.nextafter(last, F(np.inf)), 0.5], [np.nextafter(last, F(0)), 0.5, 2 * last], [0.5, 0.5, 0.5],
                         [T[-2], np.nextafter(T[-2], F(0)), 0.3]])


CASES = {"grey": grey, "ramp": ramp, "thresholds": thresholds, "named": named, "hostile": hostile, "holes": holes, "top": top}


def reference(cache, g, count, gamma, **prm):
    """The restatement's bytes, computed once per distinct (image, parameters) and session, and read-only."""
    key = (g.tobytes(), count.tobytes(), F(gamma).tobytes(), tuple(sorted(prm.items())))
    if key not in cache:
        out = R.quantize(g, count, gamma, **prm)
        out.setflags(write=False)
        cache[key] = out
    return cache[key]


def same(got, want, where):
    bad = got != want
    assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())
