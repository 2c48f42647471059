"""Film grain and dithered quantization as include/pt_hip.h states them, in numpy float32 / uint32: every line one rounded operation
in the header's order.  The random words are a vectorised Philox4x32-10 (checked against the oracle's generator and Random123's
vectors by tests/test_grain_host.py).  The threshold table is the library's (pt_display_table): it is the host's own pow, searched
once per gamma, and a channel the table does not cover goes through the library's pt_tonemap -> pt_quantize, as the header says."""
import importlib

import numpy as np

pt = importlib.import_module("path-tracing_amd")
F = np.float32
U = np.uint32
KEY1 = 0x50544831            # "PTH1"
DITHER_STREAM, LATTICE_STREAM = 1, 2
TWO_M16 = F(2.0 ** -16)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counters (arrays or scalars, broadcast) under key (k0, k1): four uint32 arrays."""
    c0, c1, c2, c3 = [np.array(np.broadcast_arrays(*[np.asarray(v, np.uint64) for v in (c0, c1, c2, c3)])[i], np.uint64) for i in range(4)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = c0 * np.uint64(0xD2511F53)
        p1 = c2 * np.uint64(0xCD9E8D57)
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c0, c1, c2, c3 = h1 ^ c1 ^ np.uint64(k0), l1, h0 ^ c3 ^ np.uint64(k1), l0
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [c.astype(U) for c in (c0, c1, c2, c3)]


def tri(w):
    w = np.asarray(w, U)
    s = (w & U(0xFFFF)).astype(np.int64) + (w >> U(16)).astype(np.int64) - 65535
    return s.astype(F) * TWO_M16


def defaults(strength=0.0, size=0.0, dither=0.0, seed=0, frame=0):
    return F(strength), F(size) if F(size) != 0 else F(1), F(dither), int(seed) & 0xFFFFFFFF, int(frame) & 0xFFFFFFFF


def lattice(ix, iy, seed, frame):
    return tri(philox(ix, iy, frame, LATTICE_STREAM, seed, KEY1)[0])


def noise(w, h, size, seed, frame):
    """n [h, w] of the header: bilinear over the four lattice values, in difference form."""
    x, y = np.meshgrid(np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64))
    s = F(size)
    fx, fy = x.astype(F) / s, y.astype(F) / s
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    tx, ty = fx - ix.astype(F), fy - iy.astype(F)
    v00, v10 = lattice(ix, iy, seed, frame), lattice(ix + 1, iy, seed, frame)
    v01, v11 = lattice(ix, iy + 1, seed, frame), lattice(ix + 1, iy + 1, seed, frame)
    a = v00 + (tx * (v10 - v00))
    b = v01 + (tx * (v11 - v01))
    return a + (ty * (b - a))


def grained(g, strength=0.0, size=0.0, seed=0, frame=0):
    """g' [h, w, 3] of g [h, w, 3]: channels outside (0, 1) keep their bits."""
    strength, size, _, seed, frame = defaults(strength, size, 0.0, seed, frame)
    g = np.ascontiguousarray(g, F)
    if strength == 0:
        return g.copy()
    h, w, _ = g.shape
    sn = (strength * noise(w, h, size, seed, frame))[..., None]
    with np.errstate(all="ignore"):
        takes = (F(0) < g) & (g < F(1))
        wt = (g * (F(1) - g)) * F(4)
        v = g + (sn * wt)
        v = np.where(v < 0, F(0), np.where(v > 1, F(1), v)).astype(F)
    return np.where(takes, v, g).astype(F)


_tables = {}


def table(gamma):
    """(thresholds, bands [(lo, hi)]) of a gamma, once per session."""
    key = F(gamma).tobytes()
    if key not in _tables:
        t = pt.display_table(F(gamma))
        bands = [(lo, hi) for lo, hi in zip(t["doubt_lo"], t["doubt_hi"]) if lo < hi]
        t["thresholds"].setflags(write=False)
        _tables[key] = (t["thresholds"], bands)
    return _tables[key]


def covered(v, gamma):
    T, bands = table(gamma)
    last = T[-1] if len(T) else F(0)
    with np.errstate(invalid="ignore"):
        ok = (v >= 0) & (v < last)
        for lo, hi in bands:
            ok &= ~((v >= lo) & (v < hi))
    return ok


def levels(v, gamma):
    """k: the number of thresholds <= v (0 for NaN)."""
    T, _ = table(gamma)
    return np.searchsorted(T, np.where(np.isnan(v), F(-1), v), side="right").astype(np.int64)


def fraction(v, k, gamma):
    """f of covered channels: (v - lo) / (hi - lo)."""
    T, _ = table(gamma)
    lo = np.where(k > 0, T[np.maximum(k - 1, 0)], F(0)).astype(F)
    hi = T[np.minimum(k, len(T) - 1)]
    with np.errstate(all="ignore"):
        return ((v - lo) / (hi - lo)).astype(F)


def quantize(g, count, gamma, strength=0.0, size=0.0, dither=0.0, seed=0, frame=0):
    """The bytes [h, w, 3] (B, G, R) of the graded image g [h, w, 3] with count [h, w]."""
    strength, size, dither, seed, frame = defaults(strength, size, dither, seed, frame)
    g = np.ascontiguousarray(g, F)
    h, w, _ = g.shape
    count = np.asarray(count, np.int32).reshape(h, w)
    v = grained(g, strength, size, seed, frame)
    cov = covered(v, gamma)
    k = levels(v, gamma)
    if dither != 0:
        x, y = np.meshgrid(np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64))
        words = np.stack(philox(x, y, frame, DITHER_STREAM, seed, KEY1)[:3], axis=-1)
        f = fraction(v, k, gamma)
        with np.errstate(all="ignore"):
            t = f + (dither * tri(words))
            j = np.where(cov, np.floor(t), 0).astype(np.int64)
        k2 = k + j
        k2 = np.where((k2 < 0) | ((k2 >> 8) != (k >> 8)), k, k2)
        k = np.where(cov, k2, k)
    rgb = (k & 255).astype(np.uint8)
    if not cov.all():                       # the host's own two steps for what the table does not cover
        own = pt.quantize(pt.tonemap(w, h, v, np.ones(h * w, np.int32), gamma), np.ones((h, w), np.int32))[..., ::-1]
        rgb = np.where(cov, rgb, own)
    rgb[count == 0] = 0
    return np.ascontiguousarray(rgb[..., ::-1])
