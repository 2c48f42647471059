"""Albedo textures restated in numpy float32 from the text of include/pt_hip.h ("albedo textures": BARYCENTRICS and their per-triangle
record, LOOKUP, the BMP decode), operation by operation: every operation is a float32 operation rounded once, in the order the header writes it, nothing fused;
the divisions are IEEE divisions.  The keyword switches of `uv_at` and `lookup` (swap_b, flip_v, clamp) are the single errors
tests/test_texture_host.py puts on the reference side to show that a frame tells them from the stated lookup."""
import numpy as np

F32 = np.float32
ONE, HALF, ZERO = F32(1.0), F32(0.5), F32(0.0)
NEAREST, BILINEAR = 0, 1


def f32(a):
    return np.ascontiguousarray(a, F32)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def bary_records(tri14):
    """The per-triangle records [n, 8] = a1.xyz, c1, a2.xyz, c2 of the scene's triangle records (plane[4], v0, v1, v2, square);
    den == 0 gives the zero record."""
    t = f32(tri14)
    v0, v1, v2 = t[:, 4:7], t[:, 7:10], t[:, 10:13]
    with np.errstate(all="ignore"):
        e1, e2 = v1 - v0, v2 - v0
        d11, d12, d22 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
        den = d11 * d22 - d12 * d12
        a1 = (e1 * d22[:, None] - e2 * d12[:, None]) / den[:, None]
        a2 = (e2 * d11[:, None] - e1 * d12[:, None]) / den[:, None]
        c1, c2 = -_dot(a1, v0), -_dot(a2, v0)
    rec = np.concatenate([a1, c1[:, None], a2, c2[:, None]], 1).astype(F32)
    rec[den == 0] = 0
    return rec


def barycentrics(rec, p):
    """b1, b2 of points p [n, 3] from their triangles' records rec [n, 8]: ((a.x p.x + a.y p.y) + a.z p.z) + c."""
    rec, p = f32(rec), f32(p)
    with np.errstate(all="ignore"):
        return (_dot(rec[:, 0:3], p) + rec[:, 3]).astype(F32), (_dot(rec[:, 4:7], p) + rec[:, 7]).astype(F32)


def interpolate(uv, b1, b2):
    """(u, v) [n, 2] from corner coordinates uv [n, 3, 2] and the barycentrics."""
    uv, b1, b2 = f32(uv), f32(b1), f32(b2)
    with np.errstate(all="ignore"):
        b0 = (ONE - b1) - b2
        u = (b0 * uv[:, 0, 0] + b1 * uv[:, 1, 0]) + b2 * uv[:, 2, 0]
        v = (b0 * uv[:, 0, 1] + b1 * uv[:, 1, 1]) + b2 * uv[:, 2, 1]
    return np.stack([u, v], 1).astype(F32)


def uv_at(tri14, uv, hit, p, swap_b=False):
    """(u, v) of points p on triangles `hit` of the scene's records tri14 (plane[4], v0, v1, v2, square) with coordinates uv [n_tri, 3, 2]."""
    b1, b2 = barycentrics(bary_records(f32(tri14)[hit]), p)
    if swap_b:
        b1, b2 = b2, b1
    return interpolate(f32(uv).reshape(-1, 3, 2)[hit], b1, b2)


def wrap(x):
    """x - floor(x) where that lies in [0, 1), else 0."""
    x = f32(x)
    with np.errstate(all="ignore"):
        f = x - np.floor(x)
    return np.where((f >= 0) & (f < 1), f, ZERO).astype(F32)


def _axis(f, n, filter):
    """The lower and the upper texel along an axis of n texels and the upper one's weight."""
    x = f * F32(n)
    if filter == NEAREST:
        i = np.minimum(x.astype(np.int64), n - 1)
        return i, i, np.zeros_like(f)
    c = x - HALF
    fl = np.floor(c)
    t = (c - fl).astype(F32)
    i = fl.astype(np.int64)
    return np.where(i < 0, n - 1, i), np.where(i + 1 > n - 1, 0, i + 1), t


def _axis_clamp(x, n, filter):
    """The single error `clamp`: the coordinate clamped into [0, 1] instead of wrapped, the neighbours clamped too."""
    x = np.where(np.isfinite(x), np.clip(x, 0, 1), ZERO).astype(F32) * F32(n)
    if filter == NEAREST:
        i = np.minimum(x.astype(np.int64), n - 1)
        return i, i, np.zeros_like(x)
    c = x - HALF
    fl = np.floor(c)
    i = fl.astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), (c - fl).astype(F32)


def taps(w, h, uv, filter, flip_v=True, clamp=False):
    """Indices (row * w + column, rows top-down) of t00, t10, t01, t11 [n, 4] and the weights tu, tv."""
    uv = f32(uv).reshape(-1, 2)
    if clamp:
        x0, x1, tu = _axis_clamp(uv[:, 0], w, filter)
        y0, y1, tv = _axis_clamp(uv[:, 1], h, filter)
    else:
        x0, x1, tu = _axis(wrap(uv[:, 0]), w, filter)
        y0, y1, tv = _axis(wrap(uv[:, 1]), h, filter)
    r0, r1 = ((h - 1 - y0), (h - 1 - y1)) if flip_v else (y0, y1)
    return np.stack([r0 * w + x0, r0 * w + x1, r1 * w + x0, r1 * w + x1], 1), tu, tv


def _lerp(a, b, t):
    return a + (b - a) * t


def lookup(texels, uv, filter, flip_v=True, clamp=False):
    """The texel [n, 3] of the (h, w, 3) picture at each (u, v)."""
    tex = f32(texels)
    h, w = tex.shape[:2]
    idx, tu, tv = taps(w, h, uv, filter, flip_v, clamp)
    flat = tex.reshape(-1, 3)
    if filter == NEAREST:
        return flat[idx[:, 0]].copy()
    t00, t10, t01, t11 = (flat[idx[:, k]] for k in range(4))
    tu, tv = tu[:, None], tv[:, None]
    return _lerp(_lerp(t00, t10, tu), _lerp(t01, t11, tu), tv).astype(F32)


def decode_table(gamma=2.2):
    """table[b] = (float)pow(b / 255.0, gamma) in double, gamma being the float the entry point takes widened to double; gamma 1: b / 255.0 rounded."""
    b = np.arange(256, dtype=np.float64) / 255.0
    g = float(F32(gamma))
    return (b if g == 1.0 else np.array([float(x) ** g for x in b])).astype(F32)


def lobe_kind(mats10, mat, w0):
    """The lobe the material's step runs for first word w0 (0 emissive, 1 glossy, 2 diffuse, -1 none): Factory's lobe table (Ke alone;
    else glossy with chance Ns / 1000 if Ns != 0 and Ks != 0, then diffuse if 1 - Ns / 1000 > 0) and unit_float(w0) - chance0 > 0."""
    m = f32(mats10)[mat]
    emits = np.any(m[:, 3:6] != 0, axis=1)
    ns = m[:, 9]
    glossy = ~emits & (ns != 0) & np.any(m[:, 6:9] != 0, axis=1)
    diffuse = ~emits & (ONE - ns / F32(1000) > 0)
    unit = (((np.asarray(w0, np.uint32) >> np.uint32(9)) << np.uint32(1)) | np.uint32(1)).astype(F32) * F32(2.0 ** -24)
    second = (unit - ns / F32(1000)) > 0
    kind = np.full(len(m), -1, np.int32)
    kind[diffuse] = 2
    kind[glossy & ~diffuse] = 1
    both = glossy & diffuse
    kind[both] = np.where(second[both], 2, 1)
    kind[emits] = 0
    return kind
