"""Local exposure restated in numpy float32 from the text of include/pt_hip.h alone (pt_local_host): the luminance plane with its
invalid pixels, L edge-stopped levels of the 5 x 5 B3 spline at tap spacing 2^k, the gain and the output.  Every line is one
float32 operation in the order the header writes it; a skipped tap leaves both sums as they were."""
import numpy as np

F = np.float32
MAX_LEVELS = 8
MAX_LUMINANCE = F(2.0 ** 64)
H5 = [F(1 / 16), F(4 / 16), F(6 / 16), F(4 / 16), F(1 / 16)]      # h_-2 .. h_2


def defaults(strength=0.0, pivot=0.0, levels=0, sigma=0.0):
    """The parameters with the defaults filled in (a zero pivot is 0.18, zero levels are 5, a zero sigma is 0.5)."""
    return F(strength), F(pivot) if F(pivot) > 0 else F(0.18), int(levels) if levels else 5, F(sigma) if F(sigma) > 0 else F(0.5)


def luminance(m):
    return ((F(0.2126) * m[..., 0]) + (F(0.7152) * m[..., 1])) + (F(0.0722) * m[..., 2])


def luminance_plane(m, count):
    """(b_0 [H, W], valid [H, W]); b_0 means nothing where valid is False."""
    with np.errstate(all="ignore"):
        l = luminance(m)
        valid = (count != 0) & (l >= 0) & (l <= MAX_LUMINANCE)       # a NaN fails both comparisons
    return np.where(valid, l, F(0)).astype(F), valid


def level(b, valid, k, sigma):
    """b_{k+1} [H, W] of b_k: 25 taps in row-major order, dy then dx, at spacing 2^k."""
    h, w = b.shape
    step = 1 << k
    sw, sd = np.zeros((h, w), F), np.zeros((h, w), F)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            qy, qx = ys + dy * step, xs + dx * step
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            bq = b[qy, qx]
            taken = valid & inside & valid[qy, qx]
            d = bq - b
            mn = np.where(bq < b, bq, b)
            s = (sigma * mn) + F(1e-30)
            r = d / s
            wr = F(1) / (F(1) + (r * r))
            wt = (H5[dy + 2] * H5[dx + 2]) * wr
            sw = np.where(taken, sw + wt, sw)
            sd = np.where(taken, sd + (wt * d), sd)
    return np.where(valid, b + (sd / np.where(valid, sw, F(1))), b).astype(F)


def base(m, count, levels, sigma):
    """(b_L [H, W], valid [H, W])."""
    b, valid = luminance_plane(m, count)
    with np.errstate(all="ignore"):
        for k in range(levels):
            b = level(b, valid, k, F(sigma))
    return b, valid


def gain(b, e, c, pivot):
    """g of a base b: scalars or arrays."""
    with np.errstate(all="ignore"):
        a = F(b) * F(e)
        return (F(1) + F(c)) / (F(1) + ((F(c) * a) / F(pivot)))


def apply(m, b, valid, e, c, pivot):
    """out [H, W, 3]: m * g where valid, m elsewhere."""
    with np.errstate(all="ignore"):
        g = gain(b, e, c, pivot).astype(F)
        out = (m * g[..., None]).astype(F)
    return np.where(valid[..., None], out, m).astype(F)


def local_exposure(mean, count, exposure=1.0, strength=0.0, pivot=0.0, levels=0, sigma=0.0):
    """out [H, W, 3] of mean [H, W, 3], count [H, W]."""
    m = np.ascontiguousarray(mean, F)
    cnt = np.asarray(count).reshape(m.shape[:2])
    c, pv, L, sg = defaults(strength, pivot, levels, sigma)
    if not c > 0:
        return m.copy()
    b, valid = base(m, cnt, L, sg)
    return apply(m, b, valid, F(exposure), c, pv)
