"""Sharpening restated in numpy float32 from the text of include/pt_hip.h alone (pt_sharpen_host): the plane of compressed luminance
with its invalid pixels, the ring with its substitution, the lobe, y', the gain and the output.  Every line is one float32 operation
in the order the header writes it; min and max are the header's single comparisons."""
import numpy as np

F = np.float32
MAX_LIMIT = F(0.1875)
MAX_EXPOSED = F(65536.0)
Y1 = F(65536.0 / 65537.0)
L1_MAX = Y1 / (F(1) - Y1)                                            # the largest exposed luminance the stage writes


def defaults(strength=0.0, limit=0.0):
    """The parameters with the default filled in (a zero limit is 0.1875)."""
    return F(strength), F(limit) if F(limit) > 0 else MAX_LIMIT


def fmin(p, q):
    return np.where(q < p, q, p)


def fmax(p, q):
    return np.where(q > p, q, p)


def luminance(m):
    return ((F(0.2126) * m[..., 0]) + (F(0.7152) * m[..., 1])) + (F(0.0722) * m[..., 2])


def compressed_plane(m, count, e):
    """(y [H, W], valid [H, W]); y means nothing where valid is False."""
    with np.errstate(all="ignore"):
        a = luminance(m) * F(e)
        valid = (count != 0) & (a >= 0) & (a <= MAX_EXPOSED)          # a NaN fails both comparisons
        a = np.where(valid, a, F(0)).astype(F)
        return (a / (F(1) + a)).astype(F), valid


def ring(y, valid):
    """b, d, f, h [H, W]: above, left, right, below; the centre's value where that pixel is outside the image or invalid."""
    h, w = y.shape
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    out = []
    for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):
        qy, qx = ys + dy + 0 * xs, xs + dx + 0 * ys
        inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
        qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
        out.append(np.where(inside & valid[qy, qx], y[qy, qx], y).astype(F))
    return out


def sharpened_plane(c, valid, strength, limit):
    """y' [H, W] of the plane c; means nothing where valid is False."""
    b, d, f, h = ring(c, valid)
    with np.errstate(all="ignore"):
        mn = fmin(fmin(b, d), fmin(f, h))
        mx = fmax(fmax(b, d), fmax(f, h))
        hmin = np.where(mx > 0, mn / (F(4) * np.where(mx > 0, mx, F(1))), F(0)).astype(F)
        hmax = (F(1) - mx) / ((F(4) * mn) - F(4))
        lobe = fmax(-hmin, hmax)
        lobe = fmin(lobe, F(0))
        lobe = fmax(lobe, -F(limit))
        lobe = (lobe * F(strength)).astype(F)
        den = F(1) + (F(4) * lobe)
        sd = (((b - c) + (d - c)) + (f - c)) + (h - c)
        y1 = c + ((lobe * sd) / den)
        y1 = np.where(~(y1 >= 0), F(0), np.where(y1 > Y1, Y1, y1))
    return y1.astype(F)


def gain(c, y1):
    """(g, l1) of a pixel's compressed luminance before and after."""
    with np.errstate(all="ignore"):
        l0 = c / (F(1) - c)
        l1 = y1 / (F(1) - y1)
        g = np.where(l0 > 0, l1 / np.where(l0 > 0, l0, F(1)), F(1))
    return g.astype(F), l1.astype(F)


def parts(mean, count, exposure, strength, limit=0.0):
    """(out [H, W, 3], g [H, W], valid [H, W], c [H, W], y' [H, W], l1 [H, W]) of mean [H, W, 3], count [H, W]; strength > 0."""
    m = np.ascontiguousarray(mean, F)
    cnt = np.asarray(count).reshape(m.shape[:2])
    s, lim = defaults(strength, limit)
    c, valid = compressed_plane(m, cnt, F(exposure))
    y1 = sharpened_plane(c, valid, s, lim)
    g, l1 = gain(c, y1)
    with np.errstate(all="ignore"):
        out = (m * g[..., None]).astype(F)
    return np.where(valid[..., None], out, m).astype(F), g, valid, c, y1, l1


def sharpen(mean, count, exposure=1.0, strength=0.0, limit=0.0):
    """out [H, W, 3] of mean [H, W, 3], count [H, W]."""
    if not F(strength) > 0:
        return np.ascontiguousarray(mean, F).copy()
    return parts(mean, count, exposure, strength, limit)[0]
