"""numpy restatement of the lens optics stage, written from the text of include/pt_hip.h ("lens optics"): every operation is one
float32 operation in the header's order, on float32 arrays and float32 scalars only, so numpy rounds each of them once."""
import numpy as np

F = np.float32
LIMITS = {"k1": (-4.0, 4.0), "k2": (-4.0, 4.0), "ca": (-0.25, 0.25), "vignette": (0.0, 64.0)}


def magnifications(ca):
    """mag = (1 - ca, 1, 1 + ca) for r, g, b, each rounded once."""
    ca = F(ca)
    return [F(1) - ca, F(1), F(1) + ca]


def geometry(w, h, k1, k2):
    """cx, cy, px [1, W], py [H, 1], r2 [H, W], f [H, W] of every output pixel."""
    k1, k2 = F(k1), F(k2)
    cx, cy = F(0.5) * F(w - 1), F(0.5) * F(h - 1)
    px = np.arange(w, dtype=F)[None, :] - cx
    py = np.arange(h, dtype=F)[:, None] - cy
    hh = F(0.5) * F(h)
    u, v = px / hh, py / hh
    r2 = (u * u) + (v * v)
    with np.errstate(all="ignore"):
        f = F(1) + (r2 * (k1 + (k2 * r2)))
    return cx, cy, px, py, r2, f


def _clamp(s, hi):
    with np.errstate(all="ignore"):
        return np.where(~(s >= F(0)), F(0), np.where(s > hi, hi, s)).astype(F)


def source(w, h, k1, k2, mag):
    """(sx, sy) [H, W] of one channel: where the output pixel reads, clamped to the image."""
    cx, cy, px, py, _, f = geometry(w, h, k1, k2)
    with np.errstate(all="ignore"):
        s = f * F(mag)
        sx = cx + (px * s)
        sy = cy + (py * s)
    return _clamp(sx, F(w - 1)), _clamp(sy, F(h - 1))


def gain(w, h, k1, k2, vignette):
    """The vignette of every output pixel, [H, W]."""
    r2 = geometry(w, h, k1, k2)[4]
    with np.errstate(all="ignore"):
        q = F(1) + (F(vignette) * r2)
        return F(1) / (q * q)


def resample(plane, count, sx, sy, divide=False):
    """One channel `plane` [H, W] resampled at (sx, sy): (val, kept) -- kept False where the channel is empty."""
    h, w = plane.shape
    x0, y0 = sx.astype(np.int32), sy.astype(np.int32)
    fx, fy = sx - x0.astype(F), sy - y0.astype(F)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    wx0, wy0 = F(1) - fx, F(1) - fy
    ref, sw, sd = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
    kept = np.zeros((h, w), bool)
    for xx, yy, wt in ((x0, y0, wx0 * wy0), (x1, y0, fx * wy0), (x0, y1, wx0 * fy), (x1, y1, fx * fy)):
        n = count[yy, xx]
        keep = (wt != 0) & (n != 0)
        with np.errstate(all="ignore"):
            m = plane[yy, xx]
            if divide:
                m = m / n.astype(F)
            first, later = keep & ~kept, keep & kept
            sw_next = sw + wt
            sd_next = sd + (wt * (m - ref))
        ref = np.where(first, m, ref)
        sw = np.where(first, wt, np.where(later, sw_next, sw))
        sd = np.where(later, sd_next, sd)
        kept |= keep
    with np.errstate(all="ignore"):
        val = ref + (sd / sw)
    return np.where(kept, val, F(0)).astype(F), kept


def optics(mean_rgb, count, k1=0.0, k2=0.0, ca=0.0, vignette=0.0, divide=False):
    """(out [H, W, 3], count_out [H, W]) of the header.  `divide`: mean_rgb holds sums, a tap's mean is sum / float(count)."""
    m = np.ascontiguousarray(mean_rgb, F)
    c = np.ascontiguousarray(count, np.int32).reshape(m.shape[:2])
    h, w, _ = m.shape
    g = gain(w, h, k1, k2, vignette)
    out, full = np.zeros((h, w, 3), F), np.ones((h, w), bool)
    for ch, mag in enumerate(magnifications(ca)):
        sx, sy = source(w, h, k1, k2, mag)
        val, kept = resample(m[:, :, ch], c, sx, sy, divide)
        with np.errstate(all="ignore"):
            out[:, :, ch] = val * g
        full &= kept
    out[~full] = 0
    return out, full.astype(np.int32)
