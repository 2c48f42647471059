"""Bloom restated in numpy float32 from the text of include/pt_hip.h alone (pt_bloom_host): the bright pass, the (1 3 3 1)/8
pyramid down, the (1 3)/4 pyramid up and the output.  Every line is one float32 operation in the order the header writes it;
indices are integers, clamped as c(i, n) = min(max(i, 0), n - 1)."""
import numpy as np

F = np.float32
MAX_LEVELS = 8
FLT_MAX = np.finfo(F).max


def c(i, n):
    return np.minimum(np.maximum(i, 0), n - 1)


def defaults(threshold=0.0, strength=0.0, levels=0):
    """The parameters with the defaults filled in (a zero threshold is 1, zero levels are 5)."""
    return F(threshold) if F(threshold) > 0 else F(1), F(strength), int(levels) if levels else 5


def luminance(m):
    return ((F(0.2126) * m[..., 0]) + (F(0.7152) * m[..., 1])) + (F(0.0722) * m[..., 2])


def bright_pass(m, count, e, T):
    """B [H, W, 3]."""
    t = F(T) / F(e)
    l = luminance(m)
    lit = (count != 0) & (l > t) & (l <= FLT_MAX)            # a NaN fails both comparisons
    s = ((l - t) / l).astype(F)
    return np.where(lit[..., None], m * s[..., None], F(0)).astype(F)


def _taps4(p, idx, axis, n):
    """((p_0 + p_1) * 0.375) + ((p_-1 + p_2) * 0.125) at the decimated positions idx along `axis` of length n."""
    t = lambda j: np.take(p, c(2 * idx + j, n), axis=axis)
    return ((t(0) + t(1)) * F(0.375)) + ((t(-1) + t(2)) * F(0.125))


def down(d):
    """D_k [h_k, w_k, 3] of D_{k-1} [h, w, 3]: horizontal at the decimated columns, then vertical on G."""
    h, w, _ = d.shape
    g = _taps4(d, np.arange((w + 1) >> 1), 1, w)
    return _taps4(g, np.arange((h + 1) >> 1), 0, h).astype(F)


def _taps2(u, n_out, axis):
    n = u.shape[axis]
    x = np.arange(n_out)
    X = x >> 1
    shape = [1, 1, 1]
    shape[axis] = n_out
    even = ((x & 1) == 0).reshape(shape)
    at = lambda i: np.take(u, c(i, n), axis=axis)
    g_even = (at(X - 1) * F(0.25)) + (at(X) * F(0.75))
    g_odd = (at(X) * F(0.75)) + (at(X + 1) * F(0.25))
    return np.where(even, g_even, g_odd).astype(F)


def up2(u, h, w):
    """V [h, w, 3] of U_{k+1}: horizontal first, then the same rule vertically on g."""
    return _taps2(_taps2(u, w, 1), h, 0)


def glare(m, count, e, T, L):
    """A [H, W, 3]."""
    d = [bright_pass(m, count, e, T)]
    for _ in range(L):
        d.append(down(d[-1]))
    u = d[L]
    for k in range(L - 1, 0, -1):
        u = (d[k] + up2(u, d[k].shape[0], d[k].shape[1])).astype(F)
    return up2(u, d[0].shape[0], d[0].shape[1])


def bloom(mean, count, exposure=1.0, threshold=0.0, strength=0.0, levels=0):
    """out [H, W, 3] of mean [H, W, 3], count [H, W]."""
    m = np.ascontiguousarray(mean, F)
    cnt = np.asarray(count).reshape(m.shape[:2])
    T, S, L = defaults(threshold, strength, levels)
    if not S > 0:
        return m.copy()
    with np.errstate(all="ignore"):
        wgt = F(S / F(L))
        a = glare(m, cnt, F(exposure), T, L)
        out = (m + (a * wgt)).astype(F)
    return np.where((cnt != 0)[..., None], out, m).astype(F)
