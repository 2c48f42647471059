"""Display grading restated in numpy float32 from the text of include/pt_hip.h alone (pt_grade_host, pt_meter_host,
pt_exposure_from_histogram): the grade, the histogram, the exposure rule and its adaptation.  Every operation is one float32
operation in the order the header writes it; the integer parts are Python integers."""
import numpy as np

F = np.float32
REFERENCE, CLAMP, REINHARD, ACES = 0, 1, 2, 3
CURVES = (REFERENCE, CLAMP, REINHARD, ACES)
ENTRIES, DARK, FIRST_INDEX = 129, 128, 444
DEFAULTS = dict(percentile=50, key=F(0.18), e_min=F(2.0 ** -8), e_max=F(2.0 ** 8), rate=F(1.0))


def curve_value(x, curve):
    x = np.asarray(x, F)
    one = F(1)
    with np.errstate(all="ignore"):
        if curve == REFERENCE:
            return x.copy()
        if curve == CLAMP:
            return np.where(x > one, one, x).astype(F)
        if curve == REINHARD:
            return (x / (one + x)).astype(F)
        if curve == ACES:
            a = x * ((F(2.51) * x) + F(0.03))
            b = (x * ((F(2.43) * x) + F(0.59))) + F(0.14)
            g = (a / b).astype(F)
            return np.where(g > one, one, g).astype(F)
    raise ValueError(curve)


def grade(mean, count, exposure, curve):
    """mean [..., 3], count [...]: curve(m * e) where count != 0, the mean's own value elsewhere."""
    m = np.asarray(mean, F)
    with np.errstate(all="ignore"):
        g = curve_value(m * F(exposure), curve)
    return np.where((np.asarray(count) != 0)[..., None], g, m).astype(F)


def luminance(m):
    m = np.asarray(m, F)
    with np.errstate(all="ignore"):
        return ((F(0.2126) * m[..., 0] + F(0.7152) * m[..., 1]) + F(0.0722) * m[..., 2]).astype(F)


def edge(b):
    return np.array([(b + FIRST_INDEX) << 21], np.uint32).view(F)[0]


def histogram(mean, count):
    l = luminance(np.asarray(mean, F).reshape(-1, 3))[np.asarray(count).reshape(-1) != 0]
    with np.errstate(invalid="ignore"):
        lit = l > 0
    hist = np.zeros(ENTRIES, np.uint32)
    hist[DARK] = np.count_nonzero(~lit)
    idx = (l[lit].view(np.uint32) >> 21).astype(np.int64)
    bins = np.clip(idx - FIRST_INDEX, 0, 127)
    hist[:128] = np.bincount(bins, minlength=128)
    return hist


def rule(percentile=0, key=0.0, e_min=0.0, e_max=0.0, rate=0.0):
    """The parameters with the defaults filled in (a zero is the default)."""
    r = dict(DEFAULTS)
    if percentile:
        r["percentile"] = int(percentile)
    for k, v in (("key", key), ("e_min", e_min), ("e_max", e_max), ("rate", rate)):
        if F(v) > 0:
            r[k] = F(v)
    return r


def exposure(hist, r, e_prev=None):
    """(e, e*) of the histogram under rule r; e_prev = None on a first frame."""
    n = sum(int(v) for v in hist[:128])
    if n == 0:
        target = F(e_prev) if e_prev is not None else F(1)
    else:
        cum, bp = 0, 127
        for b in range(128):
            cum += int(hist[b])
            if 100 * cum >= r["percentile"] * n:
                bp = b
                break
        target = F(r["key"] / edge(bp))
        target = r["e_min"] if target < r["e_min"] else (r["e_max"] if target > r["e_max"] else target)
    if e_prev is None or r["rate"] >= F(1):
        return F(target), F(target)
    ep = F(e_prev)
    return F(ep + F(F(target - ep) * r["rate"])), F(target)
