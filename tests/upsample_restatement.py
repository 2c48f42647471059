"""Feature-guided upsampling of a frame traced at reduced resolution, restated in numpy float32 from the text of include/pt_hip.h
(pt_upsample_host) -- not from the kernel.  Every operation below is one correctly rounded float operation in the order the header
states, so the device must reproduce these arrays bit for bit.

    resolved_params   the values a pt_upsample_params stands for
    upsample          (mean_rgb [H * W, 3], count_out [H * W]) of a (W / s) x (H / s) mean and the W x H feature buffers
"""
import numpy as np

import denoise_restatement as D

F32 = np.float32
SCALES = (2, 3, 4)
MIN_WEIGHT = F32(1e-4)   # below this total weight a pixel takes the low pixel that contains it


def resolved_params(scale=2, sigma_plane=0.0, normal_power_log2=0, demodulate_albedo=0):
    """Zero fields are the documented defaults, which are the denoiser's."""
    assert scale in SCALES
    return (int(scale), F32(sigma_plane) if sigma_plane > 0 else D.DEFAULT_SIGMA_PLANE,
            int(normal_power_log2) if normal_power_log2 > 0 else D.DEFAULT_NORMAL_POWER_LOG2, demodulate_albedo >= 0)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def upsample(width, height, mean_lo, count_lo, feat, scale=2, sigma_plane=0.0, normal_power_log2=0, demodulate_albedo=0):
    """pt_upsample_host's (mean_rgb, count_out) as the header states them; width x height is the OUTPUT size."""
    s, sig_p, k_n, demod = resolved_params(scale, sigma_plane, normal_power_log2, demodulate_albedo)
    W, H = width, height
    assert W % s == 0 and H % s == 0
    w, h = W // s, H // s
    m = np.ascontiguousarray(mean_lo, np.float32).reshape(h, w, 3)
    data = np.ascontiguousarray(count_lo, np.int32).reshape(h, w) > 0
    P = np.ascontiguousarray(feat["position"], np.float32).reshape(H, W, 3)
    N = np.ascontiguousarray(feat["normal"], np.float32).reshape(H, W, 3)
    A = np.ascontiguousarray(feat["albedo"], np.float32).reshape(H, W, 3)
    hit = np.ascontiguousarray(feat["hit_index"], np.int32).reshape(H, W) >= 0

    def divisor(alb, is_hit):
        if not demod:
            return np.ones_like(alb)
        return np.where(is_hit[..., None], np.where(alb > D.ALBEDO_FLOOR, alb, D.ALBEDO_FLOOR), F32(1)).astype(np.float32)

    # 1. the guide of a low pixel, c = m / a
    Y, X = np.mgrid[0:h, 0:w]
    gy, gx = s * Y + s // 2, s * X + s // 2
    Pg, Ng, hit_g = P[gy, gx], N[gy, gx], hit[gy, gx]
    with np.errstate(all="ignore"):
        c_lo = (m / divisor(A[gy, gx], hit_g)).astype(np.float32)
    # 2. position in the low grid
    ys, xs = np.mgrid[0:H, 0:W]
    fx = (2 * xs + 1 - s).astype(np.float32) / F32(2 * s)
    fy = (2 * ys + 1 - s).astype(np.float32) / F32(2 * s)
    x0f, y0f = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0f).astype(np.float32), (fy - y0f).astype(np.float32)
    X0, Y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    # 3. which taps are used, and their weights
    taps = []
    for j in (0, 1):
        for i in (0, 1):
            Xq, Yq = X0 + i, Y0 + j
            inside = (Xq >= 0) & (Xq < w) & (Yq >= 0) & (Yq < h)
            Xc, Yc = np.clip(Xq, 0, w - 1), np.clip(Yq, 0, h - 1)
            used = inside & data[Yc, Xc] & (hit_g[Yc, Xc] == hit)
            t = ((tx if i else F32(1) - tx) * (ty if j else F32(1) - ty)).astype(np.float32)
            dn = _dot(N, Ng[Yc, Xc])
            wn = np.where(dn > 0, dn, F32(0)).astype(np.float32)
            for _ in range(k_n):
                wn = wn * wn
            with np.errstate(all="ignore"):
                dist = np.abs(_dot(N, Pg[Yc, Xc] - P))
                up = dist / sig_p
                wp = F32(1) / (F32(1) + up * up)
                om = np.where(hit, (t * wn) * wp, t).astype(np.float32)
            taps.append((used, om, c_lo[Yc, Xc]))
    # 4. the heaviest used tap is the base (the first of equals); sums over the used taps in visiting order
    have = np.zeros((H, W), bool)
    best = np.zeros((H, W), np.float32)
    b = np.zeros((H, W, 3), np.float32)
    for used, om, cq in taps:
        with np.errstate(invalid="ignore"):
            take = used & (~have | (om > best))
        have |= used
        best = np.where(take, om, best)
        b = np.where(take[..., None], cq, b)
    Wt = np.zeros((H, W), np.float32)
    S = np.zeros((H, W, 3), np.float32)
    with np.errstate(all="ignore"):
        for used, om, cq in taps:
            Wt = np.where(used, Wt + om, Wt)
            S = np.where(used[..., None], S + om[..., None] * (cq - b), S).astype(np.float32)
        got = Wt > MIN_WEIGHT
        c = b + S / np.where(got, Wt, F32(1))[..., None]
        out = divisor(A, hit) * c
    out = np.where(out > 0, out, F32(0)).astype(np.float32)
    # 5. the fallback: the low pixel that contains p
    R = m[ys // s, xs // s]
    R_data = data[ys // s, xs // s]
    fallback = np.where(R_data[..., None], R, F32(0)).astype(np.float32)
    mean = np.where(got[..., None], out, fallback).astype(np.float32)
    count = np.where(got | R_data, 1, 0).astype(np.int32)
    return mean.reshape(-1, 3), count.reshape(-1)
