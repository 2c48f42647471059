"""First-hit feature buffers and the feature-guided denoiser, restated in numpy float32 from the text of include/pt_hip.h
(pt_render_features_host, pt_denoise_host) -- not from the kernels.  Every operation below is one correctly rounded float
operation in the order the header states, so the device must reproduce these arrays bit for bit.

    centre_rays   the camera ray through every pixel with jitter 0 (view_composition's normalize3 and camera layout)
    features      hit_index / hit_t from the oracle's all-triangles loop, position / normal / albedo from its tables
    denoise       the edge-avoiding a-trous wavelet filter on the linear mean
"""
import numpy as np

import oracle_lib as O
import view_composition as V

F32 = np.float32
LEVELS_MAX = 8
DEFAULT_SIGMA_LUMINANCE = F32(4.0)
DEFAULT_SIGMA_PLANE = F32(0.1)
DEFAULT_NORMAL_POWER_LOG2 = 7
ALBEDO_FLOOR = F32(0.01)
TINY = F32(1e-6)
FILL_MIN_WEIGHT = F32(1e-4)   # a pixel without data takes a value only from taps weighing more than this in all
SPATIAL_BELOW = 4   # pixels with fewer samples also take the spatial variance estimate
LUMA = (F32(0.2126), F32(0.7152), F32(0.0722))
SPLINE = (F32(0.0625), F32(0.25), F32(0.375), F32(0.25), F32(0.0625))   # the B3 spline 1/16, 1/4, 3/8, 1/4, 1/16
PREFILTER = (F32(0.25), F32(0.5), F32(0.25))                            # 3 x 3 variance prefilter, separable weights


def centre_rays(width, height, camera=None, rows=None):
    """Origins and unit directions [n, 3] of the rays through the pixels of rows [r0, r1) with jitter 0, row-major."""
    cam = np.asarray(V.REFERENCE_CAMERA if camera is None else camera, np.float32).reshape(4, 3)
    r0, r1 = rows if rows is not None else (0, height)
    y, x = np.mgrid[r0:r1, 0:width]
    x, y = x.reshape(-1).astype(np.float64), y.reshape(-1).astype(np.float64)
    u = (x / width - 0.5).astype(np.float32)
    v = (-y / height + 0.5).astype(np.float32)
    D = (u[:, None] * cam[1] + v[:, None] * cam[2]) + cam[3]
    o = np.broadcast_to(cam[0], D.shape).copy()
    return o.astype(np.float32), V.normalize3(D.astype(np.float32))


def features(scene, width, height, camera=None, rows=None, eps=1e-4):
    """What pt_render_features_host must return for an oracle_lib.Scene: dict of hit_index [n], hit_t [n], position / normal /
    albedo [n, 3] -- and nan_seen [n] (rays that lie in a triangle's plane, where the library documents a deviation)."""
    o, d = centre_rays(width, height, camera, rows)
    idx, t, nan_seen = scene.closest_hits(o, d, eps=eps)
    tri, tri_mat = scene.triangles()
    mats = scene.materials()
    hit = idx >= 0
    safe = np.where(hit, idx, 0)
    with np.errstate(invalid="ignore"):
        pos = o + d * t[:, None]
    pos = np.where(hit[:, None], pos, F32(0)).astype(np.float32)
    nrm = np.where(hit[:, None], tri[safe, 0:3], F32(0)).astype(np.float32)
    alb = np.where(hit[:, None], mats[tri_mat[safe], 0:3], F32(0)).astype(np.float32)
    return {"hit_index": idx.astype(np.int32), "hit_t": t.astype(np.float32), "position": pos, "normal": nrm, "albedo": alb,
            "nan_seen": nan_seen}


def _luma(c):
    return (LUMA[0] * c[..., 0] + LUMA[1] * c[..., 1]) + LUMA[2] * c[..., 2]


def resolved_params(levels=5, sigma_luminance=0.0, sigma_plane=0.0, normal_power_log2=0, demodulate_albedo=0):
    """The values a pt_denoise_params stands for: zero fields are the documented defaults."""
    return (int(levels), F32(sigma_luminance) if sigma_luminance > 0 else DEFAULT_SIGMA_LUMINANCE,
            F32(sigma_plane) if sigma_plane > 0 else DEFAULT_SIGMA_PLANE,
            int(normal_power_log2) if normal_power_log2 > 0 else DEFAULT_NORMAL_POWER_LOG2, demodulate_albedo >= 0)


def denoise(width, height, s, s2, c, feat, levels=5, sigma_luminance=0.0, sigma_plane=0.0, normal_power_log2=0,
            demodulate_albedo=0):
    """pt_denoise_host's (mean_rgb [H * W, 3], count_out [H * W]) as the header states them."""
    levels, sig_l, sig_p, k_n, demod = resolved_params(levels, sigma_luminance, sigma_plane, normal_power_log2, demodulate_albedo)
    H, W = height, width
    s = np.ascontiguousarray(s, np.float32).reshape(H, W, 3)
    s2 = np.ascontiguousarray(s2, np.float32).reshape(H, W, 3)
    cnt = np.ascontiguousarray(c, np.int32).reshape(H, W)
    sampled = cnt > 0
    n = np.where(sampled, cnt, 1).astype(np.float32)[..., None]
    mean = np.where(sampled[..., None], s / n, s).astype(np.float32)
    if levels == 0:
        return mean.reshape(-1, 3), cnt.reshape(-1).copy()
    P = np.ascontiguousarray(feat["position"], np.float32).reshape(H, W, 3)
    N = np.ascontiguousarray(feat["normal"], np.float32).reshape(H, W, 3)
    A = np.ascontiguousarray(feat["albedo"], np.float32).reshape(H, W, 3)
    hit = np.ascontiguousarray(feat["hit_index"], np.int32).reshape(H, W) >= 0
    # preparation: a = demodulation divisor, c0 = m / a, variance of the mean on luminance (-1: no samples)
    a = np.ones_like(mean)
    if demod:
        a = np.where(hit[..., None], np.where(A > ALBEDO_FLOOR, A, ALBEDO_FLOOR), F32(1)).astype(np.float32)
    c0 = np.where(sampled[..., None], mean / a, F32(0)).astype(np.float32)
    d = s2 / n - mean * mean
    v3 = (np.where(d > 0, d, F32(0)) / n) / (a * a)
    var = np.where(sampled, (LUMA[0] * v3[..., 0] + LUMA[1] * v3[..., 1]) + LUMA[2] * v3[..., 2], F32(-1)).astype(np.float32)
    ys, xs = np.mgrid[0:H, 0:W]

    def tap(dy, dx):
        yy, xx = ys + dy, xs + dx
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        return np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1), inside

    def feature_weight(w, yy, xx):
        """w * w_n * w_p for hit pixels, w for miss pixels"""
        dn = (N[..., 0] * N[yy, xx, 0] + N[..., 1] * N[yy, xx, 1]) + N[..., 2] * N[yy, xx, 2]
        wn = np.where(dn > 0, dn, F32(0)).astype(np.float32)
        for _ in range(k_n):
            wn = wn * wn
        e = P[yy, xx] - P
        dist = np.abs((N[..., 0] * e[..., 0] + N[..., 1] * e[..., 1]) + N[..., 2] * e[..., 2])
        up = dist / sig_p
        wp = F32(1) / (F32(1) + up * up)
        return np.where(hit, (w * wn) * wp, w).astype(np.float32)

    # variance estimate, one 7 x 7 window over the sampled pixels of the centre's class (rows outer, columns inner):
    #   g  = the 3 x 3 binomial mean of the sample variance (inner taps only, weights 1/4 1/2 1/4 squared, renormalised)
    #   sp = the feature-weighted spatial variance of the luminance, max(0, m2 / w - (m1 / w)^2)
    lum = _luma(c0)
    g_acc, g_w = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    m_w, m1, m2 = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            yy, xx, inside = tap(dy, dx)
            use = inside & sampled & (var[yy, xx] >= 0) & (hit[yy, xx] == hit)
            if abs(dy) <= 1 and abs(dx) <= 1:
                w = PREFILTER[dy + 1] * PREFILTER[dx + 1]
                g_acc = np.where(use, g_acc + w * var[yy, xx], g_acc)
                g_w = np.where(use, g_w + w, g_w)
            w = feature_weight(np.ones((H, W), np.float32), yy, xx)
            lq = lum[yy, xx]
            m_w = np.where(use, m_w + w, m_w)
            m1 = np.where(use, m1 + w * lq, m1)
            m2 = np.where(use, m2 + w * (lq * lq), m2)
    safe = np.where(sampled, m_w, F32(1))
    mu = m1 / safe
    sp = m2 / safe - mu * mu
    sp = np.where(sp > 0, sp, F32(0))
    g = g_acc / np.where(sampled, g_w, F32(1))
    est = np.where(cnt >= SPATIAL_BELOW, g, np.where(g > sp, g, sp))
    var = np.where(sampled, est, F32(-1)).astype(np.float32)
    col = c0.copy()
    w_centre = SPLINE[2] * SPLINE[2]
    for level in range(levels):
        step = 1 << level
        have = var >= 0
        lp = _luma(col)
        den = sig_l * np.sqrt(np.where(have, var, F32(0))) + TINY
        sw = np.where(have, w_centre, F32(0)).astype(np.float32)
        sc = np.zeros((H, W, 3), np.float32)
        sv = np.where(have, (w_centre * w_centre) * var, F32(0)).astype(np.float32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if dy == 0 and dx == 0:
                    continue
                yy, xx, inside = tap(dy * step, dx * step)
                cq, vq = col[yy, xx], var[yy, xx]
                use = inside & (vq >= 0) & (hit[yy, xx] == hit)
                w = feature_weight(np.full((H, W), SPLINE[dy + 2] * SPLINE[dx + 2], np.float32), yy, xx)
                t = (lp - _luma(cq)) / den
                w = np.where(have, w * (F32(1) / (F32(1) + t * t)), w).astype(np.float32)
                sw = np.where(use, sw + w, sw)
                sc = np.where(use[..., None], sc + w[..., None] * (cq - col), sc)
                sv = np.where(use, sv + (w * w) * vq, sv)
        got = sw > FILL_MIN_WEIGHT
        safe = np.where(got, sw, F32(1))
        ncol = col + sc / safe[..., None]
        nvar = sv / (safe * safe)
        col = np.where(got[..., None], ncol, col).astype(np.float32)
        var = np.where(got, nvar, var).astype(np.float32)
    filled = var >= 0
    out = np.where(sampled[..., None], mean + a * (col - c0), a * col)
    out = np.where(out > 0, out, F32(0))
    out = np.where(filled[..., None], out, mean).astype(np.float32)
    return out.reshape(-1, 3), np.where(sampled, cnt, np.where(filled, 1, 0)).astype(np.int32).reshape(-1)
