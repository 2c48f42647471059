"""The frame of a MOVING camera (pt_hip.h: camera motion), composed on the host from the CPU oracle's parts (a helper for the
motion tests; tests/view_composition.py does the same for a camera that stands still, and its parts are used here unchanged).

Only the primary ray is restated, from the header's text, in numpy float32 (round to nearest, nothing fused).  With a = start
and b = end as 12 floats (origin, right, up, forward), for pixel (x, y), pass p:

    t       = unit_float(word 0 of Philox counter (pixel, p, 0xFFFFFFFE, 0))          (the same key as every counter)
    delta_j = b_j - a_j;   c_j(t) = a_j + t * delta_j                                  (one product, one sum; j = 0 .. 11)
    u, v, D = (u right + v up) + forward, origin, normalize: as pt_camera states them, with c(t) for the camera
    lens:     r^, u^, f^ of a and of b (in double, rounded once), axis_j(t) = axis^a_j + t * (axis^b_j - axis^a_j), not
              renormalised; then pt_lens's formulas with c(t) and these axes

The words of counter (pixel, p, 0xFFFFFFFF, 0) (jitter, lens) and every segment word are those of the still frame."""
import numpy as np

import oracle_lib as O
import view_composition as V

F32 = np.float32
TIME_COUNTER = 0xFFFFFFFE


def shutter_time(pixel, pass_, seed):
    """t of the paths of `pixel` (global pixel numbers) in pass `pass_`: a multiple of 2^-24 in [2^-24, 1)."""
    return V.unit_float(V.philox(pixel, pass_, TIME_COUNTER, seed)[:, 0])


def interpolate(a, b, t):
    """[n, k]: a_j + t * (b_j - a_j) for flat float32 vectors a, b [k] and times t [n], every operation rounded to float32."""
    a = np.asarray(a, F32).ravel()
    delta = (np.asarray(b, F32).ravel() - a).astype(F32)
    t = np.asarray(t, F32)
    return (a[None, :] + (t[:, None] * delta[None, :]).astype(F32)).astype(F32)


def primary_rays(x, y, width, height, words, t, start, end, lens=None):
    """Origins and unit directions [n, 3] of the primary rays of pixels (x, y) drawn with Philox words [n, 4] at times t [n]."""
    start = np.asarray(start, F32).reshape(4, 3)
    end = np.asarray(end, F32).reshape(4, 3)
    c = interpolate(start, end, t)                      # [n, 12]
    org, right, up, fwd = c[:, 0:3], c[:, 3:6], c[:, 6:9], c[:, 9:12]
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    jx, jy = V.jitter(words[:, 0]), V.jitter(words[:, 1])
    u = ((x + jx) / width - 0.5).astype(F32)
    v = (-(y + jy) / height + 0.5).astype(F32)
    D = (u[:, None] * right + v[:, None] * up) + fwd
    o = org.copy()
    if lens is not None and F32(lens[0]) > 0:
        radius, focus = F32(lens[0]), F32(lens[1])
        ax = interpolate(V.lens_axes(start), V.lens_axes(end), t)   # [n, 9]: r^, u^, f^
        rh, uh, fh = ax[:, 0:3], ax[:, 3:6], ax[:, 6:9]
        rho = radius * np.sqrt(V.unit_float(words[:, 2]))
        sn, cs = V.sincos(F32(2 * F32(3.141593)) * V.unit_float(words[:, 3]))
        pa, pb = rho * cs, rho * sn
        Lp = pa[:, None] * rh + pb[:, None] * uh
        s = focus / ((D[:, 0] * fh[:, 0] + D[:, 1] * fh[:, 1]) + D[:, 2] * fh[:, 2])
        o = o + Lp
        D = D * s[:, None] - Lp
    return o.astype(F32), V.normalize3(D.astype(F32))


def compose(scene, width, height, pixels, spp, mrr, *, start, end, lens=None, seed=42, eps=1e-4, error=-1.0, pass_begin=0):
    """sum [n, 3], sum2 [n, 3], count [n] of the frame's pixels `pixels` ([n, 2] of (x, y)) after passes pass_begin ..
    pass_begin + spp - 1, as the library accumulates them for a camera moving from `start` to `end` (4 x 3 each) with `lens`
    ((radius, focus distance); None = a pinhole).  view_composition.compose's loop, with the interpolated camera."""
    px = np.asarray(pixels, np.int64).reshape(-1, 2)
    n = len(px)
    gpix = (px[:, 1] * width + px[:, 0]).astype(np.uint32)
    s, s2, cnt = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros(n, np.int32)
    for p in range(pass_begin, pass_begin + spp):
        skip = O.adaptive_skip(np.full(n, p, np.int32), s, s2, cnt, error)
        act = np.nonzero(~skip)[0]
        if len(act) == 0:
            continue
        words = V.philox(gpix[act], p, 0xFFFFFFFF, seed)
        t = shutter_time(gpix[act], p, seed)
        o, d = primary_rays(px[act, 0], px[act, 1], width, height, words, t, start, end, lens)
        col = np.ones((len(act), 3), F32)
        depth = np.zeros(len(act), np.int32)
        live = np.arange(len(act))
        while len(live):
            w = V.philox(gpix[act[live]], p, depth[live], seed)[:, :3]
            o2, d2, c2, dep2, contrib, did = scene.segments(o[live], d[live], col[live], depth[live], w, eps=eps, mrr=mrr,
                                                            trig=O.TRIG_PORTABLE)
            o[live], d[live], col[live], depth[live] = o2, d2, c2, dep2
            k = act[live[did]]
            s[k] += contrib[did]
            s2[k] += contrib[did] * contrib[did]
            cnt[k] += 1
            live = live[(dep2 < mrr) & np.any(c2 != 0, axis=1)]
    return s, s2, cnt
