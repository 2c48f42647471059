"""The frame of a camera under any PROJECTION (pt_hip.h: pt_projection), composed on the host from the CPU oracle's parts (a helper
for the projection tests; tests/view_composition.py does the same for the pinhole and the thin lens, and its parts are used here
unchanged, by import).

Only the primary ray is restated, from the header's text, in numpy float32 (round to nearest, nothing fused).  With o, r, p, f the
camera's origin, right, up, forward and r^, u^, f^ = r / |r|, p / |p|, f / |f| (in double, rounded to float once):

    u = float((x + jx) / W - 0.5),  v = float(-(y + jy) / H + 0.5)                  (in double, then rounded)
    perspective      D = (u r + v p) + f,  origin o                                 (view_composition.primary_rays itself)
    orthographic     origin_i = o_i + (u r_i + v p_i),  D = f
    fisheye          a = u span_x,  b = v span_y,  theta = sqrt(a a + b b),  (sn, cs) = sincos(theta),
                     k = theta == 0 ? 1 : sn / theta,  D_i = ((k a) r^_i + (k b) u^_i) + cs f^_i,  origin o
    equirectangular  phi = u span_x,  psi = v span_y,  (s, c) = sincos(|angle|) with the angle's sign bit put back on s,
                     D_i = ((c_psi s_phi) r^_i + s_psi u^_i) + (c_psi c_phi) f^_i,  origin o
    direction = normalize3(D)

The words of counter (pixel, p, 0xFFFFFFFF, 0) (the jitter) and every segment word are those of the pinhole's frame."""
import numpy as np

import oracle_lib as O
import view_composition as V

F32 = np.float32
PERSPECTIVE, ORTHOGRAPHIC, FISHEYE, EQUIRECTANGULAR = 0, 1, 2, 3


def image_coordinates(x, y, width, height, jx, jy):
    """u, v of pixels (x, y) with jitter (jx, jy) (float64): in double, then rounded to float."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    return ((x + jx) / width - 0.5).astype(F32), (-(y + jy) / height + 0.5).astype(F32)


def sign_from(x, s):
    """x with its sign bit flipped where s has its sign bit set."""
    x = np.ascontiguousarray(x, F32)
    s = np.ascontiguousarray(s, F32)
    return (x.view(np.uint32) ^ (s.view(np.uint32) & np.uint32(0x80000000))).view(F32)


def sincos_signed(angle):
    """(sin, cos) of a float angle with |angle| <= 2 pi: the portable pair of |angle|, the angle's sign put back on the sine."""
    angle = np.ascontiguousarray(angle, F32)
    s, c = V.sincos(np.abs(angle))
    return sign_from(s, angle), c


def rays_from_uv(u, v, camera, projection):
    """Origins and unit directions [n, 3] for image coordinates u, v [n] (float32) under `projection` = (kind, span_x, span_y)."""
    cam = np.asarray(V.REFERENCE_CAMERA if camera is None else camera, F32).reshape(4, 3)
    kind, span_x, span_y = int(projection[0]), F32(projection[1]), F32(projection[2])
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    n = len(u)
    o = np.broadcast_to(cam[0], (n, 3)).astype(F32).copy()
    if kind == PERSPECTIVE:
        D = (u[:, None] * cam[1] + v[:, None] * cam[2]) + cam[3]
    elif kind == ORTHOGRAPHIC:
        o = (cam[0] + (u[:, None] * cam[1] + v[:, None] * cam[2])).astype(F32)
        D = np.broadcast_to(cam[3], (n, 3)).astype(F32).copy()
    else:
        rh, uh, fh = V.lens_axes(cam)
        if kind == FISHEYE:
            a, b = u * span_x, v * span_y
            theta = np.sqrt(a * a + b * b)
            sn, cs = V.sincos(theta)
            with np.errstate(divide="ignore", invalid="ignore"):
                k = np.where(theta == 0, F32(1.0), sn / theta).astype(F32)
            wr, wu, wf = k * a, k * b, cs
        elif kind == EQUIRECTANGULAR:
            s_phi, c_phi = sincos_signed(u * span_x)
            s_psi, c_psi = sincos_signed(v * span_y)
            wr, wu, wf = c_psi * s_phi, s_psi, c_psi * c_phi
        else:
            raise ValueError(kind)
        D = (wr[:, None] * rh + wu[:, None] * uh) + wf[:, None] * fh
    return o.astype(F32), V.normalize3(D.astype(F32))


def primary_rays(x, y, width, height, words, camera, projection):
    """The primary rays of pixels (x, y) drawn with Philox words [n, 4] (words 0 and 1: the jitter)."""
    u, v = image_coordinates(x, y, width, height, V.jitter(words[:, 0]), V.jitter(words[:, 1]))
    return rays_from_uv(u, v, camera, projection)


def feature_rays(width, height, camera, projection):
    """The rays of the first-hit feature pass: every pixel of the frame, row-major, with jitter 0."""
    ys, xs = np.mgrid[0:height, 0:width]
    u, v = image_coordinates(xs.ravel(), ys.ravel(), width, height, 0.0, 0.0)
    return rays_from_uv(u, v, camera, projection)


def compose(scene, width, height, pixels, spp, mrr, *, camera=None, projection=(PERSPECTIVE, 0.0, 0.0), seed=42, eps=1e-4, error=-1.0,
            pass_begin=0):
    """sum [n, 3], sum2 [n, 3], count [n] of the frame's pixels `pixels` ([n, 2] of (x, y)) after passes pass_begin ..
    pass_begin + spp - 1, as the library accumulates them for `camera` (4 x 3; None = the reference's) under `projection`.
    view_composition.compose's loop, with the projected primary ray."""
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
        o, d = primary_rays(px[act, 0], px[act, 1], width, height, words, camera, projection)
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
