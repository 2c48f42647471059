"""The frame of ANY camera and lens, composed on the host from the CPU oracle's parts (a helper for the lens and camera tests).

The oracle renders only the reference's fixed view (orc_render), but it exposes every step of a path bit for bit: the counter
RNG (orc_probe_philox), its conversions (orc_probe_jitter, orc_probe_unit_float), the portable sine and cosine
(orc_probe_sincos), one Scene::TraceRay segment from a caller-supplied ray with caller-supplied words (orc_probe_segments) and
the adaptive-sampling test (orc_probe_adaptive_skip).  compose() chains them into the accumulators the library's kernels must
produce for a camera (pt_hip.h: pt_camera) and a thin lens (pt_lens), restating only the primary ray itself in numpy float32
(round to nearest, nothing fused -- as the library builds its kernels):

    u = float((x + jx) / W - 0.5),  v = float(-(y + jy) / H + 0.5)                      (in double, then rounded)
    D = (u right + v up) + forward                                                         (componentwise)
    lens:  rho = radius sqrt(unit(w2)),  (sn, cs) = sincos(2 * 3.141593f * unit(w3)),  L = (rho cs) r^ + (rho sn) u^,
           s = focus / ((D_x f^_x + D_y f^_y) + D_z f^_z),  origin = eye + L,  direction = normalize(D s - L)
    no lens: origin = eye,  direction = normalize(D)

The composition is pixel-local, as the counter RNG is: it can be evaluated for any subset of a frame's pixels.  It binds what
it needs through oracle_lib.lib() and changes nothing there."""
import ctypes as C

import numpy as np

import oracle_lib as O

PHILOX_KEY1 = 0x50544831   # the second key word of the counter RNG (pt_oracle.c: ORC_PHILOX_KEY1; pt_kernels.hip: kPhiloxKey1)
REFERENCE_CAMERA = np.array([[0, 0, -20], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
F32 = np.float32


def philox(pixel, pass_, c2, seed):
    """The four words of counter (pixel, pass, c2, 0) under key (seed, PHILOX_KEY1), one orc_probe_philox call per counter."""
    L = O.lib()
    pixel = np.asarray(pixel, np.uint32)
    pass_ = np.broadcast_to(np.asarray(pass_, np.uint32), pixel.shape)
    c2 = np.broadcast_to(np.asarray(c2, np.uint32), pixel.shape)
    key = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, PHILOX_KEY1)
    ctr, out = (C.c_uint32 * 4)(), (C.c_uint32 * 4)()
    words = np.zeros((len(pixel), 4), np.uint32)
    for i in range(len(pixel)):
        ctr[0], ctr[1], ctr[2], ctr[3] = int(pixel[i]), int(pass_[i]), int(c2[i]), 0
        L.orc_probe_philox(ctr, key, out)
        words[i] = out[0], out[1], out[2], out[3]
    return words


def unit_float(w):
    L = O.lib()
    return np.array([L.orc_probe_unit_float(int(x)) for x in np.asarray(w, np.uint32)], np.float32)


def jitter(w):
    L = O.lib()
    return np.array([L.orc_probe_jitter(int(x)) for x in np.asarray(w, np.uint32)], np.float64)


def sincos(a):
    a = np.ascontiguousarray(a, np.float32)
    s, c = np.zeros_like(a), np.zeros_like(a)
    O.lib().orc_probe_sincos(O._fp(a), len(a), O.TRIG_PORTABLE, O._fp(s), O._fp(c))
    return s, c


def normalize3(d):
    """glm's normalize as the library and the oracle compute it: d * (1 / sqrt((x x + y y) + z z)), in float."""
    n = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    inv = F32(1.0) / np.sqrt(n)
    return d * inv[:, None]


def lens_axes(camera):
    """r^, u^, f^: right, up, forward normalised in double and rounded to float once (pt_hip.h: pt_lens)."""
    cam = np.asarray(camera, np.float32).astype(np.float64)
    return (cam[1:] / np.linalg.norm(cam[1:], axis=1, keepdims=True)).astype(np.float32)


def primary_rays(x, y, width, height, words, camera=None, lens=None):
    """Origins and unit directions [n, 3] of the primary rays of pixels (x, y) drawn with Philox words [n, 4]."""
    cam = np.asarray(REFERENCE_CAMERA if camera is None else camera, np.float32).reshape(4, 3)
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    jx, jy = jitter(words[:, 0]), jitter(words[:, 1])
    u = ((x + jx) / width - 0.5).astype(np.float32)
    v = (-(y + jy) / height + 0.5).astype(np.float32)
    D = (u[:, None] * cam[1] + v[:, None] * cam[2]) + cam[3]
    o = np.broadcast_to(cam[0], D.shape).copy()
    if lens is not None and F32(lens[0]) > 0:
        radius, focus = F32(lens[0]), F32(lens[1])
        rh, uh, fh = lens_axes(cam)
        rho = radius * np.sqrt(unit_float(words[:, 2]))
        sn, cs = sincos(F32(2 * F32(3.141593)) * unit_float(words[:, 3]))
        pa, pb = rho * cs, rho * sn
        Lp = pa[:, None] * rh + pb[:, None] * uh
        s = focus / ((D[:, 0] * fh[0] + D[:, 1] * fh[1]) + D[:, 2] * fh[2])
        o = o + Lp
        D = D * s[:, None] - Lp
    return o.astype(np.float32), normalize3(D.astype(np.float32))


def compose(scene, width, height, pixels, spp, mrr, *, camera=None, lens=None, seed=42, eps=1e-4, error=-1.0, pass_begin=0):
    """sum [n, 3], sum2 [n, 3], count [n] of the frame's pixels `pixels` ([n, 2] of (x, y)) after passes pass_begin ..
    pass_begin + spp - 1, as the library accumulates them for `camera` (4 x 3: origin, right, up, forward; None = the
    reference's) and `lens` ((radius, focus distance); None = a pinhole).  `scene` is an oracle_lib.Scene (with its skybox, if
    the frame has one).  Contributions are added in pass order, as orc_render adds them."""
    px = np.asarray(pixels, np.int64).reshape(-1, 2)
    n = len(px)
    gpix = (px[:, 1] * width + px[:, 0]).astype(np.uint32)
    s, s2, cnt = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
    for p in range(pass_begin, pass_begin + spp):
        skip = O.adaptive_skip(np.full(n, p, np.int32), s, s2, cnt, error)
        act = np.nonzero(~skip)[0]
        if len(act) == 0:
            continue
        words = philox(gpix[act], p, 0xFFFFFFFF, seed)
        o, d = primary_rays(px[act, 0], px[act, 1], width, height, words, camera, lens)
        col = np.ones((len(act), 3), np.float32)
        depth = np.zeros(len(act), np.int32)
        live = np.arange(len(act))
        while len(live):
            w = philox(gpix[act[live]], p, depth[live], seed)[:, :3]
            o2, d2, c2, dep2, contrib, did = scene.segments(o[live], d[live], col[live], depth[live], w, eps=eps, mrr=mrr,
                                                            trig=O.TRIG_PORTABLE)
            o[live], d[live], col[live], depth[live] = o2, d2, c2, dep2
            k = act[live[did]]
            s[k] += contrib[did]
            s2[k] += contrib[did] * contrib[did]
            cnt[k] += 1
            live = live[(dep2 < mrr) & np.any(c2 != 0, axis=1)]
    return s, s2, cnt
